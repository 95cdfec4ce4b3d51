// The directed k-nearest-neighbour graph of the t-SNE, UMAP and spectral kernels, described once.
//   index (n, k)     edge e = i k + c runs from row i to index[e]: the forward edges of i, c its column.
//   rev_ptr (n + 1), the transpose (utils/graph.reverse_graph): the ids of the edges that end in i are
//   rev_edge (n k)   rev_edge[rev_ptr[i] : rev_ptr[i + 1]], ascending, so ascending by source row e / k too.
// n k < 2^31: edge ids are int32.  Every guard against a damaged graph lives in this file: a reverse range is clamped to
// 0 <= r0 <= r1 <= n k (one that is out of order is empty), edges that point outside [0, n) or at their own row and edge ids
// outside [0, n k) are passed over, so nothing that is read from the graph can address memory outside the tables.
//
// KnnEpochGraph adds the per-edge tables umap_union writes, and the INCIDENT LIST of a vertex, the pairs the UMAP epochs and
// the spectral start work on: its forward edges, then the edges of its reverse range with mutual = 0 (no opposite edge:
// a mutual pair is listed once, at each end, as a forward edge).  An entry's SLOT feeds Philox: a forward edge's is its column,
// the lone reverse edges take k, k + 1, ... in list order.  Edges the schedule pruned (eps = +inf) are listed and numbered;
// they never fire, and the spectral kernels pass them over.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct KnnGraph {
    const int* index;
    const int* rev_ptr;       // may be null (with rev_edge) for a kernel that reads forward edges only
    const int* rev_edge;
    int n, k;

    struct Range { int r0, r1; };

    __host__ __device__ bool complete() const { return index && rev_ptr && rev_edge; }
    __device__ __forceinline__ long ne() const { return (long)n * k; }

    // the part of rev_edge that holds the edges ending in i: 0 <= r0 <= r1 <= ne() whatever rev_ptr holds
    __device__ __forceinline__ Range rev_range(int i) const {
        int r0 = rev_ptr[i], r1 = rev_ptr[i + 1];
        r0 = r0 < 0 ? 0 : r0;
        r1 = r1 > ne() ? (int)ne() : r1;
        r1 = r1 < r0 ? r0 : r1;
        return Range{r0, r1};
    }
    // forward edge e of row i: its other end j; false for an edge to pass over
    __device__ __forceinline__ bool forward(int i, long e, int& j) const {
        j = index[e];
        return j >= 0 && j < n && j != i;
    }
    // entry r of a clamped reverse range: the edge e2; false for an id to pass over.  source(e2) is the row it comes from
    // (a division: asked for only where it is needed)
    __device__ __forceinline__ bool reverse(long r, int& e2) const {
        e2 = rev_edge[r];
        return e2 >= 0 && e2 < ne();
    }
    __device__ __forceinline__ int source(int e2) const { return e2 / k; }
    // the id of the edge j -> i, or -1: the first entry of i's reverse range whose source row is not below j
    __device__ __forceinline__ int opposite(int i, int j) const {
        const Range rr = rev_range(i);
        int lo = rr.r0, hi = rr.r1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (rev_edge[mid] / k < j) lo = mid + 1; else hi = mid;
        }
        int e2;
        return lo < rr.r1 && reverse(lo, e2) && source(e2) == j ? e2 : -1;
    }
};

struct KnnEpochGraph : KnnGraph {
    const uint8_t* mutual;    // the opposite edge exists
    const double* eps;        // the edge's spacing in epochs, +inf for a pruned edge

    // what a lane holds of one batch of the incident list; j, e and slot mean something where `has`.  The slot is numbered
    // for every user (a ballot and two popcounts per reverse batch), also for the spectral kernels, which do not read it
    struct Entry { bool has; int j; long e; int slot; };

    __host__ __device__ bool complete() const { return KnnGraph::complete() && mutual && eps; }

    // Called by a whole wave: f(entry) once per batch of 64 list positions of vertex i - the forward columns, then the reverse
    // range - so lane l owns positions l, l + 64, ... of each, and all forward entries come before all reverse ones.  The trip
    // count is the same in every lane: f may ballot and (in a one-wave workgroup) use barriers.
    template <typename F>
    __device__ __forceinline__ void for_incident(int i, int lane, F&& f) const {
        for (int c0 = 0; c0 < k; c0 += 64) {
            Entry t{false, 0, 0, c0 + lane};
            if (t.slot < k) {
                t.e = (long)i * k + t.slot;
                t.has = forward(i, t.e, t.j);
            }
            f(t);
        }
        const Range rr = rev_range(i);
        const unsigned long long below_me = (1ull << lane) - 1ull;
        int slot0 = k;
        for (unsigned rb = rr.r0; rb < (unsigned)rr.r1; rb += 64) {        // 0 <= r0 <= r1; unsigned: r1 may lie within 64 of 2^31
            Entry t{false, 0, 0, 0};
            bool lone = false;
            int e2;
            if (rb + lane < (unsigned)rr.r1 && reverse(rb + lane, e2) && !mutual[e2]) {
                lone = true;
                t.e = e2;
                t.j = source(e2);
                t.has = t.j != i;
            }
            const unsigned long long lm = __ballot(lone);
            t.slot = slot0 + (int)__popcll(lm & below_me);
            slot0 += (int)__popcll(lm);
            f(t);
        }
    }
};

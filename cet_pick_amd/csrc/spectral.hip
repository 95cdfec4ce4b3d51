// The spectral start of the UMAP map (umap.UMAP's init="spectral"), DESIGN.md 4.15: the eigen-solver's kernels over the graph the
// epochs use.  The incident list of vertex i is the one of knn_graph.h, walked by the walker um_epoch_kernel uses, without the
// edges the schedule pruned (eps = +inf); the weight of an entry is wsym of that directed edge.
//   components  one wave per vertex, one launch = one sweep from label_in to label_out: the smallest label among the vertex and its
//               incident vertices, then pointer jumping through label_in down to a vertex that is its own label.  `changed` is set
//               to 1 by every vertex whose label moved.  Labels are vertex ids and never grow, so the fixed point - every vertex
//               carrying the smallest id of its component - is unique, and with two buffers every sweep is a pure function of the
//               one before.
//   degree      one wave per vertex: deg = the sum of the incident weights in double, dis = 1 / sqrt(deg) (0 for deg = 0).
//   spmv        one wave per row of [row0, row0 + nrows): y = dis_i sum_j w_ij (dis_j x_j), A = D^-1/2 W D^-1/2 restricted to the
//               range (entries that leave it are passed over); x and y are the range's own vectors, nrows doubles.
//   dots        c = Q^T w for m vectors of length n (vector v at Q + v ldq): one workgroup per (2048-element chunk, vector), the
//               chunks' partial sums added in chunk order by one thread per vector.
//   update      w = beta w - Q c, one thread per element, the vectors in order.
// Every sum is taken in double in a fixed order: lanes stride, a fixed butterfly, waves and chunks in index order.  No
// floating-point atomics: the same inputs give the same bytes.
#include "common.h"
#include "knn_graph.h"
#include "../../include/cetpick_hip.h"

namespace {

constexpr int SP_CHUNK = 2048, SP_MMAX = 4096;

inline long sp_chunks(long n) { return (n + SP_CHUNK - 1) / SP_CHUNK; }

inline int sp_vec_check(int m, long n, long ldq) {
    if (m < 1 || m > SP_MMAX || n < 1 || n >= (1l << 31) || ldq < n) return MI_E_UNSUPPORTED;
    return MI_OK;
}

// f(j, e) for every entry of vertex i's incident list that this lane owns and the schedule kept: other end j, directed edge e.
template <typename F>
__device__ __forceinline__ void sp_for_incident(const KnnEpochGraph& g, int i, int lane, F&& f) {
    g.for_incident(i, lane, [&](const KnnEpochGraph::Entry& t) __attribute__((always_inline)) {
        if (t.has && g.eps[t.e] < (double)INFINITY) f(t.j, t.e);
    });
}

__global__ __launch_bounds__(256) void sp_components_kernel(KnnEpochGraph g, const int* label_in, int* label_out, int* changed) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= g.n) return;                                // (wave-uniform)
    const int i = (int)row, was = label_in[i];
    int best = (was < 0 || was >= g.n) ? i : was;
    sp_for_incident(g, i, lane, [&](int j, long) {
        const int l = label_in[j];
        if (l >= 0 && l < best) best = l;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
    if (lane == 0) {
        for (;;) {                                         // pointer jumping: the labels fall strictly, so this ends
            const int p = label_in[best];
            if (p < 0 || p >= best) break;
            best = p;
        }
        label_out[i] = best;
        if (best != was) *changed = 1;
    }
}

__global__ __launch_bounds__(256) void sp_degree_kernel(KnnEpochGraph g, const float* wsym, double* deg, double* dis) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= g.n) return;
    double acc = 0.0;
    sp_for_incident(g, (int)row, lane, [&](int, long e) { acc += (double)wsym[e]; });
    acc = wave_sum(acc);
    if (lane == 0) {
        deg[row] = acc;
        dis[row] = acc > 0.0 ? 1.0 / sqrt(acc) : 0.0;
    }
}

__global__ __launch_bounds__(256) void sp_spmv_kernel(KnnEpochGraph g, const float* wsym, const double* dis, const double* __restrict__ x,
                                                      double* __restrict__ y, int row0, int nrows) {
    const long local = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (local >= nrows) return;
    const int i = row0 + (int)local, row1 = row0 + nrows;
    double acc = 0.0;
    sp_for_incident(g, i, lane, [&](int j, long e) {
        if (j >= row0 && j < row1) acc += (double)wsym[e] * (dis[j] * x[j - row0]);
    });
    acc = wave_sum(acc);
    if (lane == 0) y[local] = dis[i] * acc;
}

__global__ __launch_bounds__(256) void sp_dots_kernel(const double* Q, long ldq, const double* w, long n, double* part, int chunks) {
    __shared__ double s[4];
    const int v = blockIdx.y, p = blockIdx.x;
    const long i0 = (long)p * SP_CHUNK, i1 = i0 + SP_CHUNK < n ? i0 + SP_CHUNK : n;
    const double* q = Q + (size_t)v * ldq;
    double acc = 0.0;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) acc += q[i] * w[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)v * chunks + p] = (s[0] + s[1]) + (s[2] + s[3]);
}

__global__ __launch_bounds__(256) void sp_dots_final_kernel(const double* part, int m, int chunks, double* c) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= m) return;
    double acc = 0.0;
    for (int p = 0; p < chunks; ++p) acc += part[(size_t)v * chunks + p];
    c[v] = acc;
}

__global__ __launch_bounds__(256) void sp_update_kernel(const double* __restrict__ Q, long ldq, int m, long n, const double* __restrict__ c,
                                                        double* w, double beta) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
#pragma unroll 4
    for (int v = 0; v < m; ++v) acc += Q[(size_t)v * ldq + i] * c[v];
    w[i] = (beta == 0.0 ? 0.0 : beta * w[i]) - acc;
}

inline int sp_dots(const double* Q, long ldq, int m, long n, const double* w, double* c, void* ws, size_t ws_bytes, hipStream_t stream) {
    const long chunks = sp_chunks(n);
    if (ws_bytes < (size_t)m * chunks * sizeof(double)) return MI_E_WORKSPACE;
    double* part = (double*)ws;
    hipLaunchKernelGGL(sp_dots_kernel, dim3((unsigned)chunks, (unsigned)m), dim3(256), 0, stream, Q, ldq, w, n, part, (int)chunks);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(sp_dots_final_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, part, m, (int)chunks, c);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

inline bool sp_inside(const double* p, const double* Q, long ldq, int m) { return p >= Q && p < Q + (size_t)m * ldq; }

}  // namespace

extern "C" int mi_graph_components(const int32_t* index, const double* eps, const uint8_t* mutual, const int32_t* rev_ptr,
                                   const int32_t* rev_edge, long n, int k, const int32_t* label_in, int32_t* label_out, int32_t* changed,
                                   mi_stream_t stream) {
    const KnnEpochGraph g{{index, rev_ptr, rev_edge, (int)n, k}, mutual, eps};
    if (!g.complete() || !label_in || !label_out || label_in == label_out || !changed) return MI_E_ARG;
    const int rc = mi_umap_check(n, k);
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(sp_components_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, label_in, label_out,
                       changed);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_spectral_degree(const int32_t* index, const float* wsym, const double* eps, const uint8_t* mutual, const int32_t* rev_ptr,
                                  const int32_t* rev_edge, long n, int k, double* out_deg, double* out_dis, mi_stream_t stream) {
    const KnnEpochGraph g{{index, rev_ptr, rev_edge, (int)n, k}, mutual, eps};
    if (!g.complete() || !wsym || !out_deg || !out_dis) return MI_E_ARG;
    const int rc = mi_umap_check(n, k);
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(sp_degree_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, wsym, out_deg, out_dis);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_spectral_spmv(const int32_t* index, const float* wsym, const double* eps, const uint8_t* mutual, const int32_t* rev_ptr,
                                const int32_t* rev_edge, long n, int k, const double* dis, const double* x, double* y, long row0,
                                long nrows, mi_stream_t stream) {
    const KnnEpochGraph g{{index, rev_ptr, rev_edge, (int)n, k}, mutual, eps};
    if (!g.complete() || !wsym || !dis || !x || !y || x == y) return MI_E_ARG;
    const int rc = mi_umap_check(n, k);
    if (rc != MI_OK) return rc;
    if (row0 < 0 || nrows < 1 || row0 + nrows > n) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(sp_spmv_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, wsym, dis, x, y, (int)row0,
                       (int)nrows);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" size_t mi_spectral_workspace_bytes(int m, long n) {
    if (sp_vec_check(m, n, n) != MI_OK) return 0;
    return (size_t)m * sp_chunks(n) * sizeof(double);
}

extern "C" int mi_spectral_dots(const double* Q, long ldq, int m, long n, const double* w, double* c, void* ws, size_t ws_bytes,
                                mi_stream_t stream) {
    if (!Q || !w || !c || !ws) return MI_E_ARG;
    const int rc = sp_vec_check(m, n, ldq);
    if (rc != MI_OK) return rc;
    return sp_dots(Q, ldq, m, n, w, c, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int mi_spectral_orth(const double* Q, long ldq, int m, long n, double* w, double* c, void* ws, size_t ws_bytes,
                                mi_stream_t stream) {
    if (!Q || !w || !c || !ws) return MI_E_ARG;
    int rc = sp_vec_check(m, n, ldq);
    if (rc != MI_OK) return rc;
    if (sp_inside(w, Q, ldq, m)) return MI_E_ARG;
    rc = sp_dots(Q, ldq, m, n, w, c, ws, ws_bytes, (hipStream_t)stream);
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(sp_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Q, ldq, m, n, c, w, 1.0);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_spectral_combine(const double* Q, long ldq, int m, long n, const double* c, double* w, double beta, mi_stream_t stream) {
    if (!Q || !w || !c) return MI_E_ARG;
    const int rc = sp_vec_check(m, n, ldq);
    if (rc != MI_OK) return rc;
    if (sp_inside(w, Q, ldq, m)) return MI_E_ARG;
    hipLaunchKernelGGL(sp_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Q, ldq, m, n, c, w, beta);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

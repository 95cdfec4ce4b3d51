// Exact k-nearest-neighbour search over embeddings (reference utils/memory_bank.py: faiss.IndexFlatIP / matmul + topk),
// DESIGN.md 4.11.  Queries q (M, d), database x (N, d), 1 <= k <= 128: the k best database rows of every query, best first.
//   prep    database -> the operand image of rowdot.h: its bf16x3 cut in B-fragment order + |x_j|^2, 0 for the columns
//           that pad N to 32 (the search never takes such a column)                                       (once per search)
//   search  a workgroup owns 64 queries (32 when the LDS bill of 64 passes 160 KB; their cut staged once in LDS) and one split
//           of the column tiles.  The M x N x d product runs on v_mfma_f32_32x32x16_bf16 in the library's bf16x3 arithmetic
//           (bf16x3.h) through the row-product tile of rowdot.h, which kmeans.hip shares.  The similarity
//           matrix is never written: every query row has a sorted top-k list in LDS, the list's last entry is the row's
//           threshold, and only accumulator entries that beat it are inserted.  Every split writes its lists.
//   merge   one workgroup per query: the rank of every partial entry among all partials of the row, lists visited in split
//           order; ranks < k are the result.
// Order: keys are "larger is better" (q.x, or 2 q.x - |x|^2 for squared L2: the exact negative of |x|^2 - 2 q.x, so the
// squared L2 distance to the nearest row and the dist of kmeans_assign are the same bytes), and (key, lower index) is a
// strict total order on the columns of a row.  The top k of a total order do not depend on the order in which candidates
// arrive or on how the columns are split, and the key of a (row, column) pair is one fixed MFMA chain: no floating-point
// atomics, same inputs -> same bytes, for any split count.  A NaN key counts as -inf.
// Rows are addressed with 64-bit offsets throughout (N x d may exceed 2 GiB); M, N < 2^31.
// hipcc-flags: -fno-slp-vectorize
#include "common.h"
#include "rowdot.h"
#include "../../include/cetpick_hip.h"

namespace {

using namespace bf3;        // the bf16x3 arithmetic, its types and helpers: bf16x3.h

constexpr int KNN_DMAX = 512, KNN_KMAX = 128, KNN_SMAX = 32;
constexpr int KNN_LDS_MAX = 160 * 1024;  // one workgroup may take the CU's whole LDS
constexpr int KNN_NONE = 0x7fffffff;     // index of a list entry that holds no column (key -inf): loses every tie

// (v2, i2) comes before (v, i): larger key, lowest index on ties
__device__ __forceinline__ bool knn_before(float v2, int i2, float v, int i) { return v2 > v || (v2 == v && i2 < i); }

// The whole wave puts (cv, cc) into the sorted list (lv, li) of k entries, if it comes before the list's last entry.
// Entry e is held by lane e & 63; the entries that come before the candidate are a prefix, so its place is their number.
__device__ __forceinline__ void knn_insert(float* lv, int* li, int k, int lane, float cv, int cc) {
    const int e0 = lane, e1 = lane + 64;
    float v0 = 0.f, p0 = 0.f, v1 = 0.f, p1 = 0.f;
    int i0 = 0, q0 = 0, i1 = 0, q1 = 0;
    if (e0 < k) { v0 = lv[e0]; i0 = li[e0]; }
    if (e0 < k && e0 > 0) { p0 = lv[e0 - 1]; q0 = li[e0 - 1]; }
    int place = __builtin_popcountll(__ballot(e0 < k && knn_before(v0, i0, cv, cc)));
    if (k > 64) {                                          // (uniform)
        if (e1 < k) { v1 = lv[e1]; i1 = li[e1]; p1 = lv[e1 - 1]; q1 = li[e1 - 1]; }
        place += __builtin_popcountll(__ballot(e1 < k && knn_before(v1, i1, cv, cc)));
    }
    if (place >= k) return;                                // (uniform) an earlier candidate has raised the threshold
    // Every lane's reads of the list come before any lane's writes (lane 0 reads entry 63, which lane 63 writes).  A wave's
    // LDS operations execute in program order; the fence keeps the compiler from moving a read below a write, which for one
    // thread alone do not alias.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (e0 < k && e0 >= place) { lv[e0] = e0 == place ? cv : p0; li[e0] = e0 == place ? cc : q0; }
    if (k > 64 && e1 < k && e1 >= place) { lv[e1] = e1 == place ? cv : p1; li[e1] = e1 == place ? cc : q1; }
}

// LDS: three planes of the queries' cut (rowdot.h), the lists' keys [RT][k] and indices [RT][k], and two sets of four
// flags.  The four waves share the rows; in step t wave w takes column tile
// ct0 + 4 t + w of the split.  A step: the products; the filter against the lists' last entries (nobody writes a list
// then); one barrier; then the waves that found candidates insert them one wave after the other, a barrier behind each, so a
// list has one writer at a time.  Once the lists have filled, most steps find nothing and cost the one barrier.
template <int RM>
__global__ __launch_bounds__(256) void knn_search_kernel(const float* q, const unsigned char* img, const float* xnorm, long M, long N,
                                                         int d, int KS, long KT, long tps, int k, int l2, int excl, float* pval,
                                                         int* pidx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    constexpr int RT = 32 * RM;
    float* lv = reinterpret_cast<float*>(knn_lds + 3 * RT * rowdot::lds_pitch(KS));
    int* li = reinterpret_cast<int*>(lv + RT * k);
    int* has = li + RT * k;                                // [2][4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const long row0 = (long)blockIdx.x * RT;
    const long ct0 = (long)blockIdx.y * tps, ct1 = ct0 + tps < KT ? ct0 + tps : KT;

    rowdot::stage_rows<RM>(knn_lds, q, row0, M, d, KS, tid);
    for (int s = tid; s < RT * k; s += 256) { lv[s] = -INFINITY; li[s] = KNN_NONE; }
    __syncthreads();

    const long steps = (ct1 - ct0 + 3) / 4;
    for (long t = 0; t < steps; ++t) {
        const long ct = ct0 + t * 4 + wave;
        const bool live = ct < ct1;                        // (wave-uniform) the last step of a split may be short
        f32x16 acc[RM];
        unsigned cand[RM];
#pragma unroll
        for (int m = 0; m < RM; ++m) cand[m] = 0u;
        const long col = ct * 32 + l32;
        if (live) {
            rowdot::tile_product<RM>(acc, knn_lds, img, ct, KS, lane, h, l32);
            const float cn = l2 ? xnorm[col] : 0.f;        // xnorm has KT 32 entries
            const bool colok = col < N;
#pragma unroll
            for (int m = 0; m < RM; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int tr = rowdot::acc_row(m, r, h);
                    float key = l2 ? fmaf(2.f, acc[m][r], -cn) : acc[m][r];
                    key = key == key ? key : -INFINITY;
                    acc[m][r] = key;
                    const bool ok = colok && row0 + tr < M && !(excl && col == row0 + tr) &&
                                    knn_before(key, (int)col, lv[tr * k + k - 1], li[tr * k + k - 1]);
                    cand[m] |= (ok ? 1u : 0u) << r;
                }
        }
        bool any = false;
#pragma unroll
        for (int m = 0; m < RM; ++m) any = any || cand[m] != 0u;
        const bool wave_any = __ballot(any) != 0ull;
        int* flag = has + (int)(t & 1) * 4;                // this set is next written two steps on, behind a barrier all passed
        if (lane == 0) flag[wave] = wave_any ? 1 : 0;
        __syncthreads();
        const int f0 = flag[0], f1 = flag[1], f2 = flag[2], f3 = flag[3];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int fw = w == 0 ? f0 : w == 1 ? f1 : w == 2 ? f2 : f3;
            if (!fw) continue;                             // (workgroup-uniform)
            if (wave == w) {
#pragma unroll
                for (int m = 0; m < RM; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        unsigned long long mask = __ballot((cand[m] >> r) & 1u);
                        while (mask) {                     // (wave-uniform)
                            const int src = __builtin_ctzll(mask);
                            mask &= mask - 1;
                            const float cv = __shfl(acc[m][r], src, 64);
                            const int tr = rowdot::acc_row(m, r, src >> 5);
                            knn_insert(lv + tr * k, li + tr * k, k, lane, cv, (int)(ct * 32 + (src & 31)));
                        }
                    }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int s = tid; s < RT * k; s += 256) {
        const int r = s / k;
        if (row0 + r < M) {
            const size_t o = ((size_t)blockIdx.y * M + row0 + r) * k + (s - r * k);
            pval[o] = lv[s];
            pidx[o] = li[s];
        }
    }
}

// One workgroup per query.  Its S sorted partial lists go to LDS; the rank of an entry is the number of entries of all lists
// that come before it (a binary search per list, lists in split order; in its own list, its position).  Entries that hold
// no column rank behind every column, and there are at least k columns.  value = key, or max(0, |q|^2 + (|x|^2 - 2 q.x)).
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* q, const float* pval, const int* pidx, long M, int d, int k, int S,
                                                        int l2, int* oidx, float* oval) {
    __shared__ float mv[KNN_SMAX * KNN_KMAX];
    __shared__ int mi[KNN_SMAX * KNN_KMAX];
    __shared__ float qn_s;
    const long row = blockIdx.x;
    const int tid = threadIdx.x;
    for (int e = tid; e < S * k; e += 256) {
        const int s = e / k;
        const size_t o = ((size_t)s * M + row) * k + (e - s * k);
        mv[e] = pval[o];
        mi[e] = pidx[o];
    }
    if (tid < 64) {
        const float s = l2 ? rowdot::row_sqnorm(q + (size_t)row * d, d, tid) : 0.f;
        if (tid == 0) qn_s = s;
    }
    __syncthreads();
    const float qn = qn_s;
    for (int e = tid; e < S * k; e += 256) {
        const float v = mv[e];
        const int i = mi[e];
        if (i == KNN_NONE) continue;
        const int own = e / k;
        int rank = e - own * k;
        for (int s = 0; s < S && rank < k; ++s) {
            if (s == own) continue;
            int lo = 0, hi = k;                            // the number of entries of list s that come before (v, i)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (knn_before(mv[s * k + mid], mi[s * k + mid], v, i)) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            oidx[(size_t)row * k + rank] = i;
            oval[(size_t)row * k + rank] = l2 ? fmaxf(0.f, qn + (-v)) : v;
        }
    }
}

inline int knn_check(long m, long n, int d, int k, int excl, int n_split) {
    if (d < 1 || d > KNN_DMAX || k < 1 || k > KNN_KMAX || m < 1 || m >= (1l << 31) || n >= (1l << 31) || n < (long)k + (excl ? 1 : 0) ||
        n_split < 0 || n_split > KNN_SMAX)
        return MI_E_UNSUPPORTED;
    return MI_OK;
}
inline size_t knn_lds_bytes(int rt, int d, int k) {
    return rowdot::lds_planes_bytes(rt, rowdot::shape(0, d).KS) + (size_t)rt * k * 8 + 32;
}
inline int knn_rows_per_wg(int d, int k) { return knn_lds_bytes(64, d, k) <= (size_t)KNN_LDS_MAX ? 64 : 32; }
struct KnnPlan { int rt, S; long tps, rtiles; };
// Splits: enough workgroups for two rounds over the chip's 256 CUs, at least eight column tiles each; a forced count is
// taken as it is (no more splits than tiles).  tps = column tiles per split.
inline KnnPlan knn_plan(long m, long n, int d, int k, int n_split) {
    KnnPlan p;
    p.rt = knn_rows_per_wg(d, k);
    p.rtiles = (m + p.rt - 1) / p.rt;
    const long KT = rowdot::shape(n, d).KT;
    long S = n_split;
    if (S == 0) {
        S = (512 + p.rtiles - 1) / p.rtiles;
        const long most = KT / 8 > 1 ? KT / 8 : 1;
        if (S > most) S = most;
        if (S > KNN_SMAX) S = KNN_SMAX;
    }
    if (S > KT) S = KT;
    p.tps = (KT + S - 1) / S;
    p.S = (int)((KT + p.tps - 1) / p.tps);
    return p;
}
struct KnnWs { size_t image, xnorm, pval, pidx, total; };
inline KnnWs knn_ws(long m, long n, int d, int k, int n_split) {
    const KnnPlan p = knn_plan(m, n, d, k, n_split);
    KnnWs w;
    size_t o = 0;
    w.image = o; o += mi_align_up(rowdot::planes_bytes(n, d), 256);
    w.xnorm = o; o += mi_align_up((size_t)rowdot::shape(n, d).KT * 32 * 4, 256);
    w.pval = o; o += mi_align_up((size_t)p.S * m * k * 4, 256);
    w.pidx = o; o += mi_align_up((size_t)p.S * m * k * 4, 256);
    w.total = o;
    return w;
}

}  // namespace

extern "C" size_t mi_knn_image_bytes(long n, int d) {
    if (d < 1 || d > KNN_DMAX || n < 1 || n >= (1l << 31)) return 0;
    return rowdot::image_bytes(n, d);
}

extern "C" size_t mi_knn_workspace_bytes(long m, long n, int d, int k, int exclude_self, int n_split) {
    if (knn_check(m, n, d, k, exclude_self, n_split) != MI_OK) return 0;
    return knn_ws(m, n, d, k, n_split).total;
}

extern "C" int mi_knn_search(const float* q, const float* x, long m, long n, int d, int k, int metric, int exclude_self, int n_split,
                             int32_t* out_index, float* out_value, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!q || !x || !out_index || !out_value || !ws) return MI_E_ARG;
    if (metric != MI_KNN_IP && metric != MI_KNN_L2) return MI_E_ARG;
    const int rc = knn_check(m, n, d, k, exclude_self, n_split);
    if (rc != MI_OK) return rc;
    if (((uintptr_t)ws & 15) || ((((uintptr_t)x | (uintptr_t)q) & 15) && !(d & 3))) return MI_E_ARG;
    const KnnWs w = knn_ws(m, n, d, k, n_split);
    if (ws_bytes < w.total) return MI_E_WORKSPACE;
    const KnnPlan p = knn_plan(m, n, d, k, n_split);
    const rowdot::Shape s = rowdot::shape(n, d);
    unsigned char* b = (unsigned char*)ws;
    unsigned char* img = b + w.image;
    float* xnorm = (float*)(b + w.xnorm);
    float* pval = (float*)(b + w.pval);
    int* pidx = (int*)(b + w.pidx);
    hipStream_t st = (hipStream_t)stream;
    static std::atomic<bool> lds_allowed[64];
    const int ra = mi_allow_dynamic_lds(lds_allowed, KNN_LDS_MAX, knn_search_kernel<2>, knn_search_kernel<1>);
    if (ra != MI_OK) return ra;
    hipLaunchKernelGGL(rowdot::prep_kernel, dim3((unsigned)(s.KT * 8)), dim3(256), 0, st, x, n, d, s.KS, 0.f, img, xnorm);
    const size_t lds = knn_lds_bytes(p.rt, d, k);
    const dim3 grid((unsigned)p.rtiles, (unsigned)p.S);
    const int l2 = metric == MI_KNN_L2, excl = exclude_self != 0;
    if (p.rt == 64)
        hipLaunchKernelGGL(knn_search_kernel<2>, grid, dim3(256), lds, st, q, img, xnorm, m, n, d, s.KS, s.KT, p.tps, k, l2, excl, pval, pidx);
    else
        hipLaunchKernelGGL(knn_search_kernel<1>, grid, dim3(256), lds, st, q, img, xnorm, m, n, d, s.KS, s.KT, p.tps, k, l2, excl, pval, pidx);
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)m), dim3(256), 0, st, q, pval, pidx, m, d, k, p.S, l2, out_index, out_value);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

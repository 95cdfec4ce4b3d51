// How good a clustering of the picks is: the exact silhouette (scikit-learn's silhouette_samples, Euclidean) and the contingency
// table of two labelings, DESIGN.md 4.28.  The reference has no counterpart.
//   mi_silhouette_sums      S[i][c] = sum over the members j != i of fine cluster c of |x_i - x_j|, float64, in ONE pass over the
//                           n x n pairs on the row-product tile of rowdot.h (what knn.hip and kmeans.hip run on):
//     count   members per fine cluster (integer atomics)
//     scan    one workgroup: per cluster its first column among the sorted picks, its first column tile (every cluster padded
//             to whole tiles of 32 columns, so a tile belongs to one cluster) and its first chunk (chunks of CH tiles)
//     prep    one wave per sorted position: the pick's bf16x3 cut into its column of the operand image, |x_j|^2, the pick's
//             index (-1 stays in the columns that pad a cluster); and |x_i|^2 of row i as knn_merge_kernel forms it
//     pairs   a workgroup stages the cut of 64 rows (32 where that passes 160 KB) in LDS; each of its four waves takes one chunk
//             of one cluster: per tile the products, d2 = |x_i|^2 + (|x_j|^2 - 2 x_i.x_j) exactly as knn.hip's l2 value, the
//             float64 square root, masked by index where the column pads or IS the row; a lane adds its column's distances
//             tile after tile, the 32 lanes of a row are added in a fixed tree, one partial per (row, chunk)
//     sum     S[i][c] = the partials of cluster c's chunks in ascending order
//   mi_silhouette_finalise  class sums from S (a merged class = its fine columns in ascending index), a, b, s, nearest per pick,
//                           per-class and overall means (chunk sums in pick order, chunks in ascending order), the confusion
//                           table.  float64 throughout.
//   mi_label_contingency    counts of (a_i, b_i), integer atomics.
// Nothing floating is added by an atomic and every order above is fixed by (n, d, k) and the labels: same input, same bytes.
// Offsets into x, the image, the partials and S are 64-bit.
// hipcc-flags: -fno-slp-vectorize
#include "common.h"
#include "rowdot.h"
#include "../../include/cetpick_hip.h"

namespace {

using namespace bf3;

constexpr int SIL_DMAX = 512, SIL_KMAX = 1024, SIL_CMAX = 1024;
constexpr int SIL_CH_MIN = 32;            // column tiles per chunk, at least
constexpr int SIL_LDS_MAX = 160 * 1024;
constexpr int SIL_ROWS = 256;             // picks per partial sum of the finalise step
constexpr long SIL_GRID = 1l << 20;       // workgroups of a grid-stride launch, at most

inline bool sil_sizes_ok(long n, int d, int k) { return n >= 2 && n < (1l << 31) && d >= 1 && d <= SIL_DMAX && k >= 1 && k <= SIL_KMAX; }

struct SilPlan {
    int rt, CH;          // rows per workgroup, tiles per chunk
    long rtiles, KT, Q;  // row tiles; column tiles and chunks, at most (Q is the pitch of the partials)
};
// sum over clusters of ceil(n_c / 32) <= n / 32 + k, of ceil(t_c / CH) <= KT / CH + k
inline SilPlan sil_plan(long n, int d, int k) {
    SilPlan p;
    p.rt = rowdot::lds_planes_bytes(64, rowdot::shape(0, d).KS) <= (size_t)SIL_LDS_MAX ? 64 : 32;
    p.rtiles = (n + p.rt - 1) / p.rt;
    p.KT = n / 32 + k;
    const long ch = (p.KT + 63) / 64;
    p.CH = (int)(ch > SIL_CH_MIN ? ch : SIL_CH_MIN);
    p.Q = p.KT / p.CH + k;
    return p;
}

struct SilWs { size_t image, cnorm, colpick, rnorm, counts, col0, tile0, chunk0, part, total; };
inline SilWs sil_ws(long n, int d, int k) {
    const SilPlan p = sil_plan(n, d, k);
    const int KS = rowdot::shape(0, d).KS;
    SilWs w;
    size_t o = 0;
    w.image = o; o += mi_align_up((size_t)p.KT * KS * 3 * 1024, 256);
    w.cnorm = o; o += mi_align_up((size_t)p.KT * 32 * 4, 256);
    w.colpick = o; o += mi_align_up((size_t)p.KT * 32 * 4, 256);
    w.rnorm = o; o += mi_align_up((size_t)n * 4, 256);
    w.counts = o; o += mi_align_up((size_t)k * 4, 256);
    w.col0 = o; o += mi_align_up((size_t)(k + 1) * 4, 256);
    w.tile0 = o; o += mi_align_up((size_t)(k + 1) * 4, 256);
    w.chunk0 = o; o += mi_align_up((size_t)(k + 1) * 4, 256);
    w.part = o; o += mi_align_up((size_t)n * p.Q * 8, 256);
    w.total = o;
    return w;
}

inline unsigned sil_blocks(long items, int per_block) {
    const long b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > SIL_GRID ? SIL_GRID : b);
}

// counts[c] = picks with label c, c in [0, k); any other label is left out
__global__ __launch_bounds__(256) void label_count_kernel(const int* __restrict__ labels, long n, int k, int* __restrict__ counts) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int c = labels[i];
        if ((unsigned)c < (unsigned)k) atomicAdd(&counts[c], 1);
    }
}

// one workgroup: exclusive prefix sums of the counts, of their tiles of 32 and of their chunks of CH tiles, entries 0..k
__global__ __launch_bounds__(256) void sil_scan_kernel(const int* __restrict__ counts, int k, int CH, int* __restrict__ col0,
                                                       int* __restrict__ tile0, int* __restrict__ chunk0) {
    __shared__ int cnt[SIL_KMAX];
    for (int c = threadIdx.x; c < k; c += 256) cnt[c] = counts[c];
    __syncthreads();
    if (threadIdx.x == 0) {
        int col = 0, tile = 0, chunk = 0;
        for (int c = 0; c < k; ++c) {
            col0[c] = col; tile0[c] = tile; chunk0[c] = chunk;
            const int t = (cnt[c] + 31) >> 5;
            col += cnt[c]; tile += t; chunk += (t + CH - 1) / CH;
        }
        col0[k] = col; tile0[k] = tile; chunk0[k] = chunk;
    }
}

// wave p: the pick at sorted position p into its column; and the squared norm of ROW p
__global__ __launch_bounds__(256) void sil_prep_kernel(const float* __restrict__ x, const int* __restrict__ labels,
                                                       const int* __restrict__ order, long n, int d, int KS, int k,
                                                       const int* __restrict__ col0, const int* __restrict__ tile0,
                                                       unsigned char* __restrict__ img, float* __restrict__ cnorm,
                                                       int* __restrict__ colpick, float* __restrict__ rnorm) {
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= n) return;                                    // (wave-uniform)
    const float rs = rowdot::row_sqnorm(x + (size_t)p * d, d, lane);
    if (lane == 0) rnorm[p] = rs;
    const int pick = order[p];
    if ((unsigned)pick >= (unsigned long)n) return;
    const int c = labels[pick];
    if ((unsigned)c >= (unsigned)k) return;
    const long rank = p - col0[c];
    if (rank < 0 || rank >= (long)col0[c + 1] - col0[c]) return;   // order is not the sort of labels
    const long j = (long)tile0[c] * 32 + rank;
    const float s = rowdot::cut_column(x + (size_t)pick * d, true, j, d, KS, lane, img);
    if (lane == 0) { cnorm[j] = s; colpick[j] = pick; }
}

template <int RM>
__global__ __launch_bounds__(256) void sil_pairs_kernel(const float* __restrict__ x, const unsigned char* __restrict__ img,
                                                        const float* __restrict__ cnorm, const int* __restrict__ colpick,
                                                        const float* __restrict__ rnorm, const int* __restrict__ tile0,
                                                        const int* __restrict__ chunk0, long n, int d, int KS, int k, int CH, long Q,
                                                        long rtiles, long ygroups, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sil_lds[];
    constexpr int RT = 32 * RM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int nch = chunk0[k];
    // work item = (row tile, four chunks), row tile fastest: workgroups that run together read the same chunks of the image
    for (long item = blockIdx.x; item < rtiles * ygroups; item += gridDim.x) {
        const long row0 = (item % rtiles) * RT;
        const int q = (int)(item / rtiles) * 4 + wave;
        rowdot::stage_rows<RM>(sil_lds, x, row0, n, d, KS, tid);
        __syncthreads();
        if (q < nch) {                                     // (wave-uniform)
            int lo = 0, hi = k;                            // the cluster of chunk q: chunk0[lo] <= q < chunk0[hi], hi - lo -> 1
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (chunk0[mid] <= q) lo = mid; else hi = mid;
            }
            const int c = lo;
            const long t0 = (long)tile0[c] + (long)(q - chunk0[c]) * CH;
            const long t1 = t0 + CH < (long)tile0[c + 1] ? t0 + CH : (long)tile0[c + 1];

            float rn[RM][16];
            double run[RM][16];
#pragma unroll
            for (int m = 0; m < RM; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long row = row0 + rowdot::acc_row(m, r, h);
                    rn[m][r] = row < n ? rnorm[row] : 0.f;
                    run[m][r] = 0.0;
                }
            for (long ct = t0; ct < t1; ++ct) {
                f32x16 acc[RM];
                rowdot::tile_product<RM>(acc, sil_lds, img, ct, KS, lane, h, l32);
                const long col = ct * 32 + l32;
                const int pk = colpick[col];               // -1: the column pads its cluster; its planes and norm were never written
                const float cn = pk >= 0 ? cnorm[col] : 0.f;
#pragma unroll
                for (int m = 0; m < RM; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const long row = row0 + rowdot::acc_row(m, r, h);
                        const float key = fmaf(2.f, acc[m][r], -cn);           // knn.hip's l2 key ...
                        const float d2 = fmaxf(0.f, rn[m][r] + (-key));        // ... and its value (a NaN is 0)
                        const double dist = sqrt((double)d2);
                        run[m][r] += (pk >= 0 && (long)pk != row) ? dist : 0.0;
                    }
            }
#pragma unroll
            for (int m = 0; m < RM; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    double v = run[m][r];
#pragma unroll
                    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);   // the 32 columns of a row: one tree, the same in every lane
                    const long row = row0 + rowdot::acc_row(m, r, h);
                    if (l32 == m * 16 + r && row < n) part[(size_t)row * Q + q] = v;
                }
        }
        __syncthreads();                                   // every wave has read the rows before the next item's are staged
    }
}

// S[i][c] = the partials of cluster c's chunks, ascending
__global__ __launch_bounds__(256) void sil_sum_kernel(const double* __restrict__ part, const int* __restrict__ chunk0, long n, int k,
                                                      long Q, double* __restrict__ S) {
    const long total = n * (long)k;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long i = e / k;
        const int c = (int)(e - i * k);
        double s = 0.0;
        for (int q = chunk0[c]; q < chunk0[c + 1]; ++q) s += part[(size_t)i * Q + q];
        S[e] = s;
    }
}

// ---- finalise ---------------------------------------------------------------------------------------------------------------

struct FinWs { size_t fcount, cptr, members, part, tot, total; };
inline FinWs fin_ws(long n, int k, int C) {
    const size_t chunks = (size_t)((n + SIL_ROWS - 1) / SIL_ROWS);
    FinWs w;
    size_t o = 0;
    w.fcount = o; o += mi_align_up((size_t)k * 4, 256);
    w.cptr = o; o += mi_align_up((size_t)(C + 1) * 4, 256);
    w.members = o; o += mi_align_up((size_t)k * 4, 256);
    w.part = o; o += mi_align_up(chunks * (size_t)C * 8, 256);
    w.tot = o; o += mi_align_up(chunks * 8, 256);
    w.total = o;
    return w;
}
inline bool fin_sizes_ok(long n, int k, int C) { return n >= 2 && n < (1l << 31) && k >= 1 && k <= SIL_KMAX && C >= 2 && C <= SIL_CMAX; }

// one workgroup: the fine clusters of every class in ascending fine index (cptr, members), the class counts, the verdict
__global__ __launch_bounds__(256) void fin_setup_kernel(const int* __restrict__ fcount, const int* __restrict__ class_of, int k, int C,
                                                        int* __restrict__ cptr, int* __restrict__ members,
                                                        int* __restrict__ class_count, int* __restrict__ info) {
    __shared__ int cnt[SIL_CMAX], fill[SIL_CMAX + 1];
    __shared__ int bad;
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) { cnt[c] = 0; fill[c] = 0; }
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int f = tid; f < k; f += 256) {
        const int c = class_of[f];
        if ((unsigned)c >= (unsigned)C) bad = 1;
        else { atomicAdd(&cnt[c], fcount[f]); atomicAdd(&fill[c], 1); }
    }
    __syncthreads();
    if (tid == 0) {
        int at = 0, nonempty = 0, largest = 0;
        for (int c = 0; c < C; ++c) {
            const int m = fill[c];
            cptr[c] = at; fill[c] = at; at += m;
            nonempty += cnt[c] > 0;
            largest = cnt[c] > largest ? cnt[c] : largest;
        }
        cptr[C] = at;
        if (!bad)
            for (int f = 0; f < k; ++f) members[fill[class_of[f]]++] = f;
        info[0] = nonempty; info[1] = largest;
        info[2] = bad ? 2 : (nonempty < 2 || largest < 2) ? 1 : 0;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) class_count[c] = cnt[c];
}

// workgroup = a chunk of SIL_ROWS picks, a wave per pick, lane l the classes l, l + 64, ...
__global__ __launch_bounds__(256) void fin_pick_kernel(const double* __restrict__ S, const int* __restrict__ labels,
                                                       const int* __restrict__ class_of, long n, int k, int C,
                                                       const int* __restrict__ cptr, const int* __restrict__ members,
                                                       const int* __restrict__ class_count, const int* __restrict__ info,
                                                       double* __restrict__ s_out, double* __restrict__ a_out,
                                                       double* __restrict__ b_out, int* __restrict__ nearest_out,
                                                       int* __restrict__ confusion, double* __restrict__ part,
                                                       double* __restrict__ tot) {
    __shared__ double sh_s[SIL_ROWS];
    __shared__ int sh_own[SIL_ROWS];
    if (info[2] != 0) return;                              // (uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long chunk = blockIdx.x, row0 = chunk * SIL_ROWS;
    const int rows = n - row0 < SIL_ROWS ? (int)(n - row0) : SIL_ROWS;
    for (int r = wave; r < rows; r += 4) {
        const long i = row0 + r;
        const int f = labels[i];
        const bool known = (unsigned)f < (unsigned)k;
        const int own = known ? class_of[f] : -1;
        const double* Si = S + (size_t)i * k;
        double bmin = INFINITY, own_sum = 0.0;
        int bcls = 0x7fffffff;
        for (int c = lane; c < C; c += 64) {
            const int cnt = class_count[c];
            if (cnt == 0) continue;
            double cs = 0.0;
            for (int e = cptr[c]; e < cptr[c + 1]; ++e) cs += Si[members[e]];
            if (c == own) own_sum = cs;
            else {
                const double v = cs / (double)cnt;
                if (v < bmin) { bmin = v; bcls = c; }      // ascending c in a lane: the first minimum stays
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bmin, o, 64);
            const int oc = __shfl_xor(bcls, o, 64);
            if (ov < bmin || (ov == bmin && oc < bcls)) { bmin = ov; bcls = oc; }
        }
        own_sum = wave_sum(own_sum);                       // one lane holds it, the others 0: exact
        if (lane == 0) {
            double a = 0.0, s = 0.0;
            if (known) {
                const int cnt = class_count[own];
                if (cnt > 1) {
                    a = own_sum / (double)(cnt - 1);
                    const double big = a > bmin ? a : bmin;
                    s = big > 0.0 ? (bmin - a) / big : 0.0;
                }
                if (bcls < C) atomicAdd(&confusion[(size_t)own * C + bcls], 1);   // (no class only where every sum is NaN)
                else bcls = -1;
            } else {
                a = s = bmin = NAN;
                bcls = -1;
            }
            s_out[i] = s; a_out[i] = a; b_out[i] = bmin; nearest_out[i] = bcls;
            sh_s[r] = known ? s : 0.0;
            sh_own[r] = own;
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        double sum = 0.0;
        for (int r = 0; r < rows; ++r) sum += sh_own[r] == c ? sh_s[r] : 0.0;
        part[(size_t)chunk * C + c] = sum;
    }
    if (tid == 255) {
        double sum = 0.0;
        for (int r = 0; r < rows; ++r) sum += sh_s[r];
        tot[chunk] = sum;
    }
}

// one workgroup: the chunks in ascending order
__global__ __launch_bounds__(256) void fin_mean_kernel(const double* __restrict__ part, const double* __restrict__ tot, long n, int C,
                                                       const int* __restrict__ class_count, const int* __restrict__ info,
                                                       double* __restrict__ class_mean, double* __restrict__ mean) {
    if (info[2] != 0) return;
    const long chunks = (n + SIL_ROWS - 1) / SIL_ROWS;
    for (int c = threadIdx.x; c < C; c += 256) {
        double sum = 0.0;
        for (long q = 0; q < chunks; ++q) sum += part[(size_t)q * C + c];
        class_mean[c] = class_count[c] > 0 ? sum / (double)class_count[c] : NAN;
    }
    if (threadIdx.x == 255) {
        double sum = 0.0;
        for (long q = 0; q < chunks; ++q) sum += tot[q];
        *mean = sum / (double)n;
    }
}

__global__ __launch_bounds__(256) void contingency_kernel(const int* __restrict__ a, const int* __restrict__ b, long n, int ca, int cb,
                                                          unsigned long long* __restrict__ table) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int u = a[i], v = b[i];
        if ((unsigned)u < (unsigned)ca && (unsigned)v < (unsigned)cb) atomicAdd(&table[(size_t)u * cb + v], 1ull);
    }
}

}  // namespace

extern "C" size_t mi_silhouette_workspace_bytes(long n, int d, int k) {
    if (!sil_sizes_ok(n, d, k)) return 0;
    return sil_ws(n, d, k).total;
}

extern "C" int mi_silhouette_sums(const float* x, const int32_t* labels, const int32_t* order, long n, int d, int k, double* sums_out,
                                  void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!x || !labels || !order || !sums_out || !ws) return MI_E_ARG;
    if (!sil_sizes_ok(n, d, k)) return MI_E_UNSUPPORTED;
    if (((uintptr_t)ws & 15) || (((uintptr_t)x & 15) && !(d & 3))) return MI_E_ARG;
    const SilWs w = sil_ws(n, d, k);
    if (ws_bytes < w.total) return MI_E_WORKSPACE;
    const SilPlan p = sil_plan(n, d, k);
    const int KS = rowdot::shape(0, d).KS;
    unsigned char* b = (unsigned char*)ws;
    unsigned char* img = b + w.image;
    float* cnorm = (float*)(b + w.cnorm);
    int* colpick = (int*)(b + w.colpick);
    float* rnorm = (float*)(b + w.rnorm);
    int* counts = (int*)(b + w.counts);
    int* col0 = (int*)(b + w.col0);
    int* tile0 = (int*)(b + w.tile0);
    int* chunk0 = (int*)(b + w.chunk0);
    double* part = (double*)(b + w.part);
    hipStream_t st = (hipStream_t)stream;
    static std::atomic<bool> lds_allowed[64];
    const int ra = mi_allow_dynamic_lds(lds_allowed, SIL_LDS_MAX, sil_pairs_kernel<2>, sil_pairs_kernel<1>);
    if (ra != MI_OK) return ra;
    MI_HIP(hipMemsetAsync(counts, 0, (size_t)k * 4, st));
    MI_HIP(hipMemsetAsync(colpick, 0xff, (size_t)p.KT * 32 * 4, st));
    hipLaunchKernelGGL(label_count_kernel, dim3(sil_blocks(n, 256)), dim3(256), 0, st, (const int*)labels, n, k, counts);
    hipLaunchKernelGGL(sil_scan_kernel, dim3(1), dim3(256), 0, st, (const int*)counts, k, p.CH, col0, tile0, chunk0);
    hipLaunchKernelGGL(sil_prep_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, x, (const int*)labels, (const int*)order, n, d,
                       KS, k, (const int*)col0, (const int*)tile0, img, cnorm, colpick, rnorm);
    MI_RETURN_IF_LAUNCH_FAILED();
    const size_t lds = rowdot::lds_planes_bytes(p.rt, KS);
    const long ygroups = (p.Q + 3) / 4;
    const dim3 grid(sil_blocks(p.rtiles * ygroups, 1));
    if (p.rt == 64)
        hipLaunchKernelGGL(sil_pairs_kernel<2>, grid, dim3(256), lds, st, x, (const unsigned char*)img, (const float*)cnorm,
                           (const int*)colpick, (const float*)rnorm, (const int*)tile0, (const int*)chunk0, n, d, KS, k, p.CH, p.Q,
                           p.rtiles, ygroups, part);
    else
        hipLaunchKernelGGL(sil_pairs_kernel<1>, grid, dim3(256), lds, st, x, (const unsigned char*)img, (const float*)cnorm,
                           (const int*)colpick, (const float*)rnorm, (const int*)tile0, (const int*)chunk0, n, d, KS, k, p.CH, p.Q,
                           p.rtiles, ygroups, part);
    hipLaunchKernelGGL(sil_sum_kernel, dim3(sil_blocks(n * (long)k, 256)), dim3(256), 0, st, (const double*)part, (const int*)chunk0, n, k,
                       p.Q, sums_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" size_t mi_silhouette_finalise_workspace_bytes(long n, int k, int C) {
    if (!fin_sizes_ok(n, k, C)) return 0;
    return fin_ws(n, k, C).total;
}

extern "C" int mi_silhouette_finalise(const double* sums, const int32_t* labels, const int32_t* class_of, long n, int k, int C,
                                      double* s_out, double* a_out, double* b_out, int32_t* nearest_out, double* class_mean_out,
                                      int32_t* class_count_out, double* mean_out, int32_t* confusion_out, int32_t* info_out, void* ws,
                                      size_t ws_bytes, mi_stream_t stream) {
    if (!sums || !labels || !class_of || !s_out || !a_out || !b_out || !nearest_out || !class_mean_out || !class_count_out ||
        !mean_out || !confusion_out || !info_out || !ws)
        return MI_E_ARG;
    if (!fin_sizes_ok(n, k, C)) return MI_E_UNSUPPORTED;
    if ((uintptr_t)ws & 15) return MI_E_ARG;
    const FinWs w = fin_ws(n, k, C);
    if (ws_bytes < w.total) return MI_E_WORKSPACE;
    unsigned char* b = (unsigned char*)ws;
    int* fcount = (int*)(b + w.fcount);
    int* cptr = (int*)(b + w.cptr);
    int* members = (int*)(b + w.members);
    double* part = (double*)(b + w.part);
    double* tot = (double*)(b + w.tot);
    hipStream_t st = (hipStream_t)stream;
    const unsigned chunks = (unsigned)((n + SIL_ROWS - 1) / SIL_ROWS);
    MI_HIP(hipMemsetAsync(fcount, 0, (size_t)k * 4, st));
    MI_HIP(hipMemsetAsync(confusion_out, 0, (size_t)C * C * 4, st));
    hipLaunchKernelGGL(label_count_kernel, dim3(sil_blocks(n, 256)), dim3(256), 0, st, (const int*)labels, n, k, fcount);
    hipLaunchKernelGGL(fin_setup_kernel, dim3(1), dim3(256), 0, st, (const int*)fcount, (const int*)class_of, k, C, cptr, members,
                       (int*)class_count_out, (int*)info_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(fin_pick_kernel, dim3(chunks), dim3(256), 0, st, sums, (const int*)labels, (const int*)class_of, n, k, C,
                       (const int*)cptr, (const int*)members, (const int*)class_count_out, (const int*)info_out, s_out, a_out, b_out,
                       (int*)nearest_out, (int*)confusion_out, part, tot);
    hipLaunchKernelGGL(fin_mean_kernel, dim3(1), dim3(256), 0, st, (const double*)part, (const double*)tot, n, C,
                       (const int*)class_count_out, (const int*)info_out, class_mean_out, mean_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_label_contingency(const int32_t* a, const int32_t* b, long n, int ca, int cb, int64_t* table_out, mi_stream_t stream) {
    if (!a || !b || !table_out) return MI_E_ARG;
    if (n < 1 || n >= (1l << 31) || ca < 1 || cb < 1 || (long)ca * cb > (1l << 24)) return MI_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    MI_HIP(hipMemsetAsync(table_out, 0, (size_t)ca * cb * 8, st));
    hipLaunchKernelGGL(contingency_kernel, dim3(sil_blocks(n, 256)), dim3(256), 0, st, (const int*)a, (const int*)b, n, ca, cb,
                       (unsigned long long*)table_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

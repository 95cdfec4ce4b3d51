// k-means over the exploration embeddings (reference plot_2d.py: faiss.Kmeans(d, 256, niter=300, gpu=True)), DESIGN.md 4.9.
//   prep    centroids (k, d) f32 -> the operand image of rowdot.h: their bf16x3 cut in B-fragment order + |c_j|^2, +inf
//           for the columns that pad k to 32                                                             (once per iteration)
//   xnorm   |x_i|^2                                                                                      (once per fit)
//   assign  labels[i] = argmin_j |x_i|^2 + (|c_j|^2 - 2 x_i . c_j), lowest index on ties; dist[i]; per-workgroup objective
//           partials.  The N x k x d product runs on v_mfma_f32_32x32x16_bf16 in the library's bf16x3 arithmetic (six
//           products of an exact 3-way cut, smallest terms first: bf16x3.h) through the row-product tile of
//           rowdot.h, which knn.hip shares: dist and the squared L2 distance of knn_search are the same bytes.
//   update  a stable counting sort of the point indices by label (integers only), sums over fixed 64-position segments
//           of the sorted order in position order, per-cluster reduction of the segment partials in segment order (f64),
//           then the empty-cluster rule and the objective on one workgroup.  No floating-point atomics: same inputs,
//           same bytes.
// Rows are addressed with 64-bit offsets throughout (N x d may exceed 2 GiB); N < 2^31.
// hipcc-flags: -fno-slp-vectorize
#include "common.h"
#include "rowdot.h"
#include "../../include/cetpick_hip.h"

namespace {

using namespace bf3;        // the bf16x3 arithmetic, its types and helpers: bf16x3.h

constexpr int KM_DMAX = 512, KM_KMAX = 1024;
constexpr int KM_CHUNK = 1024;            // points per workgroup of the counting sort
constexpr int KM_SEG = 64;                // sorted positions per first-level partial sum (one wave)
constexpr float KM_EPS = 1.f / 1024.f;

// |x_i|^2, one wave per row
__global__ __launch_bounds__(256) void km_xnorm_kernel(const float* x, long n, int d, float* xnorm) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int lane = threadIdx.x & 63;
    const float s = rowdot::row_sqnorm(x + (size_t)row * d, d, lane);
    if (lane == 0) xnorm[row] = s;
}

__device__ __forceinline__ void km_better(float& v, int& i, float v2, int i2) {
    if (v2 < v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

// A workgroup owns 32 RM points: their bf16x3 cut is staged once into LDS (rowdot.h) and stays for all k centroids.  The four
// waves share the rows and take the column tiles ct = wave, wave + 4, ...; the centroid fragments stream from the image (L2)
// to registers and serve RM row tiles each.  Epilogue per column tile: v = |c|^2 - 2 acc, a running (min, index) per
// accumulator register (columns ascend within a lane: strict < keeps the lowest index), merged across the 32 lanes of a
// row and then across the four waves with the (value, lowest index) rule.
template <int RM>
__global__ __launch_bounds__(256) void km_assign_kernel(const float* x, const float* xnorm, const unsigned char* img,
                                                        const float* cnorm, long n, int d, int KS, int KT, int* labels,
                                                        float* dist, double* objpart) {
    extern __shared__ __attribute__((aligned(16))) unsigned char km_lds[];
    constexpr int RT = 32 * RM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const long row0 = (long)blockIdx.x * RT;

    rowdot::stage_rows<RM>(km_lds, x, row0, n, d, KS, tid);
    __syncthreads();

    float best[RM][16];
    int bidx[RM][16];
#pragma unroll
    for (int m = 0; m < RM; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) { best[m][r] = INFINITY; bidx[m][r] = 0; }

    for (int ct = wave; ct < KT; ct += 4) {
        f32x16 acc[RM];
        rowdot::tile_product<RM>(acc, km_lds, img, ct, KS, lane, h, l32);
        const int col = ct * 32 + l32;
        const float cn = cnorm[col];
#pragma unroll
        for (int m = 0; m < RM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = fmaf(-2.f, acc[m][r], cn);
                if (v < best[m][r]) { best[m][r] = v; bidx[m][r] = col; }
            }
    }
    __syncthreads();                                       // the planes are done with: their memory takes the merge
    float* mv = reinterpret_cast<float*>(km_lds);          // [4][RT]
    int* mi = reinterpret_cast<int*>(km_lds + 4 * RT * 4);
    float* dv = reinterpret_cast<float*>(km_lds + 8 * RT * 4);      // [RT]
#pragma unroll
    for (int m = 0; m < RM; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = best[m][r];
            int i = bidx[m][r];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) km_better(v, i, __shfl_xor(v, o, 64), __shfl_xor(i, o, 64));
            if (l32 == 0) {
                const int tr = rowdot::acc_row(m, r, h);
                mv[wave * RT + tr] = v;
                mi[wave * RT + tr] = i;
            }
        }
    __syncthreads();
    if (tid < RT) {
        float v = mv[tid];
        int i = mi[tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) km_better(v, i, mv[w * RT + tid], mi[w * RT + tid]);
        const long row = row0 + tid;
        float dd = 0.f;
        if (row < n) {
            dd = fmaxf(0.f, xnorm[row] + v);
            labels[row] = i;
            dist[row] = dd;
        }
        dv[tid] = dd;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int r = 0; r < RT; ++r) s += (double)dv[r];
        objpart[blockIdx.x] = s;
    }
}

// ---- update: stable counting sort ---------------------------------------------------------------------------------------
// chunkhist[c][j] = number of points of chunk c with label j (labels outside [0, k) are left out of everything)
__global__ __launch_bounds__(256) void km_hist_kernel(const int* labels, long n, int k, int* chunkhist) {
    __shared__ int hcnt[KM_KMAX];
    const int tid = threadIdx.x;
    for (int j = tid; j < k; j += 256) hcnt[j] = 0;
    __syncthreads();
    const long base = (long)blockIdx.x * KM_CHUNK;
    for (int q = tid; q < KM_CHUNK; q += 256) {
        const long i = base + q;
        if (i < n) {
            const int l = labels[i];
            if ((unsigned)l < (unsigned)k) atomicAdd(&hcnt[l], 1);          // integer: the sum does not depend on the order
        }
    }
    __syncthreads();
    for (int j = tid; j < k; j += 256) chunkhist[(size_t)blockIdx.x * k + j] = hcnt[j];
}

// chunkhist becomes the exclusive scan over chunks (per label); starts[j] = first sorted position of cluster j, starts[k] = total
__global__ __launch_bounds__(1024) void km_scan_kernel(int* chunkhist, int nchunk, int k, int* starts) {
    __shared__ int tot[KM_KMAX];
    const int j = threadIdx.x;
    if (j < k) {
        int run = 0;
        for (int c = 0; c < nchunk; ++c) {
            const int t = chunkhist[(size_t)c * k + j];
            chunkhist[(size_t)c * k + j] = run;
            run += t;
        }
        tot[j] = run;
    }
    __syncthreads();
    if (j == 0) {
        int run = 0;
        for (int q = 0; q < k; ++q) { starts[q] = run; run += tot[q]; }
        starts[k] = run;
    }
}

// order[starts[l] + chunkhist[c][l] + (number of earlier points of the chunk with label l)] = point index: ascending
// point index inside every cluster
__global__ __launch_bounds__(256) void km_scatter_kernel(const int* labels, long n, int k, const int* chunkhist, const int* starts,
                                                         int* order) {
    __shared__ __attribute__((aligned(16))) int lab[KM_CHUNK];
    const int tid = threadIdx.x;
    const long base = (long)blockIdx.x * KM_CHUNK;
    for (int q = tid; q < KM_CHUNK; q += 256) {
        int l = -1;
        if (base + q < n) { l = labels[base + q]; if ((unsigned)l >= (unsigned)k) l = -1; }
        lab[q] = l;
    }
    __syncthreads();
    for (int q = tid; q < KM_CHUNK; q += 256) {
        const int l = lab[q];
        if (l < 0) continue;
        int rank = 0;
        const int q4 = q & ~3;
        for (int p = 0; p < q4; p += 4) {
            const int4 v = *reinterpret_cast<const int4*>(&lab[p]);
            rank += (v.x == l) + (v.y == l) + (v.z == l) + (v.w == l);
        }
        for (int p = q4; p < q; ++p) rank += lab[p] == l;
        order[starts[l] + chunkhist[(size_t)blockIdx.x * k + l] + rank] = (int)(base + q);
    }
}

// One wave per segment g of 64 sorted positions.  The points of the segment are added in position order; whenever the
// cluster changes the running sum goes to slot g + j of `part` (rows of d floats): along the sorted order g + j strictly
// increases, so every run of a cluster inside a segment has a slot of its own, and cluster j's runs are the slots g + j for
// g = starts[j] / 64 .. (starts[j + 1] - 1) / 64.  Lane l holds features l, l + 64, ...
template <int NQ>
__global__ __launch_bounds__(256) void km_segsum_kernel(const float* x, const int* labels, const int* order, const int* starts,
                                                        int k, int d, float* part) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long total = starts[k], p0 = g * KM_SEG;
    if (p0 >= total) return;
    const int cnt = (int)(total - p0 < KM_SEG ? total - p0 : KM_SEG);
    int my_i = 0, my_l = 0;
    if (lane < cnt) { my_i = order[p0 + lane]; my_l = labels[my_i]; }
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
    int cur = __shfl(my_l, 0, 64);
    auto flush = [&](int j) {
        float* o = part + (size_t)(g + j) * d;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (q * 64 + lane < d) o[q * 64 + lane] = acc[q];
    };
    for (int p = 0; p < cnt; p += 4) {
        float v[4][NQ];
        int ls[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int pp = p + u < cnt ? p + u : cnt - 1;
            const float* row = x + (size_t)__shfl(my_i, pp, 64) * d;
            ls[u] = __shfl(my_l, pp, 64);
#pragma unroll
            for (int q = 0; q < NQ; ++q) v[u][q] = q * 64 + lane < d ? row[q * 64 + lane] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (p + u < cnt) {
                if (ls[u] != cur) {                        // (wave-uniform)
                    flush(cur);
#pragma unroll
                    for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
                    cur = ls[u];
                }
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] += v[u][q];
            }
        }
    }
    flush(cur);
}

// cluster j: counts[j]; its mean from the segment partials in segment order (second level in f64).  An empty cluster keeps
// its centroid until km_final_kernel serves it.
__global__ __launch_bounds__(256) void km_mean_kernel(const float* part, const int* starts, int d, float* cent, int* counts) {
    const int j = blockIdx.x;
    const int s = starts[j], e = starts[j + 1];
    if (threadIdx.x == 0) counts[j] = e - s;
    if (e == s) return;
    const int g0 = s / KM_SEG, g1 = (e - 1) / KM_SEG;
    for (int f = threadIdx.x; f < d; f += 256) {
        double sum = 0.0;
        for (int g = g0; g <= g1; ++g) sum += (double)part[(size_t)(g + j) * d + f];
        cent[(size_t)j * d + f] = (float)(sum / (double)(e - s));
    }
}

// One workgroup: the objective (sum of the assign kernel's partials, fixed tree) and the empty-cluster rule.  Empty clusters
// are served in ascending index; the donor is the cluster with the most points at that moment (lowest index on ties); the
// empty cluster takes the donor's centroid with component m scaled by 1 + eps (m even) / 1 - eps (m odd), the donor the
// opposite; the donor's count n is split n / 2 (to the empty cluster) and n - n / 2.
__global__ __launch_bounds__(1024) void km_final_kernel(float* cent, int* counts, int k, int d, const double* objpart, int npart,
                                                        float* obj, int* nsplit) {
    __shared__ int cnt[KM_KMAX];
    __shared__ double red[1024];
    __shared__ int wbest_n[16], wbest_j[16];
    __shared__ int donor_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (obj) {
        double s = 0.0;
        for (int i = tid; i < npart; i += 1024) s += objpart[i];
        red[tid] = s;
        __syncthreads();
        for (int o = 512; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) obj[0] = (float)red[0];
    }
    cnt[tid] = tid < k ? counts[tid] : -1;
    __syncthreads();
    int splits = 0;
    for (int e = 0; e < k; ++e) {
        if (cnt[e] != 0) continue;                         // (uniform: LDS value read by every thread)
        int bn = cnt[tid], bj = tid;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int n2 = __shfl_xor(bn, o, 64), j2 = __shfl_xor(bj, o, 64);
            if (n2 > bn || (n2 == bn && j2 < bj)) { bn = n2; bj = j2; }
        }
        if (lane == 0) { wbest_n[wave] = bn; wbest_j[wave] = bj; }
        __syncthreads();
        if (tid == 0) {
            int n1 = wbest_n[0], j1 = wbest_j[0];
            for (int w = 1; w < 16; ++w)
                if (wbest_n[w] > n1 || (wbest_n[w] == n1 && wbest_j[w] < j1)) { n1 = wbest_n[w]; j1 = wbest_j[w]; }
            donor_s = j1;
        }
        __syncthreads();
        const int dn = donor_s;
        if (tid < d) {
            const float c = cent[(size_t)dn * d + tid];
            const float up = c * (1.f + KM_EPS), dw = c * (1.f - KM_EPS);
            cent[(size_t)e * d + tid] = (tid & 1) ? dw : up;
            cent[(size_t)dn * d + tid] = (tid & 1) ? up : dw;
        }
        __syncthreads();                                   // every thread has read cnt[] and donor_s
        if (tid == 0) {
            const int nn = cnt[dn];
            cnt[e] = nn / 2;
            cnt[dn] = nn - nn / 2;
        }
        ++splits;
        __syncthreads();
    }
    if (tid < k) counts[tid] = cnt[tid];
    if (tid == 0 && nsplit) nsplit[0] += splits;
}

struct KmWs { size_t objpart, chunkhist, starts, order, part, total; int nchunk, npart; long nseg; };
inline int km_rows_per_wg(int d) { return d <= 256 ? 64 : 32; }
inline KmWs km_ws(long n, int d, int k) {
    KmWs w;
    const int rt = km_rows_per_wg(d);
    w.npart = (int)((n + rt - 1) / rt);
    w.nchunk = (int)((n + KM_CHUNK - 1) / KM_CHUNK);
    w.nseg = (n + KM_SEG - 1) / KM_SEG;
    size_t o = 0;
    w.objpart = o; o += mi_align_up((size_t)w.npart * 8, 256);
    w.chunkhist = o; o += mi_align_up((size_t)w.nchunk * k * 4, 256);
    w.starts = o; o += mi_align_up((size_t)(k + 1) * 4, 256);
    w.order = o; o += mi_align_up((size_t)n * 4, 256);
    w.part = o; o += mi_align_up((size_t)(w.nseg + k) * d * 4, 256);
    w.total = o;
    return w;
}
inline int km_check(long n, int d, int k) {
    if (d < 1 || d > KM_DMAX || k < 2 || k > KM_KMAX || n < k || n >= (1l << 31)) return MI_E_UNSUPPORTED;
    return MI_OK;
}

}  // namespace

extern "C" size_t mi_kmeans_image_bytes(int d, int k) {
    if (d < 1 || d > KM_DMAX || k < 2 || k > KM_KMAX) return 0;
    return rowdot::image_bytes(k, d);
}

extern "C" size_t mi_kmeans_workspace_bytes(long n, int d, int k) {
    if (km_check(n, d, k) != MI_OK) return 0;
    return km_ws(n, d, k).total;
}

extern "C" int mi_kmeans_prep(const float* centroids, int d, int k, void* image, mi_stream_t stream) {
    if (!centroids || !image) return MI_E_ARG;
    if (d < 1 || d > KM_DMAX || k < 2 || k > KM_KMAX) return MI_E_UNSUPPORTED;
    if ((uintptr_t)image & 15) return MI_E_ARG;
    const rowdot::Shape s = rowdot::shape(k, d);
    unsigned char* img = (unsigned char*)image;
    hipLaunchKernelGGL(rowdot::prep_kernel, dim3((unsigned)(s.KT * 32)), dim3(64), 0, (hipStream_t)stream, centroids, (long)k, d, s.KS,
                       INFINITY, img, (float*)(img + rowdot::planes_bytes(k, d)));
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_kmeans_xnorm(const float* x, long n, int d, float* xnorm, mi_stream_t stream) {
    if (!x || !xnorm || n < 1) return MI_E_ARG;
    if (d < 1 || d > KM_DMAX || n >= (1l << 31)) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(km_xnorm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, n, d, xnorm);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_kmeans_assign(const float* x, const float* xnorm, const void* image, long n, int d, int k, int32_t* labels,
                                float* dist, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!x || !xnorm || !image || !labels || !dist || !ws) return MI_E_ARG;
    const int rc = km_check(n, d, k);
    if (rc != MI_OK) return rc;
    if (((uintptr_t)image & 15) || ((uintptr_t)ws & 15) || (((uintptr_t)x & 15) && !(d & 3))) return MI_E_ARG;
    const KmWs w = km_ws(n, d, k);
    if (ws_bytes < w.total) return MI_E_WORKSPACE;
    const rowdot::Shape s = rowdot::shape(k, d);
    const unsigned char* img = (const unsigned char*)image;
    const float* cnorm = (const float*)(img + rowdot::planes_bytes(k, d));
    double* objpart = (double*)((unsigned char*)ws + w.objpart);
    const int rt = km_rows_per_wg(d);
    const size_t lds = rowdot::lds_planes_bytes(rt, s.KS);             // <= 100 KB of the CU's 160 KB
    static std::atomic<bool> lds_allowed[64];
    const int ra = mi_allow_dynamic_lds(lds_allowed, 112 * 1024, km_assign_kernel<2>, km_assign_kernel<1>);
    if (ra != MI_OK) return ra;
    if (rt == 64)
        hipLaunchKernelGGL(km_assign_kernel<2>, dim3((unsigned)w.npart), dim3(256), lds, (hipStream_t)stream, x, xnorm, img, cnorm, n, d,
                           s.KS, (int)s.KT, labels, dist, objpart);
    else
        hipLaunchKernelGGL(km_assign_kernel<1>, dim3((unsigned)w.npart), dim3(256), lds, (hipStream_t)stream, x, xnorm, img, cnorm, n, d,
                           s.KS, (int)s.KT, labels, dist, objpart);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_kmeans_update(const float* x, const int32_t* labels, long n, int d, int k, float* centroids, int32_t* counts,
                                float* obj, int32_t* nsplit, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!x || !labels || !centroids || !counts || !ws) return MI_E_ARG;
    const int rc = km_check(n, d, k);
    if (rc != MI_OK) return rc;
    const KmWs w = km_ws(n, d, k);
    if (ws_bytes < w.total) return MI_E_WORKSPACE;
    if ((uintptr_t)ws & 15) return MI_E_ARG;
    unsigned char* b = (unsigned char*)ws;
    int* chunkhist = (int*)(b + w.chunkhist);
    int* starts = (int*)(b + w.starts);
    int* order = (int*)(b + w.order);
    float* part = (float*)(b + w.part);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(km_hist_kernel, dim3((unsigned)w.nchunk), dim3(256), 0, st, labels, n, k, chunkhist);
    hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(1024), 0, st, chunkhist, w.nchunk, k, starts);
    hipLaunchKernelGGL(km_scatter_kernel, dim3((unsigned)w.nchunk), dim3(256), 0, st, labels, n, k, chunkhist, starts, order);
    const unsigned sg = (unsigned)((w.nseg + 3) / 4);
    const int nq = (d + 63) / 64;
    if (nq <= 1) hipLaunchKernelGGL(km_segsum_kernel<1>, dim3(sg), dim3(256), 0, st, x, labels, order, starts, k, d, part);
    else if (nq <= 2) hipLaunchKernelGGL(km_segsum_kernel<2>, dim3(sg), dim3(256), 0, st, x, labels, order, starts, k, d, part);
    else if (nq <= 4) hipLaunchKernelGGL(km_segsum_kernel<4>, dim3(sg), dim3(256), 0, st, x, labels, order, starts, k, d, part);
    else hipLaunchKernelGGL(km_segsum_kernel<8>, dim3(sg), dim3(256), 0, st, x, labels, order, starts, k, d, part);
    hipLaunchKernelGGL(km_mean_kernel, dim3((unsigned)k), dim3(256), 0, st, part, starts, d, centroids, counts);
    hipLaunchKernelGGL(km_final_kernel, dim3(1), dim3(1024), 0, st, centroids, counts, k, d, (const double*)(b + w.objpart), w.npart,
                       obj, nsplit);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

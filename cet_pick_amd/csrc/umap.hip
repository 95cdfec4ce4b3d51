// UMAP over a k-nearest-neighbour graph (reference plot_2d.py --mode umap: umap.UMAP), DESIGN.md 4.14.  k is the number of
// COLUMNS of the graph: UMAP's n_neighbors counts the point itself, so k = n_neighbors - 1.
//   smooth_knn  one wave per row of the (N, k) table of squared distances, lane c holding columns c and c + 64: d = sqrt as
//               fp32, rho = the row's smallest positive d, sigma by umap-learn's bisection in double (from 1, doubling while
//               unbounded, <= 64 steps, |sum - log2(k + 1)| < 1e-5), floored at 1e-3 of the row's (or the table's) mean
//               distance; w = exp(-max(0, d - rho) / sigma).
// The graph, its transpose, the incident list of a vertex and its slot numbers: see knn_graph.h.
//   union       one thread per directed edge: wsym = a + b - a b with b the weight of the opposite edge or 0, whether that edge
//               exists, and the edge's spacing eps = wmax / wsym in double (+inf for an edge pruned at wsym < wmax / n_epochs).
//   rowmax,     the label-supervised map (fit_transform(x, y=labels)): s = wsym f(labels of the two ends), m_i the
//   supervise   largest s over the pairs of vertex i (one wave per vertex), wsup = p + q - p q with p = s / m_i, q = s / m_j (one
//               thread per directed edge), and the spacing of wsup as the union writes it.
//   epoch       one wave (one workgroup) per vertex.  The lanes stride over the vertex's incident list 64 entries at a time; the
//               pairs that fire this epoch are listed in LDS, and the lanes then stride over (firing, term): term 0 the
//               attraction, terms 1..5 the negatives, drawn by Philox from
//               (vertex, slot, epoch).  Every term is evaluated in double from the positions at the START of the epoch; the
//               lanes' sums go through a fixed butterfly, and y_out = fp32(y + alpha acc) is the only rounding to fp32.
// No floating-point atomics, no order that depends on timing: the same inputs give the same bytes.
#include "common.h"
#include "knn_graph.h"
#include "philox.h"
#include "../../include/cetpick_hip.h"

namespace {

constexpr int UM_KMAX = 127, UM_NEG = 5, UM_TERMS = 1 + UM_NEG;
constexpr double UM_CLIP = 4.0;

inline int um_check(long n, int k) {
    if (k < 1 || k > UM_KMAX || n < (long)k + 2 || n * (long)k >= (1l << 31)) return MI_E_UNSUPPORTED;
    return MI_OK;
}

// ---- smooth distances ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void um_smooth_kernel(const float* dist2, long n, int k, double mean_all, float* out_rho,
                                                        float* out_sigma, float* out_w) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;                                  // (wave-uniform)
    const float* dr = dist2 + (size_t)row * k;
    const bool h0 = lane < k, h1 = lane + 64 < k;
    const float f0 = h0 ? (float)sqrt((double)fmaxf(dr[lane], 0.f)) : 0.f;          // the correctly rounded fp32 root
    const float f1 = h1 ? (float)sqrt((double)fmaxf(dr[lane + 64], 0.f)) : 0.f;
    float mn = fminf(f0 > 0.f ? f0 : INFINITY, f1 > 0.f ? f1 : INFINITY);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
    const float rho32 = mn == INFINITY ? 0.f : mn;
    const double rho = (double)rho32, d0 = (double)f0, d1 = (double)f1;
    const double g0 = d0 - rho, g1 = d1 - rho;
    const double row_sum = wave_sum(d0 + d1);
    const double target = log2((double)(k + 1));
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int step = 0; step < 64; ++step) {
        const double t0 = h0 ? (g0 > 0.0 ? exp(-g0 / mid) : 1.0) : 0.0, t1 = h1 ? (g1 > 0.0 ? exp(-g1 / mid) : 1.0) : 0.0;
        const double s = wave_sum(t0 + t1);
        if (fabs(s - target) < 1e-5) break;                // (wave-uniform: every lane holds the same sum)
        if (s > target) {
            hi = mid;
            mid = (lo + hi) * 0.5;
        } else {
            lo = mid;
            mid = hi == INFINITY ? mid * 2.0 : (lo + hi) * 0.5;
        }
    }
    const double floor_at = 1e-3 * (rho > 0.0 ? row_sum / (double)(k + 1) : mean_all);
    const double sigma = fmax(mid, floor_at);
    if (h0) out_w[(size_t)row * k + lane] = g0 > 0.0 ? (float)exp(-g0 / sigma) : 1.f;
    if (h1) out_w[(size_t)row * k + lane + 64] = g1 > 0.0 ? (float)exp(-g1 / sigma) : 1.f;
    if (lane == 0) {
        out_rho[row] = rho32;
        out_sigma[row] = (float)sigma;
    }
}

// the spacing in epochs of an edge of weight ws (+inf: pruned, it never fires), wmax the largest weight of the graph
__device__ __forceinline__ double um_spacing(float ws, float wmax, int n_epochs) {
    const double wm = (double)wmax, v = (double)ws;
    return (!(v > 0.0) || v < wm / (double)n_epochs) ? (double)INFINITY : wm / v;
}

// ---- union -----------------------------------------------------------------------------------------------------------------
// An edge the graph passes over gets wsym 0, mutual 0 and (with wmax) eps +inf.
__global__ __launch_bounds__(256) void um_union_kernel(KnnGraph g, const float* w, const float* wmax, int n_epochs, float* out_wsym,
                                                       uint8_t* out_mutual, double* out_eps) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= g.ne()) return;
    const int i = (int)(e / g.k);
    int j;
    float ws = 0.f;
    uint8_t mu = 0;
    if (g.forward(i, e, j)) {
        const double a = (double)w[e];
        double b = 0.0;
        const int e2 = g.opposite(i, j);
        if (e2 >= 0) {
            mu = 1;
            b = (double)w[e2];
        }
        ws = (float)(a + b - a * b);
    }
    out_wsym[e] = ws;
    out_mutual[e] = mu;
    if (wmax) out_eps[e] = um_spacing(ws, wmax[0], n_epochs);
}

// ---- label supervision -----------------------------------------------------------------------------------------------------
// umap-learn's categorical intersection: the factor on the weight of a pair by the labels of its ends (any negative label: unknown)
__device__ __forceinline__ double um_factor(int la, int lb, double f_far, double f_unknown) {
    return (la < 0 || lb < 0) ? f_unknown : (la != lb ? f_far : 1.0);
}

// m_i = the largest wsym f over the pairs of vertex i: its k forward edges, then every edge of its reverse range (a mutual pair
// is met twice with the same value).  One wave per vertex; a maximum does not depend on the order.
__global__ __launch_bounds__(256) void um_rowmax_kernel(KnnGraph g, const float* wsym, const int* label, double f_far, double f_unknown,
                                                        double* out_m) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= g.n) return;                                // (wave-uniform)
    const int i = (int)row, li = label[i];
    double m = 0.0;
    int j, e2;
    for (int c = lane; c < g.k; c += 64) {
        const long e = (long)i * g.k + c;
        if (g.forward(i, e, j)) m = fmax(m, (double)wsym[e] * um_factor(li, label[j], f_far, f_unknown));
    }
    const KnnGraph::Range rr = g.rev_range(i);
    for (long r = (long)rr.r0 + lane; r < rr.r1; r += 64) {
        if (!g.reverse(r, e2)) continue;
        j = g.source(e2);
        if (j != i) m = fmax(m, (double)wsym[e2] * um_factor(label[j], li, f_far, f_unknown));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if (lane == 0) out_m[i] = m;
}

// An edge the graph passes over gets wsup 0 and (with wmax) eps +inf, as in the union.
__global__ __launch_bounds__(256) void um_supervise_kernel(KnnGraph g, const float* wsym, const int* label, const double* rowmax,
                                                           double f_far, double f_unknown, const float* wmax, int n_epochs,
                                                           float* out_wsup, double* out_eps) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= g.ne()) return;
    const int i = (int)(e / g.k);
    int j;
    float ws = 0.f;
    if (g.forward(i, e, j)) {
        const double s = (double)wsym[e] * um_factor(label[i], label[j], f_far, f_unknown);
        const double mi = rowmax[i], mj = rowmax[j];
        const double p = s / (mi > 0.0 ? mi : 1.0), q = s / (mj > 0.0 ? mj : 1.0);
        ws = (float)(p + q - p * q);
    }
    out_wsup[e] = ws;
    if (wmax) out_eps[e] = um_spacing(ws, wmax[0], n_epochs);
}

// ---- epoch -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double um_clip(double v) { return fmin(fmax(v, -UM_CLIP), UM_CLIP); }
__device__ __forceinline__ bool um_fires(double eps, double n) { return floor(n / eps) > floor((n - 1.0) / eps); }

struct UmPair { int j, slot; };

// The lanes stride over the UM_TERMS terms of each of the nf firings listed in `list`.
__device__ __forceinline__ void um_terms(const UmPair* list, int nf, int lane, const float* y, int i, int n, int epoch, double xi, double yi,
                                         double a, double b, uint32_t k0, uint32_t k1, double& ax, double& ay) {
    for (int q = lane; q < nf * UM_TERMS; q += 64) {
        const UmPair pr = list[q / UM_TERMS];
        const int t = q % UM_TERMS;
        if (t == 0) {                                      // attraction; both matrix entries of the pair fire on this schedule
            const double dx = xi - (double)y[2 * (size_t)pr.j], dy = yi - (double)y[2 * (size_t)pr.j + 1];
            const double d2 = dx * dx + dy * dy;
            if (d2 > 0.0) {
                const double p = pow(d2, b);
                const double c = -2.0 * a * b * (p / d2) / (a * p + 1.0);
                ax += 2.0 * um_clip(c * dx);
                ay += 2.0 * um_clip(c * dy);
            }
        } else {
            const int tn = t - 1;
            const u32x4 r = philox4x32_10((uint32_t)i, (uint32_t)pr.slot, (uint32_t)epoch, (uint32_t)(tn >> 2), k0, k1);
            const uint32_t word = (tn & 3) == 0 ? r.v[0] : (tn & 3) == 1 ? r.v[1] : (tn & 3) == 2 ? r.v[2] : r.v[3];
            const int kk = below(word, n);                 // in [0, n)
            if (kk == i) continue;
            const double dx = xi - (double)y[2 * (size_t)kk], dy = yi - (double)y[2 * (size_t)kk + 1];
            const double d2 = dx * dx + dy * dy;
            if (d2 > 0.0) {
                const double c = 2.0 * b / ((0.001 + d2) * (a * pow(d2, b) + 1.0));
                ax += um_clip(c * dx);
                ay += um_clip(c * dy);
            } else {
                ax += UM_CLIP;
                ay += UM_CLIP;
            }
        }
    }
}

// One wave = one workgroup per vertex, so the barriers around the LDS list are wave-wide.  Per batch of the incident list the
// entries that fire this epoch are listed in LDS, then the lanes stride over their terms.
__global__ __launch_bounds__(64) void um_epoch_kernel(const float* __restrict__ y, float* __restrict__ y_out, KnnEpochGraph g, int epoch,
                                                      int n_epochs, double a, double b, uint32_t k0, uint32_t k1) {
    __shared__ UmPair list[64];
    const int lane = threadIdx.x, i = blockIdx.x;
    const double xi = (double)y[2 * (size_t)i], yi = (double)y[2 * (size_t)i + 1], en = (double)epoch;
    const unsigned long long below_me = (1ull << lane) - 1ull;
    double ax = 0.0, ay = 0.0;
    g.for_incident(i, lane, [&](const KnnEpochGraph::Entry& t) __attribute__((always_inline)) {
        const bool fire = t.has && um_fires(g.eps[t.e], en);
        const unsigned long long mask = __ballot(fire);
        if (fire) list[__popcll(mask & below_me)] = UmPair{t.j, t.slot};
        __syncthreads();
        um_terms(list, __popcll(mask), lane, y, i, g.n, epoch, xi, yi, a, b, k0, k1, ax, ay);
        __syncthreads();
    });
    ax = wave_sum(ax);
    ay = wave_sum(ay);
    if (lane == 0) {
        const double alpha = 1.0 - (en - 1.0) / (double)n_epochs;
        y_out[2 * (size_t)i] = (float)(xi + alpha * ax);
        y_out[2 * (size_t)i + 1] = (float)(yi + alpha * ay);
    }
}

}  // namespace

extern "C" int mi_umap_check(long n, int k) { return um_check(n, k); }

extern "C" int mi_umap_smooth_knn(const float* dist2, long n, int k, double mean_all, float* out_rho, float* out_sigma, float* out_w,
                                  mi_stream_t stream) {
    if (!dist2 || !out_rho || !out_sigma || !out_w) return MI_E_ARG;
    const int rc = um_check(n, k);
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(um_smooth_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dist2, n, k, mean_all, out_rho,
                       out_sigma, out_w);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_umap_union(const int32_t* index, const float* w, const int32_t* rev_ptr, const int32_t* rev_edge, long n, int k,
                             const float* wmax, int n_epochs, float* out_wsym, uint8_t* out_mutual, double* out_eps, mi_stream_t stream) {
    const KnnGraph g{index, rev_ptr, rev_edge, (int)n, k};
    if (!g.complete() || !w || !out_wsym || !out_mutual || (wmax && !out_eps)) return MI_E_ARG;
    const int rc = um_check(n, k);
    if (rc != MI_OK) return rc;
    if (n_epochs < 1) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(um_union_kernel, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, w, wmax, n_epochs, out_wsym,
                       out_mutual, out_eps);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_umap_rowmax(const int32_t* index, const float* wsym, const int32_t* label, const int32_t* rev_ptr,
                              const int32_t* rev_edge, long n, int k, double f_far, double f_unknown, double* out_rowmax,
                              mi_stream_t stream) {
    const KnnGraph g{index, rev_ptr, rev_edge, (int)n, k};
    if (!g.complete() || !wsym || !label || !out_rowmax) return MI_E_ARG;
    const int rc = um_check(n, k);
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(um_rowmax_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, wsym, label, f_far, f_unknown,
                       out_rowmax);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_umap_supervise(const int32_t* index, const float* wsym, const int32_t* label, const double* rowmax, long n, int k,
                                 double f_far, double f_unknown, const float* wmax, int n_epochs, float* out_wsup, double* out_eps,
                                 mi_stream_t stream) {
    if (!index || !wsym || !label || !rowmax || !out_wsup || (wmax && !out_eps)) return MI_E_ARG;
    const int rc = um_check(n, k);
    if (rc != MI_OK) return rc;
    if (n_epochs < 1) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(um_supervise_kernel, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       KnnGraph{index, nullptr, nullptr, (int)n, k}, wsym, label, rowmax, f_far, f_unknown, wmax, n_epochs, out_wsup, out_eps);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_umap_epoch(const float* y_in, float* y_out, const int32_t* index, const int32_t* rev_ptr, const int32_t* rev_edge,
                             const uint8_t* mutual, const double* eps, long n, int k, int epoch, int n_epochs, double a, double b,
                             uint64_t seed, mi_stream_t stream) {
    const KnnEpochGraph g{{index, rev_ptr, rev_edge, (int)n, k}, mutual, eps};
    if (!y_in || !y_out || y_in == y_out || !g.complete()) return MI_E_ARG;
    const int rc = um_check(n, k);
    if (rc != MI_OK) return rc;
    if (n_epochs < 1 || epoch < 1 || epoch > n_epochs) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(um_epoch_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, y_in, y_out, g, epoch, n_epochs, a, b,
                       (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32));
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

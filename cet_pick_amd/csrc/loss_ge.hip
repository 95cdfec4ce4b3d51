// The GE-binomial heat-map loss of the detector trainer's --ge variant, reference cet_pick/models/loss.py:
//   _pu_ge_loss :215-253 (PUGELoss :327-337): FocalLoss over the labelled voxels (gt >= 0) + slack x a penalty that ties the
//   expected particle count among the unlabeled voxels (gt == -1) to a Binomial(N, tau) prior.
// With U the unlabeled voxels, N = |U|, mu = sum_U p, v = sum_U p (1 - p), w = v + 1e-7:
//   s_k = -(mu - k)^2 / (2 w),  q = softmax(s) over k = 0 .. N,  b_k = log Binom(k; N, tau),  B = sum_k q_k b_k
//   pen = -B  (+ entropy_penalty / 2 (log v + log 2 pi + 1))
//   g_mu = d pen / d mu = -sum_k q_k (b_k - B)(k - mu) / w
//   g_v  = d pen / d v  = -sum_k q_k (b_k - B)(k - mu)^2 / (2 w^2)  (+ entropy_penalty / (2 v))
//   d loss / d p_i = slack (g_mu + g_v (1 - 2 p_i)) on U, the focal gradient on the labelled voxels.
// Three launches forward, none of which waits on another workgroup:
//   1. ge_voxel_partial_kernel  one streaming pass, fp64 partial sums per workgroup (the focal terms are the arithmetic of
//      loss_ops.hip's voxel_loss_partial_kernel<VL_FOCAL>: the classifier part has the bits mi_focal_loss_fwd gives)
//   2. ge_count_partial_kernel  every workgroup sums the voxel partials for N, mu, v (same order everywhere: same bits), takes the
//      count window from them and walks its share of it; fp64 partial sums of the six moments of e_k = exp(s_k - s_k*)
//   3. ge_final_kernel          one workgroup: both reductions again, pen, B, g_mu, g_v, the loss
// N, mu and v never reach the host: the count grid is fixed from n (N <= n) and the k loop is a grid-stride loop over the window.
//
// The window.  k* = clamp(round(mu), 0, N) has the largest s_k.  exp(x) of a double is exactly 0 for x < -745.2, so relative to the
// term at k* every count with ((mu - k)^2 - (mu - k*)^2) / (2 w) > 746 adds nothing to any of the sums, in a float64 softmax
// over all N + 1 counts as here: only |k - mu| <= sqrt((mu - k*)^2 + 2 * 746 w) is walked - at most 2 * 39 sqrt(w) + 3 counts.
// b_k is taken relative to b_k* (three lgamma differences and one product), which keeps the covariance sums
// sum e b (k - mu) - B sum e (k - mu) free of cancellation; B gets b_k* back at the end.
#include "common.h"
#include "../../include/cetpick_hip.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int GQ = 7;                   // voxel-pass quantities
constexpr int GC = 6;                   // count-stage moments
constexpr int GE_COUNT_BLOCKS = 32;     // cap of the count grid (x 256 counts per sweep)
constexpr double GE_W_FLOOR = 1e-7;     // loss.py:237
constexpr double GE_CUT = 746.0;

int ge_voxel_blocks(long n) { return (int)std::max<long>(1, std::min<long>((n + 256 * 8 - 1) / (256 * 8), 1024)); }
int ge_count_blocks(long n) { return (int)std::max<long>(1, std::min<long>((n + 1 + 255) / 256, GE_COUNT_BLOCKS)); }

// sum of v over the workgroup's 256 threads, to every thread (fixed tree: deterministic)
__device__ __forceinline__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

// quantity j of n_part records of NQ_ doubles
template <int NQ_>
__device__ __forceinline__ double reduce_partials(const double* partials, int n_part, int j, double* red) {
    double s = 0;
    for (int b = threadIdx.x; b < n_part; b += 256) s += partials[(long)b * NQ_ + j];
    return block_sum(s, red);
}

// q0 #pos  q1 #soft  q2 #unlabeled  q3 sum log(p)(1-p)^2 [pos]  q4 sum log(1-p) p^2 (1-g)^4 [soft]
// q5 sum p [unlabeled]  q6 sum p (1-p) [unlabeled]
__global__ __launch_bounds__(256) void ge_voxel_partial_kernel(const float* pred, const float* gt, long n, double* partials) {
    double q[GQ];
#pragma unroll
    for (int k = 0; k < GQ; ++k) q[k] = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float p = pred[i], g = gt[i];
        const bool pos = (g == 1.f), soft = (g > -1.f) && (g < 1.f), unl = (g == -1.f);
        const float lp = logf(p), l1p = logf(1.f - p);
        const float a = lp * (1.f - p) * (1.f - p);          // log(p) (1-p)^2
        const float b = l1p * p * p;                         // log(1-p) p^2
        const float w = (1.f - g) * (1.f - g) * (1.f - g) * (1.f - g);
        if (pos) { q[0] += 1.0; q[3] += a; }
        if (soft) { q[1] += 1.0; q[4] += (double)(b * w); }
        if (unl) { const double pd = p; q[2] += 1.0; q[5] += pd; q[6] += pd * (1.0 - pd); }
    }
    __shared__ double red[256];
    for (int k = 0; k < GQ; ++k) {
        const double s = block_sum(q[k], red);
        if (threadIdx.x == 0) partials[(long)blockIdx.x * GQ + k] = s;
    }
}

struct GeWindow { double w, kstar, dstar; long k_lo, k_hi; };

// (a NaN or infinite mu or v gives the whole range 0 .. N: the walk stays bounded by N <= n whatever the inputs hold)
__device__ __forceinline__ GeWindow ge_window(double N, double mu, double v) {
    GeWindow g;
    g.w = v + GE_W_FLOOR;
    g.kstar = fmin(fmax(rint(mu), 0.0), N);
    g.dstar = g.kstar - mu;
    const double R = sqrt(g.dstar * g.dstar + 2.0 * GE_CUT * g.w);
    g.k_lo = (long)fmax(0.0, floor(mu - R));
    g.k_hi = (long)fmin(N, ceil(mu + R));
    return g;
}

// c0 sum e  c1 sum e b'  c2 sum e d  c3 sum e b' d  c4 sum e d^2  c5 sum e b' d^2      e = exp(s_k - s_k*), b' = b_k - b_k*, d = k - mu
__global__ __launch_bounds__(256) void ge_count_partial_kernel(const double* vpart, int n_vpart, double log_tau, double log_1mtau,
                                                              double* cpart) {
    __shared__ double red[256];
    const double N = reduce_partials<GQ>(vpart, n_vpart, 2, red);
    const double mu = reduce_partials<GQ>(vpart, n_vpart, 5, red);
    const double v = reduce_partials<GQ>(vpart, n_vpart, 6, red);
    const GeWindow gw = ge_window(N, mu, v);
    const double lg_ks = lgamma(gw.kstar + 1.0), lg_nks = lgamma(N - gw.kstar + 1.0);
    const double slope = log_tau - log_1mtau, inv2w = 1.0 / (2.0 * gw.w);
    double c[GC];
#pragma unroll
    for (int j = 0; j < GC; ++j) c[j] = 0.0;
    const long stride = (long)gridDim.x * 256;
    for (long k = gw.k_lo + (long)blockIdx.x * 256 + threadIdx.x; k <= gw.k_hi; k += stride) {
        const double kd = (double)k, dk = kd - gw.kstar, d = kd - mu;
        const double e = exp(-dk * (d + gw.dstar) * inv2w);                    // (d^2 - d*^2 = (k - k*)(d + d*), <= 0 after the sign)
        const double b = (lg_ks - lgamma(kd + 1.0)) + (lg_nks - lgamma(N - kd + 1.0)) + dk * slope;
        const double eb = e * b;
        c[0] += e; c[1] += eb; c[2] += e * d; c[3] += eb * d; c[4] += e * d * d; c[5] += eb * d * d;
    }
    for (int j = 0; j < GC; ++j) {
        const double s = block_sum(c[j], red);
        if (threadIdx.x == 0) cpart[(long)blockIdx.x * GC + j] = s;
    }
}

// the `sums` record: include/cetpick_hip.h
__global__ __launch_bounds__(256) void ge_final_kernel(const double* vpart, int n_vpart, const double* cpart, int n_cpart, long n,
                                                      double log_tau, double log_1mtau, double slack, double entropy_penalty,
                                                      double* sums, float* loss) {
    __shared__ double red[256];
    double q[GQ], c[GC];
    for (int j = 0; j < GQ; ++j) q[j] = reduce_partials<GQ>(vpart, n_vpart, j, red);
    for (int j = 0; j < GC; ++j) c[j] = reduce_partials<GC>(cpart, n_cpart, j, red);
    if (threadIdx.x) return;
    const double N = q[2], mu = q[5], v = q[6];
    const GeWindow gw = ge_window(N, mu, v);
    const double b_ref = lgamma(N + 1.0) - lgamma(gw.kstar + 1.0) - lgamma(N - gw.kstar + 1.0) + gw.kstar * log_tau +
                         (N - gw.kstar) * log_1mtau;
    const double Bp = c[1] / c[0], B = b_ref + Bp;
    double pen = -B;
    const double g_mu = -(c[3] - Bp * c[2]) / (c[0] * gw.w);
    double g_v = -(c[5] - Bp * c[4]) / (2.0 * gw.w * gw.w * c[0]);
    if (entropy_penalty > 0) {                    // v = 0: -inf, as the reference (loss.py:247-249)
        pen += entropy_penalty * 0.5 * (log(v) + 1.8378770664093453 + 1.0);
        g_v += entropy_penalty / (2.0 * v);
    }
    const double focal = q[0] == 0 ? -q[4] : -(q[3] + q[4]) / q[0];          // loss.py:403-409
    const double L = focal + slack * pen;
    for (int j = 0; j < GQ; ++j) sums[j] = q[j];
    sums[7] = focal; sums[8] = L; sums[9] = pen; sums[10] = (double)n; sums[11] = B; sums[12] = g_mu; sums[13] = g_v;
    sums[14] = (double)gw.k_lo; sums[15] = (double)gw.k_hi;
    *loss = (float)L;
}

// labelled voxels: voxel_loss_bwd_kernel<VL_FOCAL>'s coefficients; unlabeled ones: the two GE coefficients, in double (g_mu and
// g_v (1 - 2p) may cancel)
__global__ __launch_bounds__(256) void ge_bwd_kernel(const float* pred, const float* gt, long n, double slack, const double* sums,
                                                    const float* dloss, float* dpred) {
    const float up = *dloss;
    const double np = sums[0];
    float c3 = 0, c4 = 0;
    if (np == 0) c4 = -1.f; else { c3 = (float)(-1.0 / np); c4 = c3; }
    const double cm = (double)up * slack * sums[12], cv = (double)up * slack * sums[13];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float p = pred[i], g = gt[i];
        const bool pos = (g == 1.f), soft = (g > -1.f) && (g < 1.f), unl = (g == -1.f);
        float out = 0.f;
        if (unl) {
            out = (float)(cm + cv * (1.0 - 2.0 * (double)p));
        } else if (pos || soft) {
            const float lp = logf(p), l1p = logf(1.f - p);
            const float da = (1.f - p) * (1.f - p) / p - 2.f * (1.f - p) * lp;        // d/dp log(p)(1-p)^2
            const float db = -p * p / (1.f - p) + 2.f * p * l1p;                      // d/dp log(1-p) p^2
            const float w = (1.f - g) * (1.f - g) * (1.f - g) * (1.f - g);
            float d = 0.f;
            if (pos) d += c3 * da;
            if (soft) d += c4 * db * w;
            out = up * d;
        }
        dpred[i] = out;
    }
}

}  // namespace

// ---- C ABI ---------------------------------------------------------------------------------------
extern "C" size_t mi_pu_ge_loss_workspace_bytes(long n) {
    return n > 0 ? sizeof(double) * ((size_t)GQ * ge_voxel_blocks(n) + (size_t)GC * ge_count_blocks(n)) : 0;
}

extern "C" int mi_pu_ge_loss_fwd(const float* pred, const float* gt, long n, double tau, double slack, double entropy_penalty,
                                 double* sums, float* loss, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!pred || !gt || !sums || !loss || n <= 0 || !(tau > 0.0 && tau < 1.0)) return MI_E_ARG;
    if (!ws || ws_bytes < mi_pu_ge_loss_workspace_bytes(n)) return MI_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int vb = ge_voxel_blocks(n), cb = ge_count_blocks(n);
    double* vpart = (double*)ws;
    double* cpart = vpart + (size_t)GQ * vb;
    const double log_tau = std::log(tau), log_1mtau = std::log1p(-tau);
    hipLaunchKernelGGL(ge_voxel_partial_kernel, dim3(vb), dim3(256), 0, s, pred, gt, n, vpart);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(ge_count_partial_kernel, dim3(cb), dim3(256), 0, s, (const double*)vpart, vb, log_tau, log_1mtau, cpart);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(ge_final_kernel, dim3(1), dim3(256), 0, s, (const double*)vpart, vb, (const double*)cpart, cb, n, log_tau,
                       log_1mtau, slack, entropy_penalty, sums, loss);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_pu_ge_loss_bwd(const float* pred, const float* gt, long n, double slack, const double* sums, const float* dloss,
                                 float* dpred, mi_stream_t stream) {
    if (!pred || !gt || !sums || !dloss || !dpred || n <= 0) return MI_E_ARG;
    const int blocks = (int)std::max<long>(1, std::min<long>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(ge_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pred, gt, n, slack, sums, dloss, dpred);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

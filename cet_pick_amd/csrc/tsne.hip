// Exact t-SNE over a k-nearest-neighbour graph (reference plot_2d.py --mode tsne: sklearn.manifold.TSNE), DESIGN.md 4.12.
//   affinities  one wave per row of the (N, K) distance table: sklearn's _binary_search_perplexity in double (bisection on
//               beta, doubling while unbounded, <= 100 steps, |H - ln perplexity| <= 1e-5), the row's smallest distance taken
//               off first; the row is then evaluated once more at the fp32 value of beta that is returned with it.
//   gradient    repulsion  every lane owns TS_IPL points i, a workgroup TS_IB = 256 TS_IPL of them and one split of the j
//                          range.  y_j goes through LDS in tiles of TS_TJ points and is read as a broadcast; per pair
//                          q = 1 / (1 + |y_i - y_j|^2) with v_rcp_f32, sums of q, q^2 dx, q^2 dy.  A tile's sums are fp32
//                          chains of TS_TJ terms from zero; tile sums are added in double, and the splits' double partials
//                          are written to the workspace.  Only tiles that hold the workgroup's own points or run past the
//                          end of the split test j != i and j < end.
//                 merge      per point the splits in split order (double), and per workgroup the sum of its points' sum q.
//                 finish     Z = the workgroups' sums in a fixed tree, the same in every workgroup; one wave per point gathers
//                            the K forward and the reverse edges (double; the graph: see knn_graph.h), grad = 4 (attr - rep / Z);
//                            with out_kl the wave's share of KL, per workgroup.
//                 kl         one workgroup adds those in a fixed tree.
//   update      sklearn's _gradient_descent step, element-wise, every product and sum rounded once (fp contract off).
// No floating-point atomics and no order that depends on timing: same inputs and same n_split -> same bytes.
// hipcc-flags: -fno-slp-vectorize
#include "common.h"
#include "knn_graph.h"
#include "../../include/cetpick_hip.h"

namespace {

constexpr int TS_KMAX = 127, TS_SMAX = 32, TS_IPL = 4, TS_IB = 256 * TS_IPL, TS_TJ = 128;
constexpr long TS_NMAX = 1l << 24;         // N K < 2^31: edge ids are int32

__device__ __forceinline__ double block_sum_256(double v, double* red, int tid) {   // fixed tree; every thread gets the sum
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- affinities ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ts_affinity_kernel(const float* dist, long n, int K, double target, float* out_p, float* out_beta) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;                                  // (wave-uniform)
    const float* dr = dist + (size_t)row * K;
    const bool h0 = lane < K, h1 = lane + 64 < K;
    double d0 = h0 ? (double)dr[lane] : 0.0, d1 = h1 ? (double)dr[lane + 64] : 0.0;
    float mn = fminf(h0 ? dr[lane] : INFINITY, h1 ? dr[lane + 64] : INFINITY);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
    d0 -= (double)mn;
    d1 -= (double)mn;
    double beta = 1.0, lo = -INFINITY, hi = INFINITY;
    for (int step = 0; step < 100; ++step) {
        const double p0 = h0 ? exp(-d0 * beta) : 0.0, p1 = h1 ? exp(-d1 * beta) : 0.0;
        const double sp = wave_sum(p0 + p1);               // >= 1: the nearest neighbour's term is exp(0)
        const double sd = wave_sum(d0 * p0 + d1 * p1) / sp;
        const double diff = log(sp) + beta * sd - target;
        if (fabs(diff) <= 1e-5) break;                     // (wave-uniform: every lane holds the same sums)
        if (diff > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0 : (beta + hi) * 0.5;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta * 0.5 : (beta + lo) * 0.5;
        }
    }
    const float b32 = (float)beta;
    const double b = (double)b32;
    const double p0 = h0 ? exp(-d0 * b) : 0.0, p1 = h1 ? exp(-d1 * b) : 0.0;
    const double inv = 1.0 / wave_sum(p0 + p1);
    if (h0) out_p[(size_t)row * K + lane] = (float)(p0 * inv);
    if (h1) out_p[(size_t)row * K + lane + 64] = (float)(p1 * inv);
    if (lane == 0) out_beta[row] = b32;
}

// ---- repulsion -------------------------------------------------------------------------------------------------------------
template <bool CHECK>
__device__ __forceinline__ void ts_tile(const float4* tile, const float (&xi)[TS_IPL], const float (&yi)[TS_IPL], const int (&ii)[TS_IPL],
                                        int j0, int jend, float (&sq)[TS_IPL], float (&fx)[TS_IPL], float (&fy)[TS_IPL]) {
#pragma unroll 4
    for (int t = 0; t < TS_TJ / 2; ++t) {
        const float4 v = tile[t];                          // two points, the same address in every lane
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float xj = h ? v.z : v.x, yj = h ? v.w : v.y;
            const int j = j0 + 2 * t + h;
#pragma unroll
            for (int u = 0; u < TS_IPL; ++u) {
                const float dx = xi[u] - xj, dy = yi[u] - yj;
                float q = __builtin_amdgcn_rcpf(fmaf(dx, dx, fmaf(dy, dy, 1.f)));
                if (CHECK) q = (j < jend && j != ii[u]) ? q : 0.f;
                const float q2 = q * q;
                sq[u] += q;
                fx[u] = fmaf(q2, dx, fx[u]);
                fy[u] = fmaf(q2, dy, fy[u]);
            }
        }
    }
}

// part[(c S + s) N + i], c = 0 sum q, 1 sum q^2 dx, 2 sum q^2 dy over the j of split s
__global__ __launch_bounds__(256) void ts_repulsion_kernel(const float* y, int n, int jps, int S, double* part) {
    __shared__ float4 tile[TS_TJ / 2];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * TS_IB, s = blockIdx.y;
    const int jbeg = s * jps, jend = min(n, jbeg + jps);
    float xi[TS_IPL], yi[TS_IPL];
    int ii[TS_IPL];
    double asq[TS_IPL], afx[TS_IPL], afy[TS_IPL];
#pragma unroll
    for (int u = 0; u < TS_IPL; ++u) {
        ii[u] = i0 + u * 256 + tid;
        const bool ok = ii[u] < n;
        xi[u] = ok ? y[2 * (size_t)ii[u]] : 0.f;
        yi[u] = ok ? y[2 * (size_t)ii[u] + 1] : 0.f;
        asq[u] = afx[u] = afy[u] = 0.0;
    }
    float* tf = reinterpret_cast<float*>(tile);
    for (int j0 = jbeg; j0 < jend; j0 += TS_TJ) {          // (workgroup-uniform)
        __syncthreads();
        {
            const int j = j0 + (tid >> 1);                 // 256 threads, 128 points of two floats
            tf[tid] = j < jend ? y[2 * (size_t)j + (tid & 1)] : 0.f;
        }
        __syncthreads();
        float sq[TS_IPL], fx[TS_IPL], fy[TS_IPL];
#pragma unroll
        for (int u = 0; u < TS_IPL; ++u) sq[u] = fx[u] = fy[u] = 0.f;
        const bool check = j0 + TS_TJ > jend || (j0 < i0 + TS_IB && j0 + TS_TJ > i0);
        if (check) ts_tile<true>(tile, xi, yi, ii, j0, jend, sq, fx, fy);
        else ts_tile<false>(tile, xi, yi, ii, j0, jend, sq, fx, fy);
#pragma unroll
        for (int u = 0; u < TS_IPL; ++u) { asq[u] += (double)sq[u]; afx[u] += (double)fx[u]; afy[u] += (double)fy[u]; }
    }
#pragma unroll
    for (int u = 0; u < TS_IPL; ++u)
        if (ii[u] < n) {
            part[((size_t)0 * S + s) * n + ii[u]] = asq[u];
            part[((size_t)1 * S + s) * n + ii[u]] = afx[u];
            part[((size_t)2 * S + s) * n + ii[u]] = afy[u];
        }
}

// rep[c N + i] = the splits of point i in split order; zpart[block] = sum of the block's sum q
__global__ __launch_bounds__(256) void ts_merge_kernel(const double* part, int n, int S, double* rep, double* zpart) {
    __shared__ double red[4];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    double a[3] = {0.0, 0.0, 0.0};
    if (i < n)
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c] += part[((size_t)c * S + s) * n + i];
    if (i < n) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rep[(size_t)c * n + i] = a[c];
    }
    const double z = block_sum_256(i < n ? a[0] : 0.0, red, tid);
    if (tid == 0) zpart[blockIdx.x] = z;
}

// One wave per point over the graph of knn_graph.h: edge e has the conditional affinity p[e], and the joint affinity of the
// pair {i, j} is (p[i -> j] + p[j -> i]) / 2N, a missing direction counting 0.
__global__ __launch_bounds__(256) void ts_finish_kernel(const float* y, KnnGraph g, const float* p, float exaggeration, const double* rep,
                                                        const double* zpart, int nzb, float* grad, float* out_z, double* klpart) {
    __shared__ double red[4];
    __shared__ double klw[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = g.n;
    double zp = 0.0;
    for (int b = tid; b < nzb; b += 256) zp += zpart[b];
    const double Z = block_sum_256(zp, red, tid);
    if (blockIdx.x == 0 && tid == 0) out_z[0] = (float)Z;
    const int i = blockIdx.x * 4 + wave;
    const bool want_kl = klpart != nullptr;
    double ax = 0.0, ay = 0.0, kl = 0.0;
    if (i < n) {                                           // (wave-uniform)
        const double xi = y[2 * (size_t)i], yi = y[2 * (size_t)i + 1];
        const double w2n = 1.0 / (2.0 * (double)n), ex = (double)exaggeration;
        // the attractive term of one directed edge between i and j with conditional affinity pe; returns q_ij
        const auto attract = [&](int j, double pe) __attribute__((always_inline)) {
            const double dx = xi - (double)y[2 * (size_t)j], dy = yi - (double)y[2 * (size_t)j + 1];
            const double q = 1.0 / (1.0 + dx * dx + dy * dy);
            const double w = pe * w2n * ex * q;
            ax += w * dx;
            ay += w * dy;
            return q;
        };
        int j, e2;
        for (int c = lane; c < g.k; c += 64) {             // forward edges
            const long e = (long)i * g.k + c;
            if (!g.forward(i, e, j)) continue;
            const double pe = (double)p[e], q = attract(j, pe);
            if (want_kl) {                                 // the pair's joint affinity: add the edge j -> i where it exists
                const int back = g.opposite(i, j);
                const double pj = (back >= 0 ? pe + (double)p[back] : pe) * w2n;
                if (pj > 0.0) kl += pj * log(pj * Z / q);
            }
        }
        const KnnGraph::Range rr = g.rev_range(i);
        for (long r = (long)rr.r0 + lane; r < rr.r1; r += 64) {        // reverse edges: j -> i
            if (!g.reverse(r, e2)) continue;
            j = g.source(e2);
            if (j == i) continue;
            const double pe = (double)p[e2], q = attract(j, pe);
            if (want_kl) {                                 // counted above when i -> j exists too
                const double pj = pe * w2n;
                if (g.opposite(j, i) < 0 && pj > 0.0) kl += pj * log(pj * Z / q);
            }
        }
        ax = wave_sum(ax);
        ay = wave_sum(ay);
        if (lane == 0) {
            grad[2 * (size_t)i] = (float)(4.0 * (ax - rep[(size_t)n + i] / Z));
            grad[2 * (size_t)i + 1] = (float)(4.0 * (ay - rep[2 * (size_t)n + i] / Z));
        }
    }
    if (want_kl) {                                         // (uniform)
        kl = wave_sum(kl);
        if (lane == 0) klw[wave] = kl;
        __syncthreads();
        if (tid == 0) klpart[blockIdx.x] = (klw[0] + klw[1]) + (klw[2] + klw[3]);
    }
}

__global__ __launch_bounds__(256) void ts_kl_kernel(const double* klpart, int nb, float* out_kl) {
    __shared__ double red[4];
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) a += klpart[b];
    a = block_sum_256(a, red, threadIdx.x);
    if (threadIdx.x == 0) out_kl[0] = (float)a;
}

// ---- update ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ts_update_kernel(float* y, const float* grad, float* vel, float* gains, long m, float momentum, float lr,
                                                        float min_gain) {
#pragma clang fp contract(off)                             // momentum v - lr (g gains) as two products and a difference, not an fma
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const float g = grad[t], v = vel[t];
    float ga = gains[t];
    ga = v * g < 0.f ? ga + 0.2f : ga * 0.8f;
    ga = fmaxf(ga, min_gain);
    const float gg = g * ga, a = momentum * v, b = lr * gg;
    const float nv = a - b;
    gains[t] = ga;
    vel[t] = nv;
    y[t] = y[t] + nv;
}

inline int ts_check(long n, int K, int n_split) {
    if (n < 2 || n > TS_NMAX || K < 1 || K > TS_KMAX || K > n - 1 || n_split < 0 || n_split > TS_SMAX) return MI_E_UNSUPPORTED;
    return MI_OK;
}
struct TsPlan { int S, jps, iblocks, mblocks, fblocks; };
// Splits from N alone: enough workgroups for two rounds over the chip's 256 CUs, no more splits than tiles of j.
inline TsPlan ts_plan(long n, int n_split) {
    TsPlan p;
    p.iblocks = (int)((n + TS_IB - 1) / TS_IB);
    const long tiles = (n + TS_TJ - 1) / TS_TJ;
    long S = n_split;
    if (S == 0) {
        S = (512 + p.iblocks - 1) / p.iblocks;
        if (S > TS_SMAX) S = TS_SMAX;
    }
    if (S > tiles) S = tiles;
    const long tps = (tiles + S - 1) / S;
    p.jps = (int)(tps * TS_TJ);
    p.S = (int)((tiles + tps - 1) / tps);
    p.mblocks = (int)((n + 255) / 256);
    p.fblocks = (int)((n + 3) / 4);
    return p;
}
struct TsWs { size_t part, rep, zpart, klpart, total; };
inline TsWs ts_ws(long n, int n_split) {
    const TsPlan p = ts_plan(n, n_split);
    TsWs w;
    size_t o = 0;
    w.part = o; o += mi_align_up((size_t)3 * p.S * n * 8, 256);
    w.rep = o; o += mi_align_up((size_t)3 * n * 8, 256);
    w.zpart = o; o += mi_align_up((size_t)p.mblocks * 8, 256);
    w.klpart = o; o += mi_align_up((size_t)p.fblocks * 8, 256);
    w.total = o;
    return w;
}

}  // namespace

extern "C" int mi_tsne_affinities(const float* dist, long n, int k, float perplexity, float* out_p, float* out_beta, mi_stream_t stream) {
    if (!dist || !out_p || !out_beta) return MI_E_ARG;
    if (n < 1 || n > TS_NMAX || k < 1 || k > TS_KMAX || !(perplexity >= 1.f) || !(perplexity <= (float)k)) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(ts_affinity_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dist, n, k,
                       log((double)perplexity), out_p, out_beta);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" size_t mi_tsne_workspace_bytes(long n, int k, int n_split) {
    if (ts_check(n, k, n_split) != MI_OK) return 0;
    return ts_ws(n, n_split).total;
}

extern "C" int mi_tsne_gradient(const float* y, const int32_t* index, const float* p, const int32_t* rev_ptr, const int32_t* rev_edge, long n,
                                int k, float exaggeration, int n_split, float* out_grad, float* out_z, float* out_kl, void* ws,
                                size_t ws_bytes, mi_stream_t stream) {
    const KnnGraph g{index, rev_ptr, rev_edge, (int)n, k};
    if (!y || !g.complete() || !p || !out_grad || !out_z || !ws) return MI_E_ARG;
    const int rc = ts_check(n, k, n_split);
    if (rc != MI_OK) return rc;
    if ((uintptr_t)ws & 15) return MI_E_ARG;
    const TsWs w = ts_ws(n, n_split);
    if (ws_bytes < w.total) return MI_E_WORKSPACE;
    const TsPlan pl = ts_plan(n, n_split);
    unsigned char* b = (unsigned char*)ws;
    double* part = (double*)(b + w.part);
    double* rep = (double*)(b + w.rep);
    double* zpart = (double*)(b + w.zpart);
    double* klpart = out_kl ? (double*)(b + w.klpart) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ts_repulsion_kernel, dim3((unsigned)pl.iblocks, (unsigned)pl.S), dim3(256), 0, st, y, (int)n, pl.jps, pl.S, part);
    hipLaunchKernelGGL(ts_merge_kernel, dim3((unsigned)pl.mblocks), dim3(256), 0, st, part, (int)n, pl.S, rep, zpart);
    hipLaunchKernelGGL(ts_finish_kernel, dim3((unsigned)pl.fblocks), dim3(256), 0, st, y, g, p, exaggeration, rep, zpart, pl.mblocks,
                       out_grad, out_z, klpart);
    if (out_kl) hipLaunchKernelGGL(ts_kl_kernel, dim3(1), dim3(256), 0, st, klpart, pl.fblocks, out_kl);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_tsne_update(float* y, const float* grad, float* velocity, float* gains, long n, float momentum, float lr, float min_gain,
                              mi_stream_t stream) {
    if (!y || !grad || !velocity || !gains) return MI_E_ARG;
    if (n < 1 || n > TS_NMAX) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(ts_update_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, grad, velocity, gains,
                       2 * n, momentum, lr, min_gain);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

// Label spreading over the neighbour graph (Zhou et al. 2004, "Learning with local and global consistency"; scikit-learn's
// LabelSpreading), DESIGN.md 4.29.  The reference reaches the same end by hand, in its interactive session.
//   mi_spread_weights    w (n, k) fp32 of the forward edges: 1 (binary) or exp(-d2 / sqrt(s_i s_j)), s_i the largest finite dist of
//                        row i (the self-tuning Gaussian of Zelnik-Manor & Perona); 0 for an edge KnnGraph::forward passes over
//   mi_spread_csr_count  a wave per vertex walks its INCIDENT LIST (knn_graph.h): the valid forward edges in column order, then the
//                        edges of its reverse range that have no opposite edge; entries per vertex and deg_i = sum of
//                        w_sym = max(w_ij, w_ji), float64 (a batch of 64 entries in one fixed tree, the batches in list order)
//   mi_spread_csr_fill   the same walk behind the caller's exclusive scan: col, val = w_sym (dis_i dis_j), dis = 1 / sqrt(deg)
//                        (0 where deg = 0).  The product dis_i dis_j is formed first, so val(i, j) and val(j, i) are the same bytes.
//   mi_spread_step       F_out[i, :] = alpha sum_e val_e F_in[col_e, :] + (1 - alpha) Y[i, :], the hot kernel: a group of
//                        Cp = next power of two >= C lanes owns a row (64 / Cp rows per wave) and walks its entries together, one
//                        accumulator per lane in entry order; the largest |F_out - F_in| goes into one device word by an integer
//                        atomicMax on the bits of the non-negative double (one per workgroup: order-independent)
//   mi_spread_decide     label, confidence and mass per pick
//   mi_seed_nearest      a workgroup per seed: the nearest pick of the seed's tomogram, float64, ties to the lowest pick
// Nothing floating is added by an atomic; every order above is fixed by the graph: the same input gives the same bytes.
#include "common.h"
#include "knn_graph.h"
#include "../../include/cetpick_hip.h"

namespace {

constexpr long LS_GRID = 1l << 20;        // workgroups of a grid-stride launch, at most
constexpr int LS_STEP_GRID = 4096;        // workgroups of the sweep, at most: one atomicMax each on the residual word

inline bool ls_graph_ok(long n, int k) { return n >= 1 && k >= 1 && n < (1l << 31) && n * (long)k < (1l << 31); }

inline unsigned ls_blocks(long items, int per_block, long cap = LS_GRID) {
    const long b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

// ---- edge weights -----------------------------------------------------------------------------------------------------------

// scale[i] = the largest finite dist of row i (0 where there is none)
__global__ __launch_bounds__(256) void spread_scale_kernel(const float* __restrict__ dist, long n, int k, float* __restrict__ scale) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float s = 0.f;
        for (int c = 0; c < k; ++c) {
            const float d = dist[i * k + c];
            if (isfinite(d) && d > s) s = d;
        }
        scale[i] = s;
    }
}

__global__ __launch_bounds__(256) void spread_weights_kernel(KnnGraph g, const float* __restrict__ dist,
                                                             const float* __restrict__ scale, int mode, float* __restrict__ w) {
    const long ne = (long)g.n * g.k;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < ne; e += (long)gridDim.x * 256) {
        const int i = (int)(e / g.k);
        int j;
        float v = 0.f;
        if (g.forward(i, e, j)) {
            if (mode == 0) v = 1.f;
            else {
                const float d2 = dist[e];
                const float q = sqrtf(scale[i]) * sqrtf(scale[j]);          // sqrt(s_i s_j) without the product's over- and underflow
                if (isfinite(d2)) v = q > 0.f ? expf(-(fmaxf(d2, 0.f) / q)) : (d2 <= 0.f ? 1.f : 0.f);
            }
        }
        w[e] = v;
    }
}

// ---- the symmetric graph in CSR form ----------------------------------------------------------------------------------------

// What a lane holds of one batch of 64 positions of vertex i's incident list: the other end j and w_sym where `has`.
struct SpreadEntry { bool has; int j; float w; };

// Called by a whole wave: f(entry, valid lanes before this batch) per batch - the forward columns, then the lone reverse edges.
template <typename F>
__device__ __forceinline__ void spread_incident(const KnnGraph& g, const float* __restrict__ w, int i, int lane, F&& f) {
    for (int c0 = 0; c0 < g.k; c0 += 64) {
        SpreadEntry t{false, 0, 0.f};
        const int c = c0 + lane;
        if (c < g.k) {
            const long e = (long)i * g.k + c;
            t.has = g.forward(i, e, t.j);
            if (t.has) {
                const int e2 = g.opposite(i, t.j);                          // the edge j -> i, in i's reverse range
                const float wr = e2 >= 0 ? w[e2] : 0.f;
                t.w = fmaxf(w[e], wr);
            }
        }
        f(t);
    }
    const KnnGraph::Range rr = g.rev_range(i);
    for (unsigned rb = rr.r0; rb < (unsigned)rr.r1; rb += 64) {             // unsigned: r1 may lie within 64 of 2^31
        SpreadEntry t{false, 0, 0.f};
        int e2;
        if (rb + lane < (unsigned)rr.r1 && g.reverse(rb + lane, e2)) {
            const int j = g.source(e2);
            // an edge j -> i of another row, with no edge i -> j (that one sits in j's reverse range)
            if (j != i && g.index[e2] == i && g.opposite(j, i) < 0) { t.has = true; t.j = j; t.w = fmaxf(w[e2], 0.f); }
        }
        f(t);
    }
}

__global__ __launch_bounds__(256) void spread_count_kernel(KnnGraph g, const float* __restrict__ w, int64_t* __restrict__ count,
                                                           double* __restrict__ deg) {
    const int lane = threadIdx.x & 63;
    for (long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6); i < g.n; i += (long)gridDim.x * 4) {       // (wave-uniform)
        long cnt = 0;
        double sum = 0.0;
        spread_incident(g, w, (int)i, lane, [&](const SpreadEntry& t) {
            cnt += __popcll(__ballot(t.has));
            sum += wave_sum(t.has ? (double)t.w : 0.0);                     // one tree per batch, the same in every lane
        });
        if (lane == 0) { count[i] = cnt; deg[i] = sum; }
    }
}

__device__ __forceinline__ double spread_dis(double deg) { return deg > 0.0 ? 1.0 / sqrt(deg) : 0.0; }

__global__ __launch_bounds__(256) void spread_fill_kernel(KnnGraph g, const float* __restrict__ w, const int64_t* __restrict__ row_ptr,
                                                          const double* __restrict__ deg, long nnz, int* __restrict__ col,
                                                          double* __restrict__ val) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below_me = (1ull << lane) - 1ull;
    for (long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6); i < g.n; i += (long)gridDim.x * 4) {
        long at = row_ptr[i];
        const long end = row_ptr[i + 1];
        const double di = spread_dis(deg[i]);
        spread_incident(g, w, (int)i, lane, [&](const SpreadEntry& t) {
            const unsigned long long m = __ballot(t.has);
            const long p = at + (long)__popcll(m & below_me);
            if (t.has && p >= 0 && p < end && p < nnz) {                     // a row_ptr that is not the scan of the counts writes nothing outside
                col[p] = t.j;
                val[p] = (double)t.w * (di * spread_dis(deg[t.j]));
            }
            at += (long)__popcll(m);
        });
    }
}

// ---- the sweep --------------------------------------------------------------------------------------------------------------

// Workgroup = 256 / CP rows, the CP lanes of a group on the classes of one row.  TRACK: also the largest |F_out - F_in|.
template <int CP, bool TRACK>
__global__ __launch_bounds__(256) void spread_step_kernel(const int64_t* __restrict__ row_ptr, const int* __restrict__ col,
                                                          const double* __restrict__ val, long n, int C, double alpha,
                                                          const double* __restrict__ F_in, const double* __restrict__ Y,
                                                          double* __restrict__ F_out, unsigned long long* __restrict__ resid) {
    constexpr int ROWS = 256 / CP;
    const int tid = threadIdx.x, c = tid & (CP - 1), r = tid / CP;
    const double beta = 1.0 - alpha;
    const long tiles = (n + ROWS - 1) / ROWS;
    double worst = 0.0;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long i = tile * ROWS + r;
        if (i >= n || c >= C) continue;
        const long e0 = row_ptr[i], e1 = row_ptr[i + 1];
        double acc = 0.0;
        long e = e0;
        for (; e + 4 <= e1; e += 4) {                                       // four gathers in flight, added in entry order
            int j[4];
            double v[4], f[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { j[u] = col[e + u]; v[u] = val[e + u]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) f[u] = F_in[(size_t)j[u] * C + c];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = fma(v[u], f[u], acc);
        }
        for (; e < e1; ++e) acc = fma(val[e], F_in[(size_t)col[e] * C + c], acc);
        const size_t o = (size_t)i * C + c;
        const double out = alpha * acc + beta * Y[o];
        F_out[o] = out;
        if (TRACK) {
            const double d = fabs(out - F_in[o]);
            worst = d > worst || d != d ? d : worst;                        // a NaN stays: the caller never sees it converge
        }
    }
    if (TRACK) {
        __shared__ unsigned long long part[4];
        unsigned long long b = (unsigned long long)__double_as_longlong(worst);     // non-negative: the bits order as the values
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ob = __shfl_xor(b, o, 64);
            b = ob > b ? ob : b;
        }
        if ((tid & 63) == 0) part[tid >> 6] = b;
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < 4; ++q) b = part[q] > b ? part[q] : b;
            if (b) atomicMax(resid, b);
        }
    }
}

template <int CP>
void spread_step_launch(bool track, unsigned grid, hipStream_t st, const int64_t* row_ptr, const int* col, const double* val, long n,
                        int C, double alpha, const double* F_in, const double* Y, double* F_out, unsigned long long* resid) {
    if (track)
        hipLaunchKernelGGL((spread_step_kernel<CP, true>), dim3(grid), dim3(256), 0, st, row_ptr, col, val, n, C, alpha, F_in, Y, F_out,
                           resid);
    else
        hipLaunchKernelGGL((spread_step_kernel<CP, false>), dim3(grid), dim3(256), 0, st, row_ptr, col, val, n, C, alpha, F_in, Y, F_out,
                           resid);
}

// ---- decision and seed matching ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void spread_decide_kernel(const double* __restrict__ F, long n, int C, double min_conf,
                                                            int* __restrict__ label, double* __restrict__ conf,
                                                            double* __restrict__ mass) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const double* f = F + (size_t)i * C;
        double best = f[0], sum = f[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const double v = f[c];
            sum = __dadd_rn(sum, v);
            if (v > best) { best = v; arg = c; }                            // ascending c: the first maximum stays
        }
        const double p = sum > 0.0 ? best / sum : 0.0;
        label[i] = (sum > 0.0 && p >= min_conf) ? arg : -1;
        conf[i] = p;
        mass[i] = sum;
    }
}

__global__ __launch_bounds__(256) void seed_nearest_kernel(const double* __restrict__ picks, const int* __restrict__ pick_tomo, long n,
                                                           const double* __restrict__ seeds, const int* __restrict__ seed_tomo,
                                                           double radius, int* __restrict__ pick_out, double* __restrict__ dist_out) {
    __shared__ double sd[256];
    __shared__ long si[256];
    const int tid = threadIdx.x;
    const long s = blockIdx.x;
    const double sx = seeds[s * 3], sy = seeds[s * 3 + 1], sz = seeds[s * 3 + 2];
    const int tomo = seed_tomo[s];
    double best = INFINITY;
    long arg = -1;
    for (long i = tid; i < n; i += 256) {                                   // ascending i in a thread: the first minimum stays
        if (pick_tomo[i] != tomo) continue;
        const double dx = picks[i * 3] - sx, dy = picks[i * 3 + 1] - sy, dz = picks[i * 3 + 2] - sz;
        const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));     // no contraction
        if (d2 < best || (arg < 0 && d2 == d2)) { best = d2; arg = i; }
    }
    sd[tid] = best; si[tid] = arg;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const double od = sd[tid + o];
            const long oi = si[tid + o];
            if (oi >= 0 && (si[tid] < 0 || od < sd[tid] || (od == sd[tid] && oi < si[tid]))) { sd[tid] = od; si[tid] = oi; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double d = si[0] >= 0 ? sqrt(sd[0]) : INFINITY;
        pick_out[s] = (si[0] >= 0 && d <= radius) ? (int)si[0] : -1;
        dist_out[s] = d;
    }
}

}  // namespace

extern "C" int mi_spread_weights(const int32_t* index, const float* dist, long n, int k, int mode, float* scale_out, float* w_out,
                                 mi_stream_t stream) {
    if (!index || !w_out || (mode == 1 && (!dist || !scale_out))) return MI_E_ARG;
    if (!ls_graph_ok(n, k) || (mode != 0 && mode != 1)) return MI_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const KnnGraph g{(const int*)index, nullptr, nullptr, (int)n, k};
    if (mode == 1) hipLaunchKernelGGL(spread_scale_kernel, dim3(ls_blocks(n, 256)), dim3(256), 0, st, dist, n, k, scale_out);
    hipLaunchKernelGGL(spread_weights_kernel, dim3(ls_blocks(n * (long)k, 256)), dim3(256), 0, st, g, dist, (const float*)scale_out, mode,
                       w_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_spread_csr_count(const int32_t* index, const int32_t* rev_ptr, const int32_t* rev_edge, const float* w, long n, int k,
                                   int64_t* count_out, double* deg_out, mi_stream_t stream) {
    if (!index || !rev_ptr || !rev_edge || !w || !count_out || !deg_out) return MI_E_ARG;
    if (!ls_graph_ok(n, k)) return MI_E_UNSUPPORTED;
    const KnnGraph g{(const int*)index, (const int*)rev_ptr, (const int*)rev_edge, (int)n, k};
    hipLaunchKernelGGL(spread_count_kernel, dim3(ls_blocks(n, 4)), dim3(256), 0, (hipStream_t)stream, g, w, count_out, deg_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_spread_csr_fill(const int32_t* index, const int32_t* rev_ptr, const int32_t* rev_edge, const float* w, long n, int k,
                                  const int64_t* row_ptr, const double* deg, long nnz, int32_t* col_out, double* val_out,
                                  mi_stream_t stream) {
    if (!index || !rev_ptr || !rev_edge || !w || !row_ptr || !deg || !col_out || !val_out) return MI_E_ARG;
    if (!ls_graph_ok(n, k)) return MI_E_UNSUPPORTED;
    if (nnz < 0 || nnz > 2 * n * (long)k) return MI_E_ARG;
    const KnnGraph g{(const int*)index, (const int*)rev_ptr, (const int*)rev_edge, (int)n, k};
    hipLaunchKernelGGL(spread_fill_kernel, dim3(ls_blocks(n, 4)), dim3(256), 0, (hipStream_t)stream, g, w, row_ptr, deg, nnz,
                       (int*)col_out, val_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_spread_step(const int64_t* row_ptr, const int32_t* col, const double* val, long n, int C, double alpha,
                              const double* F_in, const double* Y, double* F_out, uint64_t* residual_out, mi_stream_t stream) {
    if (!row_ptr || !col || !val || !F_in || !Y || !F_out) return MI_E_ARG;
    if (C < 2 || C > 64 || n < 1 || n >= (1l << 31)) return MI_E_UNSUPPORTED;
    if (!(alpha > 0.0 && alpha < 1.0)) return MI_E_ARG;
    const size_t bytes = (size_t)n * C * 8;
    const uintptr_t a = (uintptr_t)F_in, b = (uintptr_t)F_out, y = (uintptr_t)Y;
    if ((a < b + bytes && b < a + bytes) || (y < b + bytes && b < y + bytes)) return MI_E_ARG;      // F_out overlaps an input
    hipStream_t st = (hipStream_t)stream;
    int cp = 2;
    while (cp < C) cp <<= 1;
    const unsigned grid = ls_blocks(n, 256 / cp, LS_STEP_GRID);
    const bool track = residual_out != nullptr;
    if (track) MI_HIP(hipMemsetAsync(residual_out, 0, 8, st));
    unsigned long long* rs = (unsigned long long*)residual_out;
    const int* cl = (const int*)col;
    switch (cp) {
        case 2: spread_step_launch<2>(track, grid, st, row_ptr, cl, val, n, C, alpha, F_in, Y, F_out, rs); break;
        case 4: spread_step_launch<4>(track, grid, st, row_ptr, cl, val, n, C, alpha, F_in, Y, F_out, rs); break;
        case 8: spread_step_launch<8>(track, grid, st, row_ptr, cl, val, n, C, alpha, F_in, Y, F_out, rs); break;
        case 16: spread_step_launch<16>(track, grid, st, row_ptr, cl, val, n, C, alpha, F_in, Y, F_out, rs); break;
        case 32: spread_step_launch<32>(track, grid, st, row_ptr, cl, val, n, C, alpha, F_in, Y, F_out, rs); break;
        default: spread_step_launch<64>(track, grid, st, row_ptr, cl, val, n, C, alpha, F_in, Y, F_out, rs); break;
    }
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_spread_decide(const double* F, long n, int C, double min_conf, int32_t* label_out, double* conf_out, double* mass_out,
                                mi_stream_t stream) {
    if (!F || !label_out || !conf_out || !mass_out) return MI_E_ARG;
    if (C < 2 || C > 64 || n < 1 || n >= (1l << 31)) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(spread_decide_kernel, dim3(ls_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, F, n, C, min_conf,
                       (int*)label_out, conf_out, mass_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_seed_nearest(const double* picks, const int32_t* pick_tomo, long n, const double* seeds, const int32_t* seed_tomo,
                               long m, double radius, int32_t* pick_out, double* dist_out, mi_stream_t stream) {
    if (!picks || !pick_tomo || !seeds || !seed_tomo || !pick_out || !dist_out) return MI_E_ARG;
    if (n < 1 || n >= (1l << 31) || m < 1 || m >= (1l << 31)) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(seed_nearest_kernel, dim3((unsigned)m), dim3(256), 0, (hipStream_t)stream, picks, (const int*)pick_tomo, n, seeds,
                       (const int*)seed_tomo, radius, (int*)pick_out, dist_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

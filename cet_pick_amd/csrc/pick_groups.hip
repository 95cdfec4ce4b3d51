// Grouping and tracing the picks (reference utils/post_process.py:31-113, `tomo_group_postprocess` and `tomo_fiber_postprocess`;
// detectors/tomo_det_classify.py:196-216 for --spike), DESIGN.md 4.23.
//
//   pick_adjacency_kernel   many workgroups: bit j of word (i, j / 64) = sqrt(d2(i, j)) <= cutoff, the distance-threshold graph as a
//                           bit matrix in the workspace (2 MB at 4096 points)
//   pick_merge_kernel       one workgroup, labels in LDS: rounds of "hook the root of i to the smallest label among i's neighbours"
//                           (integer atomicMin) and "point every label at its root", until a round hooks nothing; then the member
//                           counts.  The fixed point - every label the smallest index of its component - does not depend on the order
//                           in which the atomics land, so the output is the same bytes for the same input.
//   pick_fiber_kernel       one workgroup, one wave per component: range of t, two quadratic least-squares fits on the centred and
//                           scaled abscissa (normal equations, one refinement step), residuals, curvature, and the resampled rows.
//
// This file is compiled with floating-point contraction off (the flag below): numpy rounds every product and sum of d2, of
// linspace and of polyval on its own, and the integer outputs are promised to be the ones numpy truncates to.
// hipcc-flags: -ffp-contract=off
#include "common.h"

namespace {

constexpr int PICK_MAX = 4096;             // points per call
constexpr int PICK_MAX_COMP = PICK_MAX / 7;          // components of more than 6 members
constexpr int PICK_TAB = 8;                // doubles per component in the fit table: a_u b_u c_u a_v b_v c_v start stop
constexpr int PICK_INT_LIMIT = 1 << 30;    // a count of samples beyond this is "does not fit"

inline size_t pick_adj_bytes(int n) { return mi_align_up((size_t)n * (size_t)((n + 63) / 64) * sizeof(unsigned long long), 256); }
inline size_t pick_tab_bytes(int n) { return mi_align_up((size_t)(n / 7) * PICK_TAB * sizeof(double), 256); }

// d2 as numpy evaluates ((a - b) ** 2).sum(-1): every product and sum rounded on its own, (dx^2 + dy^2) + dz^2
__device__ __forceinline__ double pick_d2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

// One thread per (row i, word w): 64 pairs.  The 64 columns of the word are staged in LDS and read as broadcasts.
__global__ __launch_bounds__(256) void pick_adjacency_kernel(const double* __restrict__ pts, int n, double cutoff,
                                                             unsigned long long* __restrict__ adj, int W) {
    __shared__ double col[3][64];
    const int w = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x < 64) {
        const int j = w * 64 + threadIdx.x;
#pragma unroll
        for (int c = 0; c < 3; ++c) col[c][threadIdx.x] = j < n ? pts[3 * (size_t)j + c] : 0.0;
    }
    __syncthreads();
    if (i >= n) return;
    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    const int nj = n - w * 64 < 64 ? n - w * 64 : 64;
    unsigned long long bits = 0;
    for (int k = 0; k < nj; ++k)           // <= 64 trips
        if (sqrt(pick_d2(x, y, z, col[0][k], col[1][k], col[2][k])) <= cutoff) bits |= 1ull << k;
    adj[(size_t)i * W + w] = bits;
}

__global__ __launch_bounds__(1024) void pick_merge_kernel(const unsigned long long* __restrict__ adj, int n, int W,
                                                          int32_t* __restrict__ label, int32_t* __restrict__ size) {
    __shared__ int lab[PICK_MAX];
    __shared__ int cnt[PICK_MAX];
    const int tid = threadIdx.x, B = blockDim.x;
    if (n > PICK_MAX || B != 1024) return; // the entry refuses it; the arrays end there (4 points per thread)
    volatile int* vlab = lab;
    for (int i = tid; i < n; i += B) {     // <= 4 trips
        lab[i] = i;
        cnt[i] = 0;
    }
    __syncthreads();
    // lab[i] <= i always, and lab[i] is a member of i's component; every round but the last lowers a label: <= n rounds, in practice
    // a few more than log2 of the longest chain
    for (int round = 0; round <= n; ++round) {
        int hooked = 0;
        for (int i = tid; i < n; i += B) { // <= 4 trips
            const int li = vlab[i];
            int m = li;
            const unsigned long long* row = adj + (size_t)i * W;
            for (int w = 0; w < W; ++w) {  // <= 64 trips
                unsigned long long bits = row[w];
                while (bits) {             // one trip per neighbour
                    const int j = w * 64 + __builtin_ctzll(bits);
                    bits &= bits - 1;
                    if (j < n) {
                        const int lj = vlab[j];
                        m = lj < m ? lj : m;
                    }
                }
            }
            if (m < li) {
                atomicMin(&lab[li], m);    // the root of i (as of the last round) goes under the smaller label
                atomicMin(&lab[i], m);
                hooked = 1;
            }
        }
        if (!__syncthreads_or(hooked)) break;
        int root[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + k * 1024;
            int r = i < n ? vlab[i] : 0;
            for (int step = 0; step < n; ++step) {       // strictly descending: <= n trips
                const int p = vlab[r];
                if (p == r) break;
                r = p;
            }
            root[k] = r;
        }
        __syncthreads();                   // every walk has ended before a label moves
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (tid + k * 1024 < n) lab[tid + k * 1024] = root[k];
        __syncthreads();
    }
    for (int i = tid; i < n; i += B) atomicAdd(&cnt[lab[i]], 1);
    __syncthreads();
    for (int i = tid; i < n; i += B) {
        label[i] = lab[i];
        size[i] = cnt[lab[i]];
    }
}

// numpy's floor_divide of two float64 (npy_divmod), b > 0 and finite
__device__ __forceinline__ double pick_floor_divide(double a, double b) {
    double mod = fmod(a, b);
    double div = (a - mod) / b;
    if (mod != 0.0 && mod < 0.0) div -= 1.0;
    if (div != 0.0) {
        const double f = floor(div);
        return div - f > 0.5 ? f + 1.0 : f;
    }
    return copysign(0.0, a / b);
}

__device__ __forceinline__ int pick_count(double v) {     // int(v) of a count, "too many" where it would not fit
    if (!(v == v)) return 0;
    if (v >= (double)PICK_INT_LIMIT) return PICK_INT_LIMIT;
    return v <= 0.0 ? 0 : (int)v;
}

// numpy.linspace(start, stop, num)[j]: step = (stop - start) / (num - 1), j * step + start, the last one stop itself
__device__ __forceinline__ double pick_linspace(double start, double stop, int num, int j) {
#pragma clang fp contract(off)
    if (num == 1) return start;
    if (j == num - 1) return stop;
    const double step = (stop - start) / (double)(num - 1);
    const double p = (double)j * step;
    return p + start;
}

__device__ __forceinline__ int pick_trunc(double v) {     // (int) toward zero, held inside int32
    if (!(v == v)) return 0;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return -2147483647 - 1;
    return (int)v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max_nan(double v) {          // a NaN wins, as in numpy.max
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o, 64);
        v = (u != u || u > v) ? u : v;
    }
    return v;
}

// 3 x 3 symmetric positive definite solve (Cholesky), every lane the same numbers
__device__ __forceinline__ void pick_solve3(const double S[5], const double r[3], double out[3]) {
    // unknowns (A, B, C) of A s^2 + B s + C; matrix rows [S4 S3 S2; S3 S2 S1; S2 S1 S0]
    const double l00 = sqrt(S[4]);
    const double l10 = S[3] / l00, l20 = S[2] / l00;
    const double l11 = sqrt(S[2] - l10 * l10);
    const double l21 = (S[1] - l20 * l10) / l11;
    const double l22 = sqrt(S[0] - l20 * l20 - l21 * l21);
    const double y0 = r[0] / l00;
    const double y1 = (r[1] - l10 * y0) / l11;
    const double y2 = (r[2] - l20 * y0 - l21 * y1) / l22;
    out[2] = y2 / l22;
    out[1] = (y1 - l21 * out[2]) / l11;
    out[0] = (y0 - l10 * out[1] - l20 * out[2]) / l00;
}

// max over linspace(start, stop, m2) of 2a / (1 + (2 a y + b)^2)^(2/3), lanes striding over the samples
__device__ __forceinline__ double pick_curvature(double a, double b, double start, double stop, int m2, int lane) {
    double k = -INFINITY;
    const double a2 = 2.0 * a;
    for (int j = lane; j < m2; j += 64) {  // <= m2 / 64 trips
        const double y = pick_linspace(start, stop, m2, j);
        const double g = a2 * y + b;
        const double v = a2 / pow(1.0 + g * g, 2.0 / 3.0);
        k = (v != v || v > k) ? v : k;
    }
    return wave_max_nan(k);
}

__global__ __launch_bounds__(1024) void pick_fiber_kernel(const double* __restrict__ pts, int n, const int32_t* __restrict__ label,
                                                          const int32_t* __restrict__ size, double res_cutoff,
                                                          double curvature_cutoff, double scale, double* __restrict__ comp,
                                                          int32_t* __restrict__ rows, int cap_rows, int32_t* __restrict__ n_rows,
                                                          double* __restrict__ tab) {
    __shared__ int croot[PICK_MAX_COMP];   // the components of more than 6 members, by ascending label
    __shared__ int crows[PICK_MAX_COMP];   // rows of each, then where they start
    __shared__ int csamp[PICK_MAX_COMP];   // samples of each (m_out)
    __shared__ int wave_tot[16];
    __shared__ int n_comp_s, total_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
    if (n > PICK_MAX || blockDim.x != 1024) return;

    // the list of roots in ascending order: thread t looks at the points 4 t .. 4 t + 3, a scan gives their places
    bool mine[4];
    int n_mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = 4 * tid + k;
        mine[k] = i < n && label[i] == i && size[i] > 6;
        n_mine += mine[k];
    }
    int incl = n_mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int base = 0, all = 0;
    for (int w = 0; w < n_waves; ++w) {    // 16 trips
        if (w < wave) base += wave_tot[w];
        all += wave_tot[w];
    }
    const bool too_many = all > PICK_MAX_COMP || all > n / 7;       // label / size that no call of mi_pick_components wrote
    if (!too_many) {
        int at = base + incl - n_mine;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (mine[k]) croot[at++] = 4 * tid + k;
    }
    if (tid == 0) n_comp_s = too_many ? -1 : all;
    __syncthreads();
    const int n_comp = n_comp_s;
    if (n_comp < 0) {
        if (tid == 0) *n_rows = -1;
        return;
    }

    for (int c = wave; c < n_comp; c += n_waves) {       // <= 37 trips per wave; everything below is uniform in the wave
        const int r = croot[c];
        // members, range of t, means of u and v; members in index order per lane, lanes combined in a fixed tree
        double lo = INFINITY, hi = -INFINITY, su = 0.0, sv = 0.0;
        int members = 0;
        for (int i = lane; i < n; i += 64) {             // <= 64 trips
            if (label[i] != r) continue;
            const double t = pts[3 * (size_t)i];
            lo = fmin(lo, t);
            hi = fmax(hi, t);
            su += pts[3 * (size_t)i + 1];
            sv += pts[3 * (size_t)i + 2];
            ++members;
        }
        lo = wave_min(lo);
        hi = -wave_min(-hi);
        su = wave_sum(su);
        sv = wave_sum(sv);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) members += __shfl_xor(members, o, 64);
        const double span = hi - lo;
        const int m2 = pick_count(pick_floor_divide(span, 2.0)), m_out = pick_count(pick_floor_divide(span, scale));
        const double start = lo - 1.0, stop = hi + 1.0;

        double cu[3] = {0.0, 0.0, 0.0}, cv[3] = {0.0, 0.0, 0.0}, res_u = 0.0, res_v = 0.0, k_u = 0.0, k_v = 0.0;
        int accepted = 0;
        // a range no tomogram has (or one that is not finite): the sample counts would not be counts
        const bool absurd = !(span <= 16777216.0) || m_out >= PICK_INT_LIMIT;
        if (members > 6 && m2 > 0 && !absurd) {
            const double mid = 0.5 * (lo + hi), half = 0.5 * span, mu = su / members, mv = sv / members;
            // moments of s = (t - mid) / half in [-1, 1], and whether t takes a third value
            double S[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            int inner = 0;
            for (int i = lane; i < n; i += 64) {
                if (label[i] != r) continue;
                const double t = pts[3 * (size_t)i], s = (t - mid) / half;
                inner |= t > lo && t < hi;
                double p = 1.0;
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    S[q] += p;
                    p *= s;
                }
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) S[q] = wave_sum(S[q]);
            const bool three_values = __any(inner);
            if (!three_values) {
                res_u = res_v = 10000.0;   // numpy's empty residual; see the header for the one difference this makes
            } else {
                // A, B, C of the fits to u - mean(u) and v - mean(v): the normal equations, solved twice - the second time for the
                // residual of the first, which removes the error the squared condition number put into it
                double fu[3] = {0.0, 0.0, 0.0}, fv[3] = {0.0, 0.0, 0.0};
                for (int pass = 0; pass < 3; ++pass) {   // passes 0, 1 solve; pass 2 only sums the squared residuals
                    double ru[3] = {0.0, 0.0, 0.0}, rv[3] = {0.0, 0.0, 0.0}, qu = 0.0, qv = 0.0;
                    for (int i = lane; i < n; i += 64) {
                        if (label[i] != r) continue;
                        const double s = (pts[3 * (size_t)i] - mid) / half;
                        const double eu = (pts[3 * (size_t)i + 1] - mu) - ((fu[0] * s + fu[1]) * s + fu[2]);
                        const double ev = (pts[3 * (size_t)i + 2] - mv) - ((fv[0] * s + fv[1]) * s + fv[2]);
                        ru[0] += eu * s * s;
                        ru[1] += eu * s;
                        ru[2] += eu;
                        rv[0] += ev * s * s;
                        rv[1] += ev * s;
                        rv[2] += ev;
                        qu += eu * eu;
                        qv += ev * ev;
                    }
                    if (pass == 2) {
                        res_u = wave_sum(qu) / members;
                        res_v = wave_sum(qv) / members;
                        break;
                    }
                    double du[3], dv[3];
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        ru[q] = wave_sum(ru[q]);
                        rv[q] = wave_sum(rv[q]);
                    }
                    pick_solve3(S, ru, du);
                    pick_solve3(S, rv, dv);
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        fu[q] += du[q];
                        fv[q] += dv[q];
                    }
                }
                // back to powers of t: a t^2 + b t + c
                const double bu = fu[1] / half, bv = fv[1] / half;
                cu[0] = fu[0] / (half * half);
                cu[1] = bu - 2.0 * cu[0] * mid;
                cu[2] = (fu[2] + mu) - bu * mid + cu[0] * mid * mid;
                cv[0] = fv[0] / (half * half);
                cv[1] = bv - 2.0 * cv[0] * mid;
                cv[2] = (fv[2] + mv) - bv * mid + cv[0] * mid * mid;
                k_u = pick_curvature(cu[0], cu[1], start, stop, m2, lane);
                k_v = pick_curvature(cv[0], cv[1], start, stop, m2, lane);
                const double tot = res_u + res_v, au = fabs(k_u), av = fabs(k_v);
                accepted = (tot < res_cutoff && au < curvature_cutoff && av < curvature_cutoff) ||
                           (res_cutoff <= tot && tot < res_cutoff * 3.0 && au < curvature_cutoff / 10.0 && av < curvature_cutoff / 10.0);
            }
        }
        const int n_out = absurd ? -1 : accepted ? m_out : 0;
        if (lane == 0) {
            double* rec = comp + 16 * (size_t)c;
            rec[0] = r, rec[1] = members, rec[2] = lo, rec[3] = hi;
            rec[4] = cu[0], rec[5] = cu[1], rec[6] = cu[2], rec[7] = res_u;
            rec[8] = cv[0], rec[9] = cv[1], rec[10] = cv[2], rec[11] = res_v;
            rec[12] = k_u, rec[13] = k_v, rec[14] = accepted, rec[15] = n_out;
            double* t8 = tab + PICK_TAB * (size_t)c;
            t8[0] = cu[0], t8[1] = cu[1], t8[2] = cu[2], t8[3] = cv[0], t8[4] = cv[1], t8[5] = cv[2], t8[6] = start, t8[7] = stop;
            crows[c] = n_out;
            csamp[c] = m_out;
        }
    }
    __syncthreads();                       // also makes the table in the workspace visible to the whole workgroup

    if (tid == 0) {
        long total = 0;
        bool bad = false;
        for (int c = 0; c < n_comp; ++c) { // <= 585 trips of < 2^30 each: no overflow
            const int k = crows[c];
            bad |= k < 0;
            crows[c] = (int)(total < PICK_INT_LIMIT ? total : PICK_INT_LIMIT);
            total += k < 0 ? 0 : k;
        }
        total_s = bad ? -1 : (int)(total < PICK_INT_LIMIT ? total : PICK_INT_LIMIT);
        *n_rows = total_s;
    }
    __syncthreads();
    if (total_s < 0 || total_s > cap_rows) return;       // the entry reports it; no row is written

    for (int c = wave; c < n_comp; c += n_waves) {
        const int next = c + 1 < n_comp ? crows[c + 1] : total_s;
        const int at = crows[c], k = next - at, m_out = csamp[c];
        if (k <= 0) continue;
        const double* t8 = tab + PICK_TAB * (size_t)c;
        const double au = t8[0], bu = t8[1], cu = t8[2], av = t8[3], bv = t8[4], cv = t8[5], start = t8[6], stop = t8[7];
        for (int j = lane; j < k; j += 64) {             // <= m_out / 64 trips
#pragma clang fp contract(off)
            const double y = pick_linspace(start, stop, m_out, j);
            const double pu = au * y, qu = pu + bu, ru = qu * y, fu = ru + cu;     // numpy.polyval: Horner, each step rounded
            const double pv = av * y, qv = pv + bv, rv = qv * y, fv = rv + cv;
            int32_t* row = rows + 3 * ((size_t)at + j);
            row[0] = pick_trunc(y);
            row[1] = pick_trunc(fv);
            row[2] = pick_trunc(fu);
        }
    }
}

}  // namespace

extern "C" size_t mi_pick_workspace_bytes(int n) {
    if (n < 0 || n > PICK_MAX) return 0;
    return 256 + pick_adj_bytes(n) + pick_tab_bytes(n);
}

extern "C" int mi_pick_components(const double* pts, int n, double cutoff, int32_t* label, int32_t* size, void* ws, size_t ws_bytes,
                                  mi_stream_t stream) {
    if (n < 0) return MI_E_ARG;
    if (n == 0) return MI_OK;
    if (n > PICK_MAX) return MI_E_UNSUPPORTED;           // never truncated: refused before any launch
    if (!pts || !label || !size || !ws) return MI_E_ARG;
    if (ws_bytes < mi_pick_workspace_bytes(n)) return MI_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const int W = (n + 63) / 64;
    unsigned long long* adj = (unsigned long long*)((unsigned char*)ws + 256);
    hipLaunchKernelGGL(pick_adjacency_kernel, dim3((unsigned)mi_cdiv(n, 256), (unsigned)W), dim3(256), 0, s, pts, n, cutoff, adj, W);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(pick_merge_kernel, dim3(1), dim3(1024), 0, s, adj, n, W, label, size);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_pick_fiber_fit(const double* pts, int n, const int32_t* label, const int32_t* size, double res_cutoff,
                                 double curvature_cutoff, double scale, double* comp, int32_t* rows, int cap_rows, int32_t* n_rows,
                                 void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (n < 0 || cap_rows < 0 || !n_rows) return MI_E_ARG;
    if (n > PICK_MAX) return MI_E_UNSUPPORTED;
    if (!(scale > 0.0) || !(scale <= 1.7e308) || !(res_cutoff == res_cutoff) || !(curvature_cutoff == curvature_cutoff)) return MI_E_ARG;
    const hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        MI_HIP(hipMemsetAsync(n_rows, 0, sizeof(int32_t), s));
        return MI_OK;
    }
    if (!pts || !label || !size || !ws || (n >= 7 && !comp) || (cap_rows > 0 && !rows)) return MI_E_ARG;
    if (ws_bytes < mi_pick_workspace_bytes(n)) return MI_E_WORKSPACE;
    double* tab = (double*)((unsigned char*)ws + 256 + pick_adj_bytes(n));
    hipLaunchKernelGGL(pick_fiber_kernel, dim3(1), dim3(1024), 0, s, pts, n, label, size, res_cutoff, curvature_cutoff, scale, comp,
                       rows, cap_rows, n_rows, tab);
    MI_RETURN_IF_LAUNCH_FAILED();
    // the status depends on the count: the one place where this entry waits for the stream
    int32_t needed = 0;
    MI_HIP(hipMemcpyAsync(&needed, n_rows, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    if (needed < 0) return MI_E_ARG;       // label / size do not describe components
    return needed > cap_rows ? MI_E_UNSUPPORTED : MI_OK;
}

// The SCAN step on stored embeddings ("learning to classify by nearest neighbours": the reference's models/loss.py SCANLoss and
// entropy, summed over the heads as its TomoSCANLoss does), DESIGN.md 4.25:
//   mi_scan_loss_fwd   per head the consistency of anchor and neighbour, the entropy of the mean anchor distribution, their total;
//                      and the sum of the totals over the heads
//   mi_scan_loss_bwd   the gradient of that sum with respect to both logits tensors, one launch
//   mi_scan_assign     per row and head the class (argmax, lowest index on a tie), its probability, optionally all
//                      probabilities, and the class counts
//
// Layout and order are scan_rows.h's.  The forward is workgroups (chunk, head), then the finalise launch, whose thread 0 adds the
// totals h = 0..H-1.  The backward pass has no sum across rows at all.  mi_scan_assign strides a grid over the rows.
#include <limits.h>

#include "scan_rows.h"

namespace {

constexpr int SCAN_ASSIGN_BLOCKS = 4096;   // grid-stride over the rows above that
constexpr double SCAN_BCE_FLOOR = (double)1e-12f;      // 1e-12 as torch holds it, a float constant in float64 too: 9.99999996e-13

__global__ __launch_bounds__(256) void scan_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int B, int C, int H,
                                                       double* __restrict__ part_p, double* __restrict__ part_l) {
    __shared__ double sh_p[4][64];
    __shared__ double sh_l[4];
    const int chunk = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool on = lane < C;
    const ScanRows W = scan_rows(chunk, h, B, C, H, lane);
    double ps = 0.0, ls = 0.0;
    for (int r = wave; r < W.rows; r += 4) {
        const size_t at = W.at(W.row0 + r);
        const ScanExp xa = scan_row_exp(on ? a[at] : 0.f, on), xb = scan_row_exp(on ? b[at] : 0.f, on);
        const double p = xa.e / xa.sum, q = xb.e / xb.sum;
        const double s = wave_sum(p * q);
        ps += p;
        ls += fmax(log(s), -100.0);                        // (log 0 = -inf -> -100: torch's BCELoss clamp)
    }
    sh_p[wave][lane] = ps;
    if (lane == 0) sh_l[wave] = ls;
    __syncthreads();
    if (wave == 0) {
        part_p[((size_t)chunk * H + h) * 64 + lane] = scan_add_waves(&sh_p[0][lane], 64);
        if (lane == 0) part_l[(size_t)chunk * H + h] = scan_add_waves(sh_l, 1);
    }
}

// one workgroup of H waves: wave h finishes head h, thread 0 adds the totals in head order
__global__ __launch_bounds__(1024) void scan_final_kernel(const double* __restrict__ part_p, const double* __restrict__ part_l,
                                                          int B, int C, int H, double entropy_weight, float* __restrict__ stats,
                                                          float* __restrict__ loss, double* __restrict__ mean) {
    __shared__ double totals[SCAN_MAX_H];
    const int tid = threadIdx.x, lane = tid & 63, h = tid >> 6;
    const bool on = lane < C;
    const ScanHead F = scan_head_finish(part_p, part_l, scan_chunks(B), H, h, lane, on, (double)B, (double)B);
    const double total = F.consistency - entropy_weight * F.entropy;
    if (on) mean[(size_t)h * C + lane] = F.mean;
    F.store(total, h, lane, stats, totals);
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < H; ++i) t += totals[i];
        *loss = (float)t;
    }
}

__global__ __launch_bounds__(256) void scan_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int B, int C, int H,
                                                       double entropy_weight, const double* __restrict__ mean,
                                                       const float* __restrict__ dloss, float* __restrict__ da,
                                                       float* __restrict__ db) {
    const int chunk = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool on = lane < C;
    const ScanRows W = scan_rows(chunk, h, B, C, H, lane);
    const double up = (double)*dloss, inv_b = 1.0 / (double)B;
    const double m = on ? mean[(size_t)h * C + lane] : 1.0;
    const double gm = on && m >= 1e-8 ? entropy_weight * (log(m) + 1.0) * inv_b : 0.0;   // d total / d p_ic through the mean
    for (int r = wave; r < W.rows; r += 4) {
        const size_t at = W.at(W.row0 + r);
        const ScanExp xa = scan_row_exp(on ? a[at] : 0.f, on), xb = scan_row_exp(on ? b[at] : 0.f, on);
        const double p = xa.e / xa.sum, q = xb.e / xb.sum;
        const double s = wave_sum(p * q);
        const double ds = (s - 1.0) / fmax((1.0 - s) * s, SCAN_BCE_FLOOR) * inv_b;      // torch's BCELoss backward against ones
        const double ga = ds * q + gm, gb = ds * p;
        const double dza = p * (ga - wave_sum(p * ga)), dzb = q * (gb - wave_sum(q * gb));
        if (on) {
            da[at] = (float)(up * dza);
            db[at] = (float)(up * dzb);
        }
    }
}

__global__ __launch_bounds__(256) void scan_assign_kernel(const float* __restrict__ z, long n, int C, int H, int* __restrict__ cls,
                                                          float* __restrict__ conf, float* __restrict__ prob,
                                                          int* __restrict__ counts) {
    __shared__ int hist[64];
    const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool on = lane < C;
    scan_hist_zero(hist, tid);
    __syncthreads();
    const ScanRows W = scan_rows(0, h, n, C, H, lane);     // (its ld and col: the rows are the grid's)
    for (long row = (long)blockIdx.x * 4 + wave; row < n; row += (long)gridDim.x * 4) {
        const size_t at = W.at(row);
        const float v = on ? z[at] : -INFINITY;
        const ScanExp x = scan_row_exp(v, on);
        const int c = scan_row_argmax(v, x.mx, on);
        if (prob && on) prob[at] = (float)(x.e / x.sum);
        if (lane == c) {
            cls[(size_t)row * H + h] = c;
            conf[(size_t)row * H + h] = (float)(x.e / x.sum);
            atomicAdd(&hist[c], 1);
        }
    }
    __syncthreads();
    scan_hist_flush(hist, tid, C, counts + (size_t)h * C);
}

}  // namespace

extern "C" size_t mi_scan_loss_workspace_bytes(int B, int C, int H) {
    if (!scan_sizes_ok(B, SCAN_MAX_B, C, H)) return 0;
    return scan_carve_parts(nullptr, scan_chunks(B), H).bytes;
}

extern "C" int mi_scan_loss_fwd(const float* anchors, const float* neighbours, int B, int C, int H, double entropy_weight,
                                float* stats_out, float* loss_out, double* mean_out, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!scan_sizes_ok(B, SCAN_MAX_B, C, H) || !anchors || !neighbours || !stats_out || !loss_out || !mean_out) return MI_E_ARG;
    if (!ws || ws_bytes < mi_scan_loss_workspace_bytes(B, C, H)) return MI_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const ScanParts W = scan_carve_parts(ws, scan_chunks(B), H);
    hipLaunchKernelGGL(scan_fwd_kernel, dim3((unsigned)scan_chunks(B), (unsigned)H), dim3(256), 0, s, anchors, neighbours, B, C, H,
                       W.part_p, W.part_l);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(scan_final_kernel, dim3(1), dim3(64 * (unsigned)H), 0, s, (const double*)W.part_p, (const double*)W.part_l, B,
                       C, H, entropy_weight, stats_out, loss_out, mean_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_scan_loss_bwd(const float* anchors, const float* neighbours, int B, int C, int H, double entropy_weight,
                                const double* mean, const float* dloss, float* d_anchors, float* d_neighbours, mi_stream_t stream) {
    if (!scan_sizes_ok(B, SCAN_MAX_B, C, H) || !anchors || !neighbours || !mean || !dloss || !d_anchors || !d_neighbours)
        return MI_E_ARG;
    hipLaunchKernelGGL(scan_bwd_kernel, dim3((unsigned)scan_chunks(B), (unsigned)H), dim3(256), 0, (hipStream_t)stream, anchors,
                       neighbours, B, C, H, entropy_weight, mean, dloss, d_anchors, d_neighbours);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_scan_assign(const float* logits, long n, int C, int H, int32_t* class_out, float* conf_out, float* prob_out,
                              int32_t* counts_out, mi_stream_t stream) {
    if (!scan_sizes_ok(n, LONG_MAX, C, H) || !logits || !class_out || !conf_out || !counts_out) return MI_E_ARG;
    const hipStream_t s = (hipStream_t)stream;
    MI_HIP(hipMemsetAsync(counts_out, 0, sizeof(int32_t) * (size_t)H * C, s));
    const unsigned blocks = (unsigned)std::min<long>(SCAN_ASSIGN_BLOCKS, (n + 3) / 4);
    hipLaunchKernelGGL(scan_assign_kernel, dim3(blocks, (unsigned)H), dim3(256), 0, s, logits, n, C, H, (int*)class_out, conf_out,
                       prob_out, (int*)counts_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

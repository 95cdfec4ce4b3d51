// What follows SCAN's clustering step: the heads scored over the whole neighbour graph (the reference's
// scan_evaluate, trains/eval_utils.py) and the self-labelling loss (ConfidenceBasedCE + MaskedCrossEntropyLoss, models/loss.py:15-66).
//   mi_scan_graph_eval      per head the consistency over every (pick, table entry) pair, the entropy of the mean distribution,
//                           their total (weight 1), and the head with the lowest total
//   mi_scan_selflabel_fwd   one head: target and mask from the weak logits, class weights from the masked counts, the weighted
//                           mean cross-entropy of the strong logits
//   mi_scan_selflabel_bwd   its gradient with respect to the strong logits, one launch
//
// Layout and order are scan_rows.h's; within a row the table entries are added ascending.  Only the counts of the self-label
// forward are added by (integer) atomics.
//
// The graph evaluation reads a neighbour's probabilities from a float64 workspace (N, H C) that its first launch fills: a pick is
// the neighbour of about K others, and a float64 exp per class costs more than a float64 load.
#include "scan_rows.h"

namespace {

constexpr int SL_MAX_K = 64;               // graph neighbours per pick
constexpr long SL_MAX_N = 2147483647L;     // picks: an int32 table entry names one

// the workspace: prob (N, H C) float64, the softmax of every row and head, at its start; behind it the partial sums (part_l over
// the chunk's rows and their table entries)
ScanParts graph_carve(void* ws, long N, int C, int H) {
    const size_t o_p = mi_align_up(sizeof(double) * (size_t)N * (size_t)H * (size_t)C, 256);
    ScanParts w = scan_carve_parts(ws ? (unsigned char*)ws + o_p : nullptr, scan_chunks(N), H);
    w.bytes += o_p;
    return w;
}

// first launch: the probabilities of every (row, head) into the workspace, and their sum over the chunk's rows
__global__ __launch_bounds__(256) void graph_prob_kernel(const float* __restrict__ z, long N, int C, int H, double* __restrict__ prob,
                                                         double* __restrict__ part_p) {
    __shared__ double sh_p[4][64];
    const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t chunk = blockIdx.x;
    const bool on = lane < C;
    const ScanRows W = scan_rows(chunk, h, N, C, H, lane);
    double ps = 0.0;
    for (int r = wave; r < W.rows; r += 4) {
        const size_t at = W.at(W.row0 + r);
        const ScanExp x = scan_row_exp(on ? z[at] : -INFINITY, on);
        const double p = x.e / x.sum;
        if (on) prob[at] = p;
        ps += p;
    }
    sh_p[wave][lane] = ps;
    __syncthreads();
    if (wave == 0) part_p[(chunk * H + h) * 64 + lane] = scan_add_waves(&sh_p[0][lane], 64);
}

// second launch: every pick against the entries of its table row ([itself,] neighbour 1..k), in that order
__global__ __launch_bounds__(256) void graph_pair_kernel(const double* __restrict__ prob, const int* __restrict__ index, long N, int C,
                                                         int H, int k, int with_self, double* __restrict__ part_l) {
    __shared__ double sh_l[4];
    const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t chunk = blockIdx.x;
    const bool on = lane < C;
    const ScanRows W = scan_rows(chunk, h, N, C, H, lane);
    double ls = 0.0;
    for (int r = wave; r < W.rows; r += 4) {
        const size_t row = (size_t)(W.row0 + r);
        const double p = on ? prob[W.at(row)] : 0.0;
        if (with_self) ls += fmax(log(wave_sum(p * p)), -100.0);
        for (int j = 0; j < k; ++j) {
            const long other = index[row * (size_t)k + j];                 // (the wrapper has checked the table: 0 <= entry < N)
            const double q = on ? prob[W.at(other)] : 0.0;
            ls += fmax(log(wave_sum(p * q)), -100.0);                      // (log 0 = -inf -> -100: torch's BCE clamp)
        }
    }
    if (lane == 0) sh_l[wave] = ls;
    __syncthreads();
    if (tid == 0) part_l[chunk * H + h] = scan_add_waves(sh_l, 1);
}

// third launch, one workgroup of H waves: wave h finishes head h, thread 0 picks the head with the lowest total
__global__ __launch_bounds__(1024) void graph_final_kernel(const double* __restrict__ part_p, const double* __restrict__ part_l, long N,
                                                           int C, int H, int K, float* __restrict__ stats, int* __restrict__ best) {
    __shared__ double totals[SCAN_MAX_H];
    const int tid = threadIdx.x, lane = tid & 63, h = tid >> 6;
    const ScanHead F = scan_head_finish(part_p, part_l, scan_chunks(N), H, h, lane, lane < C, (double)N, (double)N * (double)K);
    F.store(F.consistency - F.entropy, h, lane, stats, totals);
    __syncthreads();
    if (tid == 0) {
        int b = 0;
        for (int i = 1; i < H; ++i)
            if (totals[i] < totals[b]) b = i;              // strictly lower: the lowest index on an exact tie
        *best = b;
    }
}

// ---- self-labelling ------------------------------------------------------------------------------------------------------------

// the class weight of lane's class: 1 / (count / n) in fp32, two correctly rounded divisions (the reference forms it from
// counts.float() / n whatever the logits' type), 1 for a class no confident row targets or without balancing
__device__ __forceinline__ double selflabel_weight(int count, int n, int balance) {
    return balance && count > 0 ? (double)__fdiv_rn(1.0f, __fdiv_rn((float)count, (float)n)) : 1.0;
}

// first launch: target, mask, and the counts of the masked rows (info[0] = n)
__global__ __launch_bounds__(256) void selflabel_target_kernel(const float* __restrict__ weak, int B, int C, double threshold,
                                                               int* __restrict__ target, unsigned char* __restrict__ mask,
                                                               int* __restrict__ count, int* __restrict__ info) {
    __shared__ int hist[64];
    __shared__ int sh_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool on = lane < C;
    scan_hist_zero(hist, tid);
    if (tid == 0) sh_n = 0;
    __syncthreads();
    const ScanRows W = scan_rows(blockIdx.x, 0, B, C, 1, lane);
    for (int r = wave; r < W.rows; r += 4) {
        const long row = W.row0 + r;
        const float v = on ? weak[W.at(row)] : -INFINITY;
        const ScanExp x = scan_row_exp(v, on);
        const int c = scan_row_argmax(v, x.mx, on);                        // (a row of NaNs: class 0, not confident)
        const bool confident = 1.0 / x.sum > threshold;                    // the maximum's exp is exp(0) = 1
        if (lane == 0) {
            target[row] = c;
            mask[row] = confident ? 1 : 0;
            if (confident) {
                atomicAdd(&hist[c], 1);
                atomicAdd(&sh_n, 1);
            }
        }
    }
    __syncthreads();
    scan_hist_flush(hist, tid, C, count);
    if (tid == 0 && sh_n) atomicAdd(&info[0], sh_n);
}

// second launch (the counts are complete): per chunk the sums of w_t nll and of w_t over its masked rows
__global__ __launch_bounds__(256) void selflabel_sum_kernel(const float* __restrict__ strong, int B, int C, int balance,
                                                            const int* __restrict__ target, const unsigned char* __restrict__ mask,
                                                            const int* __restrict__ count, const int* __restrict__ info,
                                                            double* __restrict__ part) {
    __shared__ double sh[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool on = lane < C;
    const double w = selflabel_weight(on ? count[lane] : 0, info[0], balance);
    const ScanRows W = scan_rows(blockIdx.x, 0, B, C, 1, lane);
    double num = 0.0, den = 0.0;
    for (int r = wave; r < W.rows; r += 4) {
        const long row = W.row0 + r;
        if (!mask[row]) continue;                                          // (the same for every lane of the wave)
        const int t = target[row];
        const float v = on ? strong[W.at(row)] : -INFINITY;
        const ScanExp x = scan_row_exp(v, on);
        const double vt = (double)__shfl(v, t, 64), wt = __shfl(w, t, 64);
        num += wt * (log(x.sum) - (vt - (double)x.mx));                    // w_t (-log softmax(strong)_t)
        den += wt;
    }
    if (lane == 0) {
        sh[wave][0] = num;
        sh[wave][1] = den;
    }
    __syncthreads();
    if (tid < 2) part[(size_t)blockIdx.x * 2 + tid] = scan_add_waves(&sh[0][tid], 2);
}

// third launch, one wave: the chunks in ascending order, the loss, the classes present
__global__ __launch_bounds__(64) void selflabel_final_kernel(const double* __restrict__ part, int B, int C, const int* __restrict__ count,
                                                             int* __restrict__ info, float* __restrict__ loss,
                                                             double* __restrict__ denom) {
    const int lane = threadIdx.x;
    const unsigned long long present = __ballot(lane < C && count[lane] > 0);
    if (lane == 0) {
        const size_t chunks = scan_chunks(B);
        double num = 0.0, den = 0.0;
        for (size_t q = 0; q < chunks; ++q) {
            num += part[q * 2];
            den += part[q * 2 + 1];
        }
        const bool any = info[0] > 0;                                      // no confident row: loss 0, nothing divided
        *loss = any ? (float)(num / den) : 0.f;
        *denom = any ? den : 0.0;
        info[1] = __popcll(present);
        info[2] = B;
    }
}

__global__ __launch_bounds__(256) void selflabel_bwd_kernel(const float* __restrict__ strong, int B, int C, int balance,
                                                            const int* __restrict__ info, const int* __restrict__ count,
                                                            const int* __restrict__ target, const unsigned char* __restrict__ mask,
                                                            const double* __restrict__ denom, const float* __restrict__ dloss,
                                                            float* __restrict__ d_strong) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool on = lane < C;
    const int n = info[0];
    const double w = selflabel_weight(on ? count[lane] : 0, n, balance);
    const double scale = n > 0 ? (double)*dloss / *denom : 0.0;
    const ScanRows W = scan_rows(blockIdx.x, 0, B, C, 1, lane);
    for (int r = wave; r < W.rows; r += 4) {
        const long row = W.row0 + r;
        const size_t at = W.at(row);
        if (n <= 0 || !mask[row]) {
            if (on) d_strong[at] = 0.f;
            continue;
        }
        const int t = target[row];
        const ScanExp x = scan_row_exp(on ? strong[at] : -INFINITY, on);
        const double p = x.e / x.sum;
        const double wt = __shfl(w, t, 64);
        if (on) d_strong[at] = (float)(scale * wt * (p - (lane == t ? 1.0 : 0.0)));
    }
}

}  // namespace

extern "C" size_t mi_scan_graph_eval_workspace_bytes(long N, int C, int H) {
    if (!scan_sizes_ok(N, SL_MAX_N, C, H)) return 0;
    return graph_carve(nullptr, N, C, H).bytes;
}

extern "C" int mi_scan_graph_eval(const float* logits, long N, int C, int H, const int32_t* index, int k, int with_self,
                                  float* stats_out, int32_t* best_out, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!scan_sizes_ok(N, SL_MAX_N, C, H) || k < 1 || k > SL_MAX_K || !logits || !index || !stats_out || !best_out) return MI_E_ARG;
    if (!ws || ws_bytes < mi_scan_graph_eval_workspace_bytes(N, C, H)) return MI_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const ScanParts W = graph_carve(ws, N, C, H);
    double* prob = (double*)ws;
    const dim3 grid((unsigned)scan_chunks(N), (unsigned)H);
    hipLaunchKernelGGL(graph_prob_kernel, grid, dim3(256), 0, s, logits, N, C, H, prob, W.part_p);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(graph_pair_kernel, grid, dim3(256), 0, s, (const double*)prob, (const int*)index, N, C, H, k,
                       with_self ? 1 : 0, W.part_l);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(graph_final_kernel, dim3(1), dim3(64 * (unsigned)H), 0, s, (const double*)W.part_p, (const double*)W.part_l, N,
                       C, H, k + (with_self ? 1 : 0), stats_out, (int*)best_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" size_t mi_scan_selflabel_workspace_bytes(int B, int C) {
    if (!scan_sizes_ok(B, SCAN_MAX_B, C, 1)) return 0;
    return mi_align_up(sizeof(double) * 2 * scan_chunks(B), 256);
}

extern "C" int mi_scan_selflabel_fwd(const float* weak, const float* strong, int B, int C, double threshold, int balance,
                                     float* loss_out, int32_t* info_out, int32_t* count_out, int32_t* target_out, uint8_t* mask_out,
                                     double* denom_out, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!scan_sizes_ok(B, SCAN_MAX_B, C, 1) || !(threshold == threshold) || !weak || !strong || !loss_out || !info_out ||
        !count_out || !target_out || !mask_out || !denom_out)
        return MI_E_ARG;
    if (!ws || ws_bytes < mi_scan_selflabel_workspace_bytes(B, C)) return MI_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const unsigned chunks = (unsigned)scan_chunks(B);
    MI_HIP(hipMemsetAsync(count_out, 0, sizeof(int32_t) * (size_t)C, s));
    MI_HIP(hipMemsetAsync(info_out, 0, sizeof(int32_t) * 3, s));
    hipLaunchKernelGGL(selflabel_target_kernel, dim3(chunks), dim3(256), 0, s, weak, B, C, threshold, (int*)target_out,
                       (unsigned char*)mask_out, (int*)count_out, (int*)info_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(selflabel_sum_kernel, dim3(chunks), dim3(256), 0, s, strong, B, C, balance ? 1 : 0, (const int*)target_out,
                       (const unsigned char*)mask_out, (const int*)count_out, (const int*)info_out, (double*)ws);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(selflabel_final_kernel, dim3(1), dim3(64), 0, s, (const double*)ws, B, C, (const int*)count_out, (int*)info_out,
                       loss_out, denom_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_scan_selflabel_bwd(const float* strong, int B, int C, int balance, const int32_t* info, const int32_t* count,
                                     const int32_t* target, const uint8_t* mask, const double* denom, const float* dloss,
                                     float* d_strong, mi_stream_t stream) {
    if (!scan_sizes_ok(B, SCAN_MAX_B, C, 1) || !strong || !info || !count || !target || !mask || !denom || !dloss || !d_strong)
        return MI_E_ARG;
    hipLaunchKernelGGL(selflabel_bwd_kernel, dim3((unsigned)scan_chunks(B)), dim3(256), 0, (hipStream_t)stream, strong, B, C,
                       balance ? 1 : 0, (const int*)info, (const int*)count, (const int*)target, (const unsigned char*)mask, denom,
                       dloss, d_strong);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

// What follows SCAN's clustering step: the heads scored over the whole neighbour graph (the reference's
// scan_evaluate, trains/eval_utils.py) and the self-labelling loss (ConfidenceBasedCE + MaskedCrossEntropyLoss, models/loss.py:15-66).
//   mi_scan_graph_eval      per head the consistency over every (pick, table entry) pair, the entropy of the mean distribution,
//                           their total (weight 1), and the head with the lowest total
//   mi_scan_selflabel_fwd   one head: target and mask from the weak logits, class weights from the masked counts, the weighted
//                           mean cross-entropy of the strong logits
//   mi_scan_selflabel_bwd   its gradient with respect to the strong logits, one launch
//
// Layout and arithmetic are scan_loss.hip's: logits (rows, H C) fp32, head h in columns h C .. h C + C - 1, C <= 64, a wave per
// (row, head), lane c = class c; the row maximum on the fp32 logits, everything after it in float64, rounded once where stored.
//
// Order.  Every floating sum has a fixed order: rows of a wave ascending (table entries of a row ascending), waves 0..3, chunks of
// MI_SCAN_CHUNK rows ascending in a finalise launch of its own, heads ascending.  Only the counts of the self-label forward are
// added by (integer) atomics.  The same input gives the same bytes.
//
// The graph evaluation reads a neighbour's probabilities from a float64 workspace (N, H C) that its first launch fills: a pick is
// the neighbour of about K others, and a float64 exp per class costs more than a float64 load.
#include "common.h"

namespace {

constexpr int SL_CHUNK = MI_SCAN_CHUNK;    // rows per partial sum
constexpr int SL_MAX_C = 64;               // a class per lane
constexpr int SL_MAX_H = 16;               // a head per wave of the finalise workgroup
constexpr int SL_MAX_B = 65536;            // rows of a self-label batch
constexpr int SL_MAX_K = 64;               // graph neighbours per pick
constexpr long SL_MAX_N = 2147483647L;     // picks: an int32 table entry names one

bool graph_sizes_ok(long N, int C, int H) { return N >= 1 && N <= SL_MAX_N && C >= 1 && C <= SL_MAX_C && H >= 1 && H <= SL_MAX_H; }
bool selflabel_sizes_ok(long B, int C) { return B >= 1 && B <= SL_MAX_B && C >= 1 && C <= SL_MAX_C; }

struct GraphWs {
    double* prob;        // (N, H C): softmax of every row and head
    double* part_p;      // (chunks, H, 64): sum of p over the chunk's rows
    double* part_l;      // (chunks, H): sum of max(log s, -100) over the chunk's rows and their table entries
    size_t bytes;
};

GraphWs graph_carve(void* ws, long N, int C, int H) {
    GraphWs w = {};
    const size_t chunks = ((size_t)N + SL_CHUNK - 1) / SL_CHUNK;
    const size_t o_p = mi_align_up(sizeof(double) * (size_t)N * (size_t)H * (size_t)C, 256);
    const size_t o_l = o_p + mi_align_up(sizeof(double) * chunks * (size_t)H * 64, 256);
    w.bytes = o_l + mi_align_up(sizeof(double) * chunks * (size_t)H, 256);
    if (ws) {
        w.prob = (double*)ws;
        w.part_p = (double*)((unsigned char*)ws + o_p);
        w.part_l = (double*)((unsigned char*)ws + o_l);
    }
    return w;
}

// first launch: the probabilities of every (row, head) into the workspace, and their sum over the chunk's rows
__global__ __launch_bounds__(256) void graph_prob_kernel(const float* __restrict__ z, long N, int C, int H, double* __restrict__ prob,
                                                         double* __restrict__ part_p) {
    __shared__ double sh_p[4][64];
    const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t chunk = blockIdx.x;
    const bool on = lane < C;
    const long row0 = (long)chunk * SL_CHUNK;
    const int rows = N - row0 < SL_CHUNK ? (int)(N - row0) : SL_CHUNK;
    const size_t ld = (size_t)H * C, col = (size_t)h * C + (on ? lane : 0);
    double ps = 0.0;
    for (int r = wave; r < rows; r += 4) {
        const size_t at = (size_t)(row0 + r) * ld + col;
        const float v = on ? z[at] : -INFINITY;
        const float mx = wave_max(v);
        const double e = on ? exp((double)v - (double)mx) : 0.0;
        const double p = e / wave_sum(e);
        if (on) prob[at] = p;
        ps += p;
    }
    sh_p[wave][lane] = ps;
    __syncthreads();
    if (wave == 0) part_p[(chunk * H + h) * 64 + lane] = ((sh_p[0][lane] + sh_p[1][lane]) + sh_p[2][lane]) + sh_p[3][lane];
}

// second launch: every pick against the entries of its table row ([itself,] neighbour 1..k), in that order
__global__ __launch_bounds__(256) void graph_pair_kernel(const double* __restrict__ prob, const int* __restrict__ index, long N, int C,
                                                         int H, int k, int with_self, double* __restrict__ part_l) {
    __shared__ double sh_l[4];
    const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t chunk = blockIdx.x;
    const bool on = lane < C;
    const long row0 = (long)chunk * SL_CHUNK;
    const int rows = N - row0 < SL_CHUNK ? (int)(N - row0) : SL_CHUNK;
    const size_t ld = (size_t)H * C, col = (size_t)h * C + (on ? lane : 0);
    double ls = 0.0;
    for (int r = wave; r < rows; r += 4) {
        const size_t row = (size_t)(row0 + r);
        const double p = on ? prob[row * ld + col] : 0.0;
        if (with_self) ls += fmax(log(wave_sum(p * p)), -100.0);
        for (int j = 0; j < k; ++j) {
            const size_t other = (size_t)index[row * (size_t)k + j];       // (the wrapper has checked the table: 0 <= entry < N)
            const double q = on ? prob[other * ld + col] : 0.0;
            ls += fmax(log(wave_sum(p * q)), -100.0);                      // (log 0 = -inf -> -100: torch's BCE clamp)
        }
    }
    if (lane == 0) sh_l[wave] = ls;
    __syncthreads();
    if (tid == 0) part_l[chunk * H + h] = ((sh_l[0] + sh_l[1]) + sh_l[2]) + sh_l[3];
}

// third launch, one workgroup of H waves: wave h finishes head h, thread 0 picks the head with the lowest total
__global__ __launch_bounds__(1024) void graph_final_kernel(const double* __restrict__ part_p, const double* __restrict__ part_l, long N,
                                                           int C, int H, int K, float* __restrict__ stats, int* __restrict__ best) {
    __shared__ double totals[SL_MAX_H];
    const int tid = threadIdx.x, lane = tid & 63, h = tid >> 6;
    const size_t chunks = ((size_t)N + SL_CHUNK - 1) / SL_CHUNK;
    const bool on = lane < C;
    double sp = 0.0, sl = 0.0;
    for (size_t q = 0; q < chunks; ++q) {
        sp += part_p[(q * H + h) * 64 + lane];
        sl += part_l[q * H + h];
    }
    const double x = fmax(sp / (double)N, 1e-8);
    const double entropy = -wave_sum(on ? x * log(x) : 0.0);
    const double consistency = -sl / ((double)N * (double)K);
    const double total = consistency - entropy;
    if (lane == 0) {
        stats[3 * h] = (float)total;
        stats[3 * h + 1] = (float)consistency;
        stats[3 * h + 2] = (float)entropy;
        totals[h] = total;
    }
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
    if (tid < 64) hist[tid] = 0;
    if (tid == 0) sh_n = 0;
    __syncthreads();
    const int row0 = blockIdx.x * SL_CHUNK;
    const int rows = B - row0 < SL_CHUNK ? B - row0 : SL_CHUNK;
    for (int r = wave; r < rows; r += 4) {
        const size_t row = (size_t)(row0 + r);
        const float v = on ? weak[row * C + lane] : -INFINITY;
        const float mx = wave_max(v);
        const unsigned long long top = __ballot(on && v == mx);            // (empty only for a row of NaNs: class 0, not confident)
        const int c = top ? __ffsll((long long)top) - 1 : 0;
        const double sum = wave_sum(on ? exp((double)v - (double)mx) : 0.0);
        const bool confident = 1.0 / sum > threshold;                      // the maximum's exp is exp(0) = 1
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
    if (tid < C && hist[tid]) atomicAdd(&count[tid], hist[tid]);
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
    const int row0 = blockIdx.x * SL_CHUNK;
    const int rows = B - row0 < SL_CHUNK ? B - row0 : SL_CHUNK;
    double num = 0.0, den = 0.0;
    for (int r = wave; r < rows; r += 4) {
        const size_t row = (size_t)(row0 + r);
        if (!mask[row]) continue;                                          // (the same for every lane of the wave)
        const int t = target[row];
        const float v = on ? strong[row * C + lane] : -INFINITY;
        const float mx = wave_max(v);
        const double sum = wave_sum(on ? exp((double)v - (double)mx) : 0.0);
        const double vt = (double)__shfl(v, t, 64), wt = __shfl(w, t, 64);
        num += wt * (log(sum) - (vt - (double)mx));                        // w_t (-log softmax(strong)_t)
        den += wt;
    }
    if (lane == 0) {
        sh[wave][0] = num;
        sh[wave][1] = den;
    }
    __syncthreads();
    if (tid < 2) part[(size_t)blockIdx.x * 2 + tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
}

// third launch, one wave: the chunks in ascending order, the loss, the classes present
__global__ __launch_bounds__(64) void selflabel_final_kernel(const double* __restrict__ part, int B, int C, const int* __restrict__ count,
                                                             int* __restrict__ info, float* __restrict__ loss,
                                                             double* __restrict__ denom) {
    const int lane = threadIdx.x;
    const unsigned long long present = __ballot(lane < C && count[lane] > 0);
    if (lane == 0) {
        const int chunks = (B + SL_CHUNK - 1) / SL_CHUNK;
        double num = 0.0, den = 0.0;
        for (int q = 0; q < chunks; ++q) {
            num += part[(size_t)q * 2];
            den += part[(size_t)q * 2 + 1];
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
    const int row0 = blockIdx.x * SL_CHUNK;
    const int rows = B - row0 < SL_CHUNK ? B - row0 : SL_CHUNK;
    for (int r = wave; r < rows; r += 4) {
        const size_t row = (size_t)(row0 + r);
        if (n <= 0 || !mask[row]) {
            if (on) d_strong[row * C + lane] = 0.f;
            continue;
        }
        const int t = target[row];
        const float v = on ? strong[row * C + lane] : -INFINITY;
        const float mx = wave_max(v);
        const double e = on ? exp((double)v - (double)mx) : 0.0;
        const double p = e / wave_sum(e);
        const double wt = __shfl(w, t, 64);
        if (on) d_strong[row * C + lane] = (float)(scale * wt * (p - (lane == t ? 1.0 : 0.0)));
    }
}

}  // namespace

extern "C" size_t mi_scan_graph_eval_workspace_bytes(long N, int C, int H) {
    if (!graph_sizes_ok(N, C, H)) return 0;
    return graph_carve(nullptr, N, C, H).bytes;
}

extern "C" int mi_scan_graph_eval(const float* logits, long N, int C, int H, const int32_t* index, int k, int with_self,
                                  float* stats_out, int32_t* best_out, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!graph_sizes_ok(N, C, H) || k < 1 || k > SL_MAX_K || !logits || !index || !stats_out || !best_out) return MI_E_ARG;
    if (!ws || ws_bytes < mi_scan_graph_eval_workspace_bytes(N, C, H)) return MI_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const GraphWs W = graph_carve(ws, N, C, H);
    const dim3 grid((unsigned)((N + SL_CHUNK - 1) / SL_CHUNK), (unsigned)H);
    hipLaunchKernelGGL(graph_prob_kernel, grid, dim3(256), 0, s, logits, N, C, H, W.prob, W.part_p);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(graph_pair_kernel, grid, dim3(256), 0, s, (const double*)W.prob, (const int*)index, N, C, H, k,
                       with_self ? 1 : 0, W.part_l);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(graph_final_kernel, dim3(1), dim3(64 * (unsigned)H), 0, s, (const double*)W.part_p, (const double*)W.part_l, N,
                       C, H, k + (with_self ? 1 : 0), stats_out, (int*)best_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" size_t mi_scan_selflabel_workspace_bytes(int B, int C) {
    if (!selflabel_sizes_ok(B, C)) return 0;
    return mi_align_up(sizeof(double) * 2 * (size_t)mi_cdiv(B, SL_CHUNK), 256);
}

extern "C" int mi_scan_selflabel_fwd(const float* weak, const float* strong, int B, int C, double threshold, int balance,
                                     float* loss_out, int32_t* info_out, int32_t* count_out, int32_t* target_out, uint8_t* mask_out,
                                     double* denom_out, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!selflabel_sizes_ok(B, C) || !(threshold == threshold) || !weak || !strong || !loss_out || !info_out || !count_out ||
        !target_out || !mask_out || !denom_out)
        return MI_E_ARG;
    if (!ws || ws_bytes < mi_scan_selflabel_workspace_bytes(B, C)) return MI_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const unsigned chunks = (unsigned)mi_cdiv(B, SL_CHUNK);
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
    if (!selflabel_sizes_ok(B, C) || !strong || !info || !count || !target || !mask || !denom || !dloss || !d_strong) return MI_E_ARG;
    hipLaunchKernelGGL(selflabel_bwd_kernel, dim3((unsigned)mi_cdiv(B, SL_CHUNK)), dim3(256), 0, (hipStream_t)stream, strong, B, C,
                       balance ? 1 : 0, (const int*)info, (const int*)count, (const int*)target, (const unsigned char*)mask, denom,
                       dloss, d_strong);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

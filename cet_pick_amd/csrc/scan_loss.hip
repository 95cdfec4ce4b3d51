// The SCAN step on stored embeddings ("learning to classify by nearest neighbours": the reference's models/loss.py SCANLoss and
// entropy, summed over the heads as its TomoSCANLoss does), DESIGN.md 4.25:
//   mi_scan_loss_fwd   per head the consistency of anchor and neighbour, the entropy of the mean anchor distribution, their total;
//                      and the sum of the totals over the heads
//   mi_scan_loss_bwd   the gradient of that sum with respect to both logits tensors, one launch
//   mi_scan_assign     per row and head the class (argmax, lowest index on a tie), its probability, optionally all
//                      probabilities, and the class counts
//
// Layout.  Logits are (B, H C) fp32, head h owns columns h C .. h C + C - 1, C <= 64: a wave takes one (row, head) at a time, lane c
// holds class c.  The softmax is max-subtracted; the maximum is taken on the fp32 logits (exact), everything after it runs in
// float64 and is rounded to fp32 once, where it is stored.
//
// Order.  Workgroup (chunk, head) of the forward walks MI_SCAN_CHUNK rows: wave w takes the rows w, w + 4, ... of the chunk in
// ascending order and keeps one running sum of p per lane and one of max(log s, -100); the four waves' sums are added w = 0..3 into
// one partial sum per (chunk, head, class).  A second launch of ONE workgroup (wave h = head h) adds the partial sums chunk by
// chunk, finishes the three figures of its head, and thread 0 adds the totals h = 0..H-1.  Nothing floating is added by an
// atomic: the same input gives the same bytes.  The backward pass has no sum across rows at all.  mi_scan_assign counts classes
// with integer atomics (a count does not depend on the order of arrival).
#include "common.h"

namespace {

constexpr int SCAN_CHUNK = MI_SCAN_CHUNK;  // rows per partial sum
constexpr int SCAN_MAX_C = 64;             // a class per lane
constexpr int SCAN_MAX_H = 16;             // a head per wave of the finalise workgroup
constexpr int SCAN_MAX_B = 65536;
constexpr int SCAN_ASSIGN_BLOCKS = 4096;   // grid-stride over the rows above that
constexpr double SCAN_BCE_FLOOR = (double)1e-12f;      // 1e-12 as torch holds it, a float constant in float64 too: 9.99999996e-13

bool scan_sizes_ok(long B, int C, int H) { return B >= 1 && B <= SCAN_MAX_B && C >= 1 && C <= SCAN_MAX_C && H >= 1 && H <= SCAN_MAX_H; }

struct ScanWs {
    double* part_p;      // (chunks, H, 64): sum of p over the chunk's rows
    double* part_l;      // (chunks, H): sum of max(log s, -100)
    size_t bytes;
};

ScanWs scan_carve(void* ws, int B, int H) {
    ScanWs w = {};
    const size_t chunks = (size_t)mi_cdiv(B, SCAN_CHUNK);
    const size_t o_l = mi_align_up(sizeof(double) * chunks * (size_t)H * 64, 256);
    w.bytes = o_l + mi_align_up(sizeof(double) * chunks * (size_t)H, 256);
    if (ws) {
        w.part_p = (double*)ws;
        w.part_l = (double*)((unsigned char*)ws + o_l);
    }
    return w;
}

// softmax of lane's logit among the first C lanes: z is read only where on; every lane gets the same maximum and sum
__device__ __forceinline__ double scan_softmax(float z, bool on) {
    const float mx = wave_max(on ? z : -INFINITY);
    const double e = on ? exp((double)z - (double)mx) : 0.0;
    return e / wave_sum(e);
}

__global__ __launch_bounds__(256) void scan_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int B, int C, int H,
                                                       double* __restrict__ part_p, double* __restrict__ part_l) {
    __shared__ double sh_p[4][64];
    __shared__ double sh_l[4];
    const int chunk = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool on = lane < C;
    const int row0 = chunk * SCAN_CHUNK;
    const int rows = B - row0 < SCAN_CHUNK ? B - row0 : SCAN_CHUNK;
    const size_t ld = (size_t)H * C, col = (size_t)h * C + (on ? lane : 0);
    double ps = 0.0, ls = 0.0;
    for (int r = wave; r < rows; r += 4) {
        const size_t at = (size_t)(row0 + r) * ld + col;
        const double p = scan_softmax(on ? a[at] : 0.f, on), q = scan_softmax(on ? b[at] : 0.f, on);
        const double s = wave_sum(p * q);
        ps += p;
        ls += fmax(log(s), -100.0);                        // (log 0 = -inf -> -100: torch's BCELoss clamp)
    }
    sh_p[wave][lane] = ps;
    if (lane == 0) sh_l[wave] = ls;
    __syncthreads();
    if (wave == 0) {
        part_p[((size_t)chunk * H + h) * 64 + lane] = ((sh_p[0][lane] + sh_p[1][lane]) + sh_p[2][lane]) + sh_p[3][lane];
        if (lane == 0) part_l[(size_t)chunk * H + h] = ((sh_l[0] + sh_l[1]) + sh_l[2]) + sh_l[3];
    }
}

// one workgroup of H waves: wave h finishes head h, thread 0 adds the totals in head order
__global__ __launch_bounds__(1024) void scan_final_kernel(const double* __restrict__ part_p, const double* __restrict__ part_l,
                                                          int B, int C, int H, double entropy_weight, float* __restrict__ stats,
                                                          float* __restrict__ loss, double* __restrict__ mean) {
    __shared__ double totals[SCAN_MAX_H];
    const int tid = threadIdx.x, lane = tid & 63, h = tid >> 6;
    const int chunks = (B + SCAN_CHUNK - 1) / SCAN_CHUNK;
    const bool on = lane < C;
    double sp = 0.0, sl = 0.0;
    for (int q = 0; q < chunks; ++q) {
        sp += part_p[((size_t)q * H + h) * 64 + lane];
        sl += part_l[(size_t)q * H + h];
    }
    const double m = sp / (double)B;
    const double x = fmax(m, 1e-8);
    const double entropy = -wave_sum(on ? x * log(x) : 0.0);
    const double consistency = -sl / (double)B;
    const double total = consistency - entropy_weight * entropy;
    if (on) mean[(size_t)h * C + lane] = m;
    if (lane == 0) {
        stats[3 * h] = (float)total;
        stats[3 * h + 1] = (float)consistency;
        stats[3 * h + 2] = (float)entropy;
        totals[h] = total;
    }
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
    const int row0 = chunk * SCAN_CHUNK;
    const int rows = B - row0 < SCAN_CHUNK ? B - row0 : SCAN_CHUNK;
    const size_t ld = (size_t)H * C, col = (size_t)h * C + (on ? lane : 0);
    const double up = (double)*dloss, inv_b = 1.0 / (double)B;
    const double m = on ? mean[(size_t)h * C + lane] : 1.0;
    const double gm = on && m >= 1e-8 ? entropy_weight * (log(m) + 1.0) * inv_b : 0.0;   // d total / d p_ic through the mean
    for (int r = wave; r < rows; r += 4) {
        const size_t at = (size_t)(row0 + r) * ld + col;
        const double p = scan_softmax(on ? a[at] : 0.f, on), q = scan_softmax(on ? b[at] : 0.f, on);
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
    if (tid < 64) hist[tid] = 0;
    __syncthreads();
    const size_t ld = (size_t)H * C, col = (size_t)h * C + (on ? lane : 0);
    for (long row = (long)blockIdx.x * 4 + wave; row < n; row += (long)gridDim.x * 4) {
        const size_t at = (size_t)row * ld + col;
        const float v = on ? z[at] : -INFINITY;
        const float mx = wave_max(v);
        const unsigned long long best = __ballot(on && v == mx);       // (empty only for a row of NaNs: class 0)
        const int c = best ? __ffsll((long long)best) - 1 : 0;
        const double e = on ? exp((double)v - (double)mx) : 0.0;
        const double sum = wave_sum(e);
        if (prob && on) prob[at] = (float)(e / sum);
        if (lane == c) {
            cls[(size_t)row * H + h] = c;
            conf[(size_t)row * H + h] = (float)(e / sum);
            atomicAdd(&hist[c], 1);
        }
    }
    __syncthreads();
    if (tid < C && hist[tid]) atomicAdd(&counts[(size_t)h * C + tid], hist[tid]);
}

}  // namespace

extern "C" size_t mi_scan_loss_workspace_bytes(int B, int C, int H) {
    if (!scan_sizes_ok(B, C, H)) return 0;
    return scan_carve(nullptr, B, H).bytes;
}

extern "C" int mi_scan_loss_fwd(const float* anchors, const float* neighbours, int B, int C, int H, double entropy_weight,
                                float* stats_out, float* loss_out, double* mean_out, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!scan_sizes_ok(B, C, H) || !anchors || !neighbours || !stats_out || !loss_out || !mean_out) return MI_E_ARG;
    if (!ws || ws_bytes < mi_scan_loss_workspace_bytes(B, C, H)) return MI_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const ScanWs W = scan_carve(ws, B, H);
    hipLaunchKernelGGL(scan_fwd_kernel, dim3((unsigned)mi_cdiv(B, SCAN_CHUNK), (unsigned)H), dim3(256), 0, s, anchors, neighbours, B,
                       C, H, W.part_p, W.part_l);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(scan_final_kernel, dim3(1), dim3(64 * (unsigned)H), 0, s, (const double*)W.part_p, (const double*)W.part_l, B,
                       C, H, entropy_weight, stats_out, loss_out, mean_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_scan_loss_bwd(const float* anchors, const float* neighbours, int B, int C, int H, double entropy_weight,
                                const double* mean, const float* dloss, float* d_anchors, float* d_neighbours, mi_stream_t stream) {
    if (!scan_sizes_ok(B, C, H) || !anchors || !neighbours || !mean || !dloss || !d_anchors || !d_neighbours) return MI_E_ARG;
    hipLaunchKernelGGL(scan_bwd_kernel, dim3((unsigned)mi_cdiv(B, SCAN_CHUNK), (unsigned)H), dim3(256), 0, (hipStream_t)stream,
                       anchors, neighbours, B, C, H, entropy_weight, mean, dloss, d_anchors, d_neighbours);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_scan_assign(const float* logits, long n, int C, int H, int32_t* class_out, float* conf_out, float* prob_out,
                              int32_t* counts_out, mi_stream_t stream) {
    if (n < 1 || C < 1 || C > SCAN_MAX_C || H < 1 || H > SCAN_MAX_H) return MI_E_ARG;
    if (!logits || !class_out || !conf_out || !counts_out) return MI_E_ARG;
    const hipStream_t s = (hipStream_t)stream;
    MI_HIP(hipMemsetAsync(counts_out, 0, sizeof(int32_t) * (size_t)H * C, s));
    const unsigned blocks = (unsigned)std::min<long>(SCAN_ASSIGN_BLOCKS, (n + 3) / 4);
    hipLaunchKernelGGL(scan_assign_kernel, dim3(blocks, (unsigned)H), dim3(256), 0, s, logits, n, C, H, (int*)class_out, conf_out,
                       prob_out, (int*)counts_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

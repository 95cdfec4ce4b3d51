// How the SCAN kernels (scan_loss.hip, scan_selflabel.hip) walk logits, written once.
//
// Layout.  Logits are (rows, H C) fp32, head h owns columns h C .. h C + C - 1, C <= 64: a wave takes one (row, head) at a time,
// lane c holds class c (`on` = lane < C).  The softmax is max-subtracted; the maximum is taken on the fp32 logits (exact),
// everything after it runs in float64 and is rounded to fp32 once, where it is stored.  A one-head kernel is H = 1, h = 0.
//
// Order.  Every floating sum has a fixed order: a workgroup of four waves walks a chunk of MI_SCAN_CHUNK rows, wave w the rows
// w, w + 4, ... ascending into running sums of its own; the waves' sums are added ((w0 + w1) + w2) + w3 into one partial sum per
// chunk; a finalise launch of ONE workgroup (wave h = head h) adds the chunks ascending, and its thread 0 walks the heads
// ascending.  Nothing floating is added by an atomic: the same input gives the same bytes.  Only class counts go through
// (integer) atomics - a count does not depend on the order of arrival.
#pragma once
#include "common.h"

constexpr int SCAN_CHUNK = MI_SCAN_CHUNK;  // rows per partial sum
constexpr int SCAN_MAX_C = 64;             // a class per lane
constexpr int SCAN_MAX_H = 16;             // a head per wave of the finalise workgroup
constexpr int SCAN_MAX_B = 65536;          // rows of a training batch

static inline bool scan_sizes_ok(long rows, long max_rows, int C, int H) {
    return rows >= 1 && rows <= max_rows && C >= 1 && C <= SCAN_MAX_C && H >= 1 && H <= SCAN_MAX_H;
}
__host__ __device__ static inline size_t scan_chunks(long rows) { return ((size_t)rows + SCAN_CHUNK - 1) / SCAN_CHUNK; }

// the partial sums of `chunks` chunks and H heads, carved from ws (sizes only when ws is null)
struct ScanParts {
    double* part_p;      // (chunks, H, 64): sum of p over the chunk's rows
    double* part_l;      // (chunks, H): sum of max(log s, -100) over the chunk's rows
    size_t bytes;
};
static inline ScanParts scan_carve_parts(void* ws, size_t chunks, int H) {
    ScanParts w = {};
    const size_t o_l = mi_align_up(sizeof(double) * chunks * (size_t)H * 64, 256);
    w.bytes = o_l + mi_align_up(sizeof(double) * chunks * (size_t)H, 256);
    if (ws) {
        w.part_p = (double*)ws;
        w.part_l = (double*)((unsigned char*)ws + o_l);
    }
    return w;
}

// the rows of a (chunk, head) workgroup: wave w walks r = w, w + 4, ... < rows, row = row0 + r; at(row) is lane's logit
struct ScanRows {
    long row0;
    int rows;
    size_t ld, col;
    __device__ __forceinline__ size_t at(long row) const { return (size_t)row * ld + col; }
};
__device__ __forceinline__ ScanRows scan_rows(size_t chunk, int h, long total, int C, int H, int lane) {
    const long row0 = (long)chunk * SCAN_CHUNK;
    return ScanRows{row0, total - row0 < SCAN_CHUNK ? (int)(total - row0) : SCAN_CHUNK, (size_t)H * C,
                    (size_t)h * C + (lane < C ? lane : 0)};
}

// the row's exponentials: v is read only where on; every lane gets the same maximum and sum.  p = e / sum, max p = 1.0 / sum
struct ScanExp { float mx; double e, sum; };
__device__ __forceinline__ ScanExp scan_row_exp(float v, bool on) {
    const float mx = wave_max(on ? v : -INFINITY);
    const double e = on ? exp((double)v - (double)mx) : 0.0;
    return ScanExp{mx, e, wave_sum(e)};
}

// the row's argmax: the lowest index on a tie; class 0 for a row without a maximum (a row of NaNs)
__device__ __forceinline__ int scan_row_argmax(float v, float mx, bool on) {
    const unsigned long long top = __ballot(on && v == mx);
    return top ? __ffsll((long long)top) - 1 : 0;
}

// the four waves' sums s[0], s[stride], ... (LDS, after a barrier) in wave order
__device__ __forceinline__ double scan_add_waves(const double* s, int stride) {
    return ((s[0] + s[stride]) + s[2 * stride]) + s[3 * stride];
}

// wave h of the finalise workgroup: the chunks of head h in ascending order -> lane's mean probability, the entropy of the mean
// distribution, the consistency; store() writes the head's three figures and leaves `total` for thread 0
struct ScanHead {
    double mean, entropy, consistency;
    __device__ __forceinline__ void store(double total, int h, int lane, float* stats, double* totals) const {
        if (lane == 0) {
            stats[3 * h] = (float)total;
            stats[3 * h + 1] = (float)consistency;
            stats[3 * h + 2] = (float)entropy;
            totals[h] = total;
        }
    }
};
__device__ __forceinline__ ScanHead scan_head_finish(const double* __restrict__ part_p, const double* __restrict__ part_l,
                                                     size_t chunks, int H, int h, int lane, bool on, double mean_div,
                                                     double consistency_div) {
    double sp = 0.0, sl = 0.0;
    for (size_t q = 0; q < chunks; ++q) {
        sp += part_p[(q * H + h) * 64 + lane];
        sl += part_l[q * H + h];
    }
    const double m = sp / mean_div;
    const double x = fmax(m, 1e-8);
    return ScanHead{m, -wave_sum(on ? x * log(x) : 0.0), -sl / consistency_div};
}

// the workgroup's class histogram in LDS (int hist[64]): zero, barrier, count, barrier, flush the non-zero bins
__device__ __forceinline__ void scan_hist_zero(int* hist, int tid) {
    if (tid < 64) hist[tid] = 0;
}
__device__ __forceinline__ void scan_hist_flush(const int* hist, int tid, int C, int* __restrict__ counts) {
    if (tid < C && hist[tid]) atomicAdd(&counts[tid], hist[tid]);
}

// The class gallery of plot_2d --class_gallery (this project's own: the reference chooses classes in a Phoenix session), DESIGN.md 4.24:
//   mi_gallery_moments    per class the member count and, per pixel, the mean and the population deviation of the members' patches
//   mi_gallery_exemplars  per class the m members nearest to their own centroid, by (squared distance, pick index)
//   mi_gallery_raster     one picture row per class: number and count, mean patch, deviation patch, the first exemplars
//
// Order.  Both reductions start from the same counting sort of the picks by class: a histogram (integer atomics: a count does not
// depend on the order of arrival), an exclusive scan by one workgroup, and a scatter in which workgroup c walks the labels front to
// back and writes the members of class c in ascending pick index (their places come from a prefix sum, not from an atomic).  Every
// float64 sum then runs over a class's bucket in that order: GAL_CHUNK members at a time, one after the other, into one partial sum
// per (chunk, pixel); a second launch adds a class's partial sums in chunk order.  Nothing floating is added by an atomic, so the
// same input gives the same bytes.  The deviation takes two passes: the float64 mean first, then the squared distances from it.
//
// Exemplars.  One workgroup per class walks the bucket 256 members at a time, one member per thread: d2 = sum_j (x_j - c_j)^2 in
// float64, j ascending, every product and sum rounded on its own (this file is compiled with contraction off, so numpy's
// operations give the same doubles).  The best 64 so far sit sorted in LDS; a tile in which no member beats the m-th best is
// dropped after one vote, any other is merged by a bitonic sort of 512 (distance bits, pick index) keys.  The bits of a double
// that is not negative order as the double does; a NaN distance counts as +inf.
//
// Raster.  All of it float32, operation by operation (DESIGN.md 4.24 states the chain), so numpy's float32 gives the same bytes.
// hipcc-flags: -ffp-contract=off
#include "common.h"

namespace {

constexpr int GAL_CHUNK = 256;             // members per partial sum
constexpr long GAL_MAX_N = 1L << 24;
constexpr int GAL_MAX_K = 4096;            // classes (the histogram of a workgroup sits in LDS)
constexpr int GAL_MAX_M = 64;
constexpr int GAL_MAX_PIXELS = 1 << 20;
constexpr int GAL_SCATTER_THREADS = 1024, GAL_SCATTER_TILE = 4 * GAL_SCATTER_THREADS;
constexpr unsigned long long GAL_INF_BITS = 0x7ff0000000000000ull;
constexpr int GAL_NO_PICK = 0x7fffffff;

// the picture: fixed sizes in pixels (cet_pick_amd/utils/plot2d.py gallery_layout has the same numbers)
constexpr int GAL_PAD = 4, GAL_GLYPH_PX = 2, GAL_GLYPH_GAP = 2, GAL_TEXT_DIGITS = 8, GAL_LINE_GAP = 4;
constexpr int GAL_DIGIT_PITCH = 5 * GAL_GLYPH_PX + GAL_GLYPH_GAP;                     // 12
constexpr int GAL_TEXT_W = GAL_TEXT_DIGITS * GAL_DIGIT_PITCH - GAL_GLYPH_GAP;         // 94
constexpr int GAL_LINE_H = 7 * GAL_GLYPH_PX;                                          // 14
constexpr int GAL_TEXT_H = 2 * GAL_LINE_H + GAL_LINE_GAP;                             // 32

struct GalWs {
    int* cnt;            // k + 1 (the last one unused: zero)
    int* start;          // k + 1: where a class's bucket starts in `sorted`
    int* chunk_start;    // k + 1: where a class's partial sums start
    int* sorted;         // n: pick indices by class, ascending inside a class
    double* mean_d;      // k b
    double* partial;     // (n / GAL_CHUNK + k) b
    size_t bytes;
};

GalWs gal_carve(void* ws, long n, int k, int b) {
    GalWs g = {};
    const size_t kk = mi_align_up(sizeof(int) * ((size_t)k + 1), 256);
    const size_t o_sorted = 3 * kk, o_mean = o_sorted + mi_align_up(sizeof(int) * (size_t)n, 256);
    const size_t o_partial = o_mean + mi_align_up(sizeof(double) * (size_t)k * (size_t)b, 256);
    g.bytes = o_partial + mi_align_up(sizeof(double) * ((size_t)(n / GAL_CHUNK) + (size_t)k) * (size_t)b, 256);
    if (ws) {                                              // (the size query carves nothing)
        unsigned char* p = (unsigned char*)ws;
        g.cnt = (int*)p, g.start = (int*)(p + kk), g.chunk_start = (int*)(p + 2 * kk);
        g.sorted = (int*)(p + o_sorted), g.mean_d = (double*)(p + o_mean), g.partial = (double*)(p + o_partial);
    }
    return g;
}

bool gal_sizes_ok(long n, int k, int b, int m) {
    return n > 0 && n <= GAL_MAX_N && k > 0 && k <= GAL_MAX_K && b >= 0 && b <= GAL_MAX_PIXELS && m >= 1 && m <= GAL_MAX_M;
}

// cnt[c] = members of class c; cnt holds zeros on entry.  A label outside [0, k) is counted nowhere.
__global__ __launch_bounds__(256) void gal_hist_kernel(const int* __restrict__ labels, int n, int k, int per_block,
                                                       int* __restrict__ cnt) {
    __shared__ int h[GAL_MAX_K];
    const int tid = threadIdx.x;
    for (int c = tid; c < k; c += 256) h[c] = 0;
    __syncthreads();
    const long lo = (long)blockIdx.x * per_block;
    const long hi = lo + per_block < n ? lo + per_block : n;
    for (long i = lo + tid; i < hi; i += 256) {
        const int c = labels[i];
        if (c >= 0 && c < k) atomicAdd(&h[c], 1);
    }
    __syncthreads();
    for (int c = tid; c < k; c += 256)
        if (h[c]) atomicAdd(&cnt[c], h[c]);
}

// one workgroup of 256: start and chunk_start, the exclusive sums of cnt and of ceil(cnt / GAL_CHUNK); entry k holds the totals
__global__ __launch_bounds__(256) void gal_scan_kernel(const int* __restrict__ cnt, int k, int* __restrict__ start,
                                                       int* __restrict__ chunk_start) {
    __shared__ int wave_a[4], wave_b[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (k + 255) / 256;                       // <= 16 classes per thread, consecutive
    const int c0 = tid * per, c1 = c0 + per < k ? c0 + per : k;
    int a = 0, b = 0;
    for (int c = c0; c < c1; ++c) {
        a += cnt[c];
        b += (cnt[c] + GAL_CHUNK - 1) / GAL_CHUNK;
    }
    int ia = a, ib = b;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int ua = __shfl_up(ia, o, 64), ub = __shfl_up(ib, o, 64);
        if (lane >= o) { ia += ua; ib += ub; }
    }
    if (lane == 63) { wave_a[wave] = ia; wave_b[wave] = ib; }
    __syncthreads();
    int ea = ia - a, eb = ib - b;
    for (int w = 0; w < wave; ++w) { ea += wave_a[w]; eb += wave_b[w]; }
    for (int c = c0; c < c1; ++c) {
        start[c] = ea;
        chunk_start[c] = eb;
        ea += cnt[c];
        eb += (cnt[c] + GAL_CHUNK - 1) / GAL_CHUNK;
    }
    if (tid == 255) {                                      // the last thread's running sums are the totals (its range may be empty)
        start[k] = ea;
        chunk_start[k] = eb;
    }
}

// workgroup c: the members of class c in ascending pick index, at sorted[start[c] ...]
__global__ __launch_bounds__(GAL_SCATTER_THREADS) void gal_scatter_kernel(const int* __restrict__ labels, int n,
                                                                          const int* __restrict__ start,
                                                                          int* __restrict__ sorted) {
    __shared__ int wave_tot[GAL_SCATTER_THREADS / 64];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = start[c], members = start[c + 1] - base;
    int done = 0;
    for (int t0 = 0; t0 < n && done < members; t0 += GAL_SCATTER_TILE) {              // (uniform: done is the same on every thread)
        const int i0 = t0 + 4 * tid;
        bool hit[4];
        int mine = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            hit[u] = i0 + u < n && labels[i0 + u] == c;
            mine += hit[u];
        }
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < GAL_SCATTER_THREADS / 64; ++w) {
            if (w < wave) before += wave_tot[w];
            all += wave_tot[w];
        }
        int at = done + before + incl - mine;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (hit[u] && at < members) sorted[base + at++] = i0 + u;                 // (at < members always: the histogram counted them)
        done += all;
        __syncthreads();
    }
}

// block (q, tile): the sum over the members of chunk q, in bucket order, of x (mean_d null) or of (x - mean)^2, for 256 pixels
__global__ __launch_bounds__(256) void gal_partial_kernel(const float* __restrict__ patches, const int* __restrict__ sorted,
                                                          const int* __restrict__ start, const int* __restrict__ chunk_start,
                                                          int k, int b, const double* __restrict__ mean_d,
                                                          double* __restrict__ partial) {
    __shared__ int ids[GAL_CHUNK];
    const int q = blockIdx.x, tid = threadIdx.x;
    if (q >= chunk_start[k]) return;
    int lo = 0, hi = k - 1;                                // the class c with chunk_start[c] <= q < chunk_start[c + 1]
    while (lo < hi) {                                      // <= 12 trips
        const int mid = (lo + hi + 1) >> 1;
        if (chunk_start[mid] <= q) lo = mid; else hi = mid - 1;
    }
    const int c = lo;
    const int m0 = start[c] + (q - chunk_start[c]) * GAL_CHUNK;
    const int m1 = m0 + GAL_CHUNK < start[c + 1] ? m0 + GAL_CHUNK : start[c + 1];
    if (m0 + tid < m1) ids[tid] = sorted[m0 + tid];
    __syncthreads();
    const int p = blockIdx.y * 256 + tid;
    if (p >= b) return;
    const int len = m1 - m0;
    double s = 0.0;
    if (mean_d) {
        const double mu = mean_d[(size_t)c * b + p];
        for (int t = 0; t < len; ++t) {
            const double d = (double)patches[(size_t)ids[t] * b + p] - mu;
            s += d * d;
        }
    } else {
        for (int t = 0; t < len; ++t) s += (double)patches[(size_t)ids[t] * b + p];
    }
    partial[(size_t)q * b + p] = s;
}

// block (tile, c): a class's partial sums added in chunk order.  pass 0: the float64 mean (kept) and mean_out, count_out;
// pass 1: std_out = sqrt(sum / count)
__global__ __launch_bounds__(256) void gal_final_kernel(const double* __restrict__ partial, const int* __restrict__ chunk_start,
                                                        const int* __restrict__ cnt, int b, int pass, double* __restrict__ mean_d,
                                                        float* __restrict__ out, int* __restrict__ count_out) {
    const int c = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    const int members = cnt[c];
    if (pass == 0 && p == 0) count_out[c] = members;
    if (p >= b) return;
    double s = 0.0;
    for (int q = chunk_start[c]; q < chunk_start[c + 1]; ++q) s += partial[(size_t)q * b + p];
    if (pass == 0) {
        const double mu = members > 0 ? s / (double)members : 0.0;
        mean_d[(size_t)c * b + p] = mu;
        out[(size_t)c * b + p] = (float)mu;
    } else {
        out[(size_t)c * b + p] = members > 0 ? (float)sqrt(s / (double)members) : 0.f;
    }
}

__device__ __forceinline__ bool gal_key_less(unsigned long long da, int ia, unsigned long long db, int ib) {
    return da < db || (da == db && ia < ib);
}

// 512 (distance bits, pick) keys in LDS, ascending, by 256 threads; ends with a barrier
__device__ __forceinline__ void gal_sort512(unsigned long long* kd, int* ki, int tid) {
    for (int k2 = 2; k2 <= 512; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const int i = ((tid / j) * (j << 1)) + (tid % j), l = i + j;
            const bool asc = (i & k2) == 0;
            const unsigned long long da = kd[i], db = kd[l];
            const int ia = ki[i], ib = ki[l];
            const bool swap = asc ? gal_key_less(db, ib, da, ia) : gal_key_less(da, ia, db, ib);
            if (swap) {
                kd[i] = db; ki[i] = ib;
                kd[l] = da; ki[l] = ia;
            }
            __syncthreads();
        }
    }
}

// workgroup c: the m members of class c nearest to the centroid they are assigned to
__global__ __launch_bounds__(256) void gal_exemplar_kernel(const float* __restrict__ emb, const float* __restrict__ centroids,
                                                           const int* __restrict__ assign, const int* __restrict__ sorted,
                                                           const int* __restrict__ start, int dim, int k_centroids, int m,
                                                           int* __restrict__ idx_out, double* __restrict__ d2_out) {
    __shared__ unsigned long long kd[512];
    __shared__ int ki[512];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int s0 = start[c], s1 = start[c + 1];
    for (int t = tid; t < 512; t += 256) { kd[t] = GAL_INF_BITS; ki[t] = GAL_NO_PICK; }
    __syncthreads();
    for (int base = s0; base < s1; base += 256) {
        const bool valid = base + tid < s1;
        unsigned long long key = GAL_INF_BITS;
        int id = GAL_NO_PICK;
        if (valid) {
            id = sorted[base + tid];
            const int a = assign[id];
            if (a >= 0 && a < k_centroids) {
                const float* x = emb + (size_t)id * dim;
                const float* cc = centroids + (size_t)a * dim;
                double s = 0.0;
                for (int j = 0; j < dim; ++j) {
                    const double d = (double)x[j] - (double)cc[j];
                    s = s + d * d;
                }
                if (s == s) key = (unsigned long long)__double_as_longlong(s);
            }
        }
        const bool pass = valid && gal_key_less(key, id, kd[m - 1], ki[m - 1]);
        if (!__syncthreads_or(pass)) continue;             // (also: every thread has read the m-th best before it moves)
        kd[64 + tid] = pass ? key : GAL_INF_BITS;
        ki[64 + tid] = pass ? id : GAL_NO_PICK;
        if (tid < 192) { kd[320 + tid] = GAL_INF_BITS; ki[320 + tid] = GAL_NO_PICK; }
        __syncthreads();
        gal_sort512(kd, ki, tid);
    }
    if (tid < m) {
        const int id = ki[tid];
        idx_out[(size_t)c * m + tid] = id == GAL_NO_PICK ? -1 : id;
        d2_out[(size_t)c * m + tid] = id == GAL_NO_PICK ? (double)INFINITY : __longlong_as_double((long long)kd[tid]);
    }
}

// ---- the picture ---------------------------------------------------------------------------------------------------------------

struct GalLayout {
    int k, m, m_show, h, w, scale, cw, ch, row_h, x0, H, W;
};

GalLayout gal_layout(int k, int m, int m_show, int h, int w, int scale) {
    GalLayout L;
    L.k = k, L.m = m, L.m_show = m_show, L.h = h, L.w = w, L.scale = scale;
    L.cw = w * scale, L.ch = h * scale;
    L.row_h = L.ch > GAL_TEXT_H ? L.ch : GAL_TEXT_H;
    L.x0 = 2 * GAL_PAD + GAL_TEXT_W;
    L.H = GAL_PAD + k * (L.row_h + GAL_PAD);
    L.W = L.x0 + (2 + m_show) * (L.cw + GAL_PAD);
    return L;
}

// order[r] = the class of row r: descending count, ascending class among equal counts
__global__ __launch_bounds__(256) void gal_order_kernel(const int* __restrict__ count, int k, int* __restrict__ order) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    const int mine = count[c];
    int rank = 0;
    for (int o = 0; o < k; ++o) {                          // <= 4096 trips
        const int v = count[o];
        rank += v > mine || (v == mine && o < c);
    }
    order[rank] = c;
}

// block (cell, c): min and max of the patch cell `cell` of class c shows (0 the mean, 1 the deviation, 2 + e exemplar e); a cell
// without a patch gets (0, 0)
__global__ __launch_bounds__(256) void gal_cell_kernel(const float* __restrict__ mean, const float* __restrict__ std,
                                                       const int* __restrict__ idx, const float* __restrict__ patches, long long n,
                                                       int b, int m, int cells, float2* __restrict__ range) {
    __shared__ float red[8];
    const int cell = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const float* src = nullptr;
    if (cell == 0) src = mean + (size_t)c * b;
    else if (cell == 1) src = std + (size_t)c * b;
    else {
        const long long id = idx[(size_t)c * m + (cell - 2)];
        if (id >= 0 && id < n) src = patches + (size_t)id * b;
    }
    float mn = INFINITY, mx = -INFINITY;
    if (src)
        for (int i = tid; i < b; i += 256) {
            const float v = src[i];
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    mn = -wave_max(-mn);
    mx = wave_max(mx);
    if ((tid & 63) == 0) { red[tid >> 6] = mn; red[4 + (tid >> 6)] = mx; }
    __syncthreads();
    if (tid == 0) {
        mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
        mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        range[(size_t)c * cells + cell] = src ? make_float2(mn, mx) : make_float2(0.f, 0.f);
    }
}

// one workgroup: the largest deviation of all classes
__global__ __launch_bounds__(256) void gal_smax_kernel(const float2* __restrict__ range, int k, int cells, float* __restrict__ smax) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    float mx = 0.f;
    for (int c = tid; c < k; c += 256) mx = fmaxf(mx, range[(size_t)c * cells + 1].y);
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) *smax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// rne(fl(fl(fl(v - lo) / span) * 255)) held in 0..255; 0 where span is not positive or the value is a NaN
__device__ __forceinline__ unsigned char gal_byte(float v, float lo, float span) {
    if (!(span > 0.f)) return 0;
    const float t = rintf(__fmul_rn(__fdiv_rn(__fsub_rn(v, lo), span), 255.f));
    return t >= 255.f ? 255 : (t > 0.f ? (unsigned char)(int)t : 0);
}

__device__ __forceinline__ bool gal_digit_pixel(int value, int tx, int ty, const unsigned char* __restrict__ glyphs) {
    unsigned v = value > 0 ? (unsigned)value : 0u;
    int nd = 1;
    for (unsigned u = v; u >= 10u; u /= 10u) ++nd;
    const int d = tx / GAL_DIGIT_PITCH, gx = (tx - d * GAL_DIGIT_PITCH) / GAL_GLYPH_PX, gy = ty / GAL_GLYPH_PX;
    if (d >= nd || gx >= 5) return false;
    for (int s = nd - 1 - d; s > 0; --s) v /= 10u;
    return (glyphs[(v % 10u) * 7 + gy] >> (4 - gx)) & 1;                             // bit 4 of a row is its left pixel
}

__global__ __launch_bounds__(256) void gal_paint_kernel(const float* __restrict__ mean, const float* __restrict__ std,
                                                        const int* __restrict__ count, const int* __restrict__ idx,
                                                        const float* __restrict__ patches, long long n,
                                                        const unsigned char* __restrict__ glyphs, const int* __restrict__ order,
                                                        const float2* __restrict__ range, const float* __restrict__ smax,
                                                        GalLayout L, unsigned char* __restrict__ out) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)L.H * L.W) return;
    const int y = (int)(q / L.W), x = (int)(q - (long long)y * L.W);
    unsigned char g = 255;
    const int pitch_y = L.row_h + GAL_PAD, pitch_x = L.cw + GAL_PAD;
    const int r = (y - GAL_PAD) / pitch_y, ry = (y - GAL_PAD) - r * pitch_y;
    if (y >= GAL_PAD && r < L.k && ry < L.row_h) {
        const int c = order[r];
        const int b = L.h * L.w, cells = 2 + L.m_show;
        if (x >= GAL_PAD && x < GAL_PAD + GAL_TEXT_W) {
            const int tx = x - GAL_PAD;
            if (ry < GAL_LINE_H) g = gal_digit_pixel(c, tx, ry, glyphs) ? 0 : 255;
            else if (ry >= GAL_LINE_H + GAL_LINE_GAP && ry < GAL_TEXT_H)
                g = gal_digit_pixel(count[c], tx, ry - GAL_LINE_H - GAL_LINE_GAP, glyphs) ? 0 : 255;
        } else if (x >= L.x0) {
            const int cell = (x - L.x0) / pitch_x, cx = (x - L.x0) - cell * pitch_x;
            if (cell < cells && cx < L.cw && ry < L.ch) {
                const int p = (ry / L.scale) * L.w + cx / L.scale;
                const float2 mm = range[(size_t)c * cells + cell];
                if (cell == 0) g = gal_byte(mean[(size_t)c * b + p], mm.x, __fsub_rn(mm.y, mm.x));
                else if (cell == 1) g = gal_byte(std[(size_t)c * b + p], 0.f, *smax);
                else {
                    const long long id = idx[(size_t)c * L.m + (cell - 2)];
                    if (id >= 0 && id < n) g = gal_byte(patches[(size_t)id * b + p], mm.x, __fsub_rn(mm.y, mm.x));
                }
            }
        }
    }
    out[3 * q] = g; out[3 * q + 1] = g; out[3 * q + 2] = g;
}

// the counting sort shared by both reductions: after it W.cnt, W.start, W.chunk_start and W.sorted are set
int gal_bucket(const int32_t* labels, long n, int k, const GalWs& W, hipStream_t s) {
    MI_HIP(hipMemsetAsync(W.cnt, 0, sizeof(int) * ((size_t)k + 1), s));
    const int blocks = (int)std::min<long>(1024, (n + 4095) / 4096);
    const int per_block = (int)((n + blocks - 1) / blocks);
    hipLaunchKernelGGL(gal_hist_kernel, dim3(blocks), dim3(256), 0, s, (const int*)labels, (int)n, k, per_block, W.cnt);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(gal_scan_kernel, dim3(1), dim3(256), 0, s, (const int*)W.cnt, k, W.start, W.chunk_start);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(gal_scatter_kernel, dim3(k), dim3(GAL_SCATTER_THREADS), 0, s, (const int*)labels, (int)n,
                       (const int*)W.start, W.sorted);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

}  // namespace

extern "C" size_t mi_gallery_workspace_bytes(long n, int k_classes, int b, int m) {
    if (!gal_sizes_ok(n, k_classes, b, m)) return 0;
    return gal_carve(nullptr, n, k_classes, b).bytes;
}

extern "C" int mi_gallery_moments(const float* patches, const int32_t* labels, long n, int h, int w, int k_classes, float* mean_out,
                                  float* std_out, int32_t* count_out, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (h <= 0 || w <= 0 || (long long)h * w > GAL_MAX_PIXELS) return MI_E_ARG;
    const int b = h * w;
    if (!gal_sizes_ok(n, k_classes, b, 1)) return MI_E_ARG;
    if (!patches || !labels || !mean_out || !std_out || !count_out) return MI_E_ARG;
    if (!ws || ws_bytes < mi_gallery_workspace_bytes(n, k_classes, b, 1)) return MI_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const GalWs W = gal_carve(ws, n, k_classes, b);
    const int rc = gal_bucket(labels, n, k_classes, W, s);
    if (rc != MI_OK) return rc;
    const unsigned max_chunks = (unsigned)(n / GAL_CHUNK) + (unsigned)k_classes, tiles = (unsigned)mi_cdiv(b, 256);
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(gal_partial_kernel, dim3(max_chunks, tiles), dim3(256), 0, s, patches, (const int*)W.sorted,
                           (const int*)W.start, (const int*)W.chunk_start, k_classes, b, pass ? (const double*)W.mean_d : nullptr,
                           W.partial);
        MI_RETURN_IF_LAUNCH_FAILED();
        hipLaunchKernelGGL(gal_final_kernel, dim3(tiles, (unsigned)k_classes), dim3(256), 0, s, (const double*)W.partial,
                           (const int*)W.chunk_start, (const int*)W.cnt, b, pass, W.mean_d, pass ? std_out : mean_out,
                           (int*)count_out);
        MI_RETURN_IF_LAUNCH_FAILED();
    }
    return MI_OK;
}

extern "C" int mi_gallery_exemplars(const float* emb, const float* centroids, const int32_t* assign, const int32_t* labels, long n,
                                    int dim, int k_centroids, int k_classes, int m, int32_t* idx_out, double* d2_out, void* ws,
                                    size_t ws_bytes, mi_stream_t stream) {
    if (m < 1 || m > GAL_MAX_M) return MI_E_ARG;             // before anything is enqueued
    if (!gal_sizes_ok(n, k_classes, 0, m) || dim <= 0 || dim > 65536 || k_centroids <= 0) return MI_E_ARG;
    if (!emb || !centroids || !assign || !labels || !idx_out || !d2_out) return MI_E_ARG;
    if (!ws || ws_bytes < mi_gallery_workspace_bytes(n, k_classes, 0, m)) return MI_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const GalWs W = gal_carve(ws, n, k_classes, 0);
    const int rc = gal_bucket(labels, n, k_classes, W, s);
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(gal_exemplar_kernel, dim3(k_classes), dim3(256), 0, s, emb, centroids, (const int*)assign,
                       (const int*)W.sorted, (const int*)W.start, dim, k_centroids, m, (int*)idx_out, d2_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" size_t mi_gallery_raster_workspace_bytes(int k_classes, int m_show) {
    if (k_classes <= 0 || k_classes > GAL_MAX_K || m_show < 0 || m_show > GAL_MAX_M) return 0;
    return 256 + mi_align_up(sizeof(float2) * (size_t)k_classes * (size_t)(2 + m_show), 256);
}

extern "C" int mi_gallery_raster(const float* mean, const float* std, const int32_t* count, const int32_t* idx, const float* patches,
                                 long n, int h, int w, int k_classes, int m, int m_show, int scale, const uint8_t* glyphs,
                                 int32_t* order_out, uint8_t* out_rgb, int H, int W, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (h <= 0 || w <= 0 || (long long)h * w > GAL_MAX_PIXELS || scale < 1 || scale > 64) return MI_E_ARG;
    if (!gal_sizes_ok(n, k_classes, h * w, m) || m_show < 0 || m_show > m) return MI_E_ARG;
    if (!mean || !std || !count || !idx || !patches || !glyphs || !order_out || !out_rgb) return MI_E_ARG;
    if ((long long)w * scale > 65536 || (long long)h * scale > 65536) return MI_E_ARG;
    const GalLayout L = gal_layout(k_classes, m, m_show, h, w, scale);
    if (H != L.H || W != L.W) return MI_E_ARG;               // the caller's canvas is the one this layout paints
    if ((long long)L.H * L.W > 0x3fffffffLL) return MI_E_UNSUPPORTED;
    if (!ws || ws_bytes < mi_gallery_raster_workspace_bytes(k_classes, m_show)) return MI_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    float* smax = (float*)ws;
    float2* range = (float2*)((unsigned char*)ws + 256);
    const int cells = 2 + m_show;
    hipLaunchKernelGGL(gal_order_kernel, dim3((unsigned)mi_cdiv(k_classes, 256)), dim3(256), 0, s, (const int*)count, k_classes,
                       (int*)order_out);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(gal_cell_kernel, dim3((unsigned)cells, (unsigned)k_classes), dim3(256), 0, s, mean, std, (const int*)idx,
                       patches, (long long)n, h * w, m, cells, range);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(gal_smax_kernel, dim3(1), dim3(256), 0, s, (const float2*)range, k_classes, cells, smax);
    MI_RETURN_IF_LAUNCH_FAILED();
    const long long pixels = (long long)L.H * L.W;
    hipLaunchKernelGGL(gal_paint_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, mean, std, (const int*)count,
                       (const int*)idx, patches, (long long)n, glyphs, (const int*)order_out, (const float2*)range,
                       (const float*)smax, L, out_rgb);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

// The pictures of the exploration map and the thumbnails of the picks (the reference's plot_2d.py:96-103 and :121-218), DESIGN.md 4.18:
//   mi_plot_select       which picks get a thumbnail: the reference's greedy filter in input order (:123-137), exactly
//   mi_plot_thumbs       z-score of a whole patch, quantize(-3, 3) to a byte, channel 0 resized to T x T (:145-151)
//   mi_plot_patch_bytes  plt.imsave(patch[0], cmap='gray') of every pick: min-max, colour-table index, table byte (:103)
//   mi_plot_raster       discs, framed thumbnails and class boxes painted in matplotlib's draw order onto a white canvas
//
// Selection.  Pick i is shown unless a pick shown before it lies at a float32 squared distance below thr.  The order
// dependence is kept, the search over all shown picks is not: shown picks sit in a uniform grid over the unit square, one
// linked list per cell (head[cell], next[pick]: no slot count to overflow), and a candidate meets only the 3 x 3 cells around
// its own.  The cell side is at least 1.001 sqrt(thr): fl(fl(dx dx) + fl(dy dy)) < thr bounds |x_i - x_j| by
// sqrt(thr) (1 + 2^-21), so the exact products x G of a blocking pair differ by less than 1 and their floors by at most 1
// (the product of a float and G <= 1024 is exact in double; clamping the cell to the grid is monotone and keeps that).
// One wave walks the picks 64 at a time: every lane tests its candidate against the grid (whoever is blocked there stays
// blocked, the lists only grow), then the survivors are settled among themselves in index order with ballots - the lowest
// surviving lane is shown, is inserted, and strikes the later lanes it blocks - and the next 64 follow.  No list or round is
// capped; a walk longer than the number of picks (a corrupted list) ends the kernel with count = -1 instead of spinning.
//
// Raster.  "Later over earlier" without ordered launches, as mi_vis_paint has it: every primitive writes its draw-order number
// into an int32 priority image with an atomic max, then every pixel looks its winner up and takes the colour that primitive
// has there.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SELECT_MAX_GRID = 1024;                     // cells per side at most (4 MB of heads)
constexpr long SELECT_MAX_N = 1L << 24;
constexpr int THUMB_MAX_SIDE = 192;                       // channel 0 of a patch as bytes in LDS: 36 KB

// cells per side: 0 when thr does not block anything (thr <= 0 or NaN)
int select_grid(long n, float thr) {
    if (!(thr > 0.0f)) return 0;
    const double side = 1.001 * sqrt((double)thr);
    long g = side >= 1.0 ? 1 : (long)floor(1.0 / side);
    g = std::min<long>(g, SELECT_MAX_GRID);
    g = std::min<long>(g, std::max<long>(1, (long)sqrt((double)n)));          // no more cells than picks
    return (int)std::max<long>(g, 1);
}

__device__ __forceinline__ int cell_of(float v, int G) {
    const double t = floor((double)v * (double)G);
    return t >= (double)(G - 1) ? G - 1 : (t > 0.0 ? (int)t : 0);               // (a NaN goes to 0)
}

__device__ __forceinline__ float dist2(float xi, float yi, float xj, float yj) {
    const float dx = __fsub_rn(xi, xj), dy = __fsub_rn(yi, yj);
    return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}

__device__ __forceinline__ int list_load(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void list_store(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(64) void plot_select_all_kernel(int n, int* __restrict__ shown, int* __restrict__ count) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) shown[i] = i;
    if (i == 0) *count = n;
}

// one wave; head[G G] holds -1 on entry
__global__ __launch_bounds__(64) void plot_select_kernel(const float* __restrict__ y01, int n, float thr, int G, int* head,
                                                         int* next, int* __restrict__ shown, int* __restrict__ count) {
    const int lane = threadIdx.x;
    const float2* pts = reinterpret_cast<const float2*>(y01);
    if (lane == 0) {                                       // shown starts as [y01[0]]: it blocks, and is not emitted here
        const float2 p = pts[0];
        list_store(next, -1);
        list_store(head + cell_of(p.y, G) * G + cell_of(p.x, G), 0);
    }
    __threadfence_block();
    __syncthreads();
    int cnt = 0;
    bool broken = false;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool valid = i < n;
        float2 p = make_float2(0.f, 0.f);
        int cx = 0, cy = 0;
        bool alive = valid;
        if (valid) {
            p = pts[i];
            cx = cell_of(p.x, G);
            cy = cell_of(p.y, G);
            int cur[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const int gx = cx + c % 3 - 1, gy = cy + c / 3 - 1;
                cur[c] = gx >= 0 && gx < G && gy >= 0 && gy < G ? list_load(head + gy * G + gx) : -1;
            }
            int hops = 0;
            bool more = true;
            while (more && alive) {
                more = false;
#pragma unroll
                for (int c = 0; c < 9; ++c) {
                    const int j = cur[c];
                    if (j >= 0 && j < n) {
                        const float2 q = pts[j];
                        cur[c] = list_load(next + j);
                        if (dist2(p.x, p.y, q.x, q.y) < thr) alive = false;
                        more = true;
                    } else {
                        cur[c] = -1;
                    }
                }
                if (++hops > n) { broken = true; break; }
            }
        }
        // the survivors among themselves, in index order
        unsigned long long m = __ballot(alive);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            const float sx = __shfl(p.x, l, 64), sy = __shfl(p.y, l, 64);
            if (lane == l) {
                int* h = head + cy * G + cx;
                list_store(next + i, list_load(h));
                list_store(h, i);
                shown[cnt] = i;
                alive = false;
            } else if (alive && dist2(p.x, p.y, sx, sy) < thr) {
                alive = false;
            }
            ++cnt;
            m = __ballot(alive);
        }
        __threadfence_block();
        __syncthreads();
        if (__any(broken)) break;
    }
    if (lane == 0) *count = __any(broken) ? -1 : cnt;
}

// the sum of v over the 256 threads of a block, on every thread; red: 4 doubles of LDS
__device__ __forceinline__ double block_sum256(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

// one block per shown pick; dynamic LDS: 8 doubles, then b b bytes
__global__ __launch_bounds__(256) void plot_thumbs_kernel(const float* __restrict__ patches, long long N,
                                                          const int* __restrict__ idx, int C, int b, int T,
                                                          unsigned char* __restrict__ out, unsigned char* __restrict__ pre) {
    extern __shared__ double smem[];
    double* red = smem;
    unsigned char* img = reinterpret_cast<unsigned char*>(smem + 8);
    const long long k = blockIdx.x;
    const long long id = idx[k];
    const int bb = b * b, E = C * bb, tid = threadIdx.x;
    const bool ok = id >= 0 && id < N;
    const float* x = patches + (ok ? id : 0) * (long long)E;
    double s = 0.0;
    for (int i = tid; i < E; i += 256) s += (double)x[i];
    const double mean = block_sum256(s, red) / (double)E;
    double v = 0.0;
    for (int i = tid; i < E; i += 256) {
        const double d = (double)x[i] - mean;
        v += d * d;
    }
    const double std = sqrt(block_sum256(v, red) / (double)E);
    const bool flat = !ok || !(std > 0.0);
    for (int i = tid; i < E; i += 256) {
        double t = ((double)x[i] - mean) / std;
        t = 255.0 * (t + 3.0) / 6.0;
        t = t < 0.0 ? 0.0 : (t > 255.0 ? 255.0 : t);
        const unsigned char q = flat || t != t ? (unsigned char)0 : (unsigned char)(int)rint(t);
        if (pre) pre[k * E + i] = q;
        if (i < bb) img[i] = q;
    }
    __syncthreads();
    // torch's upsample_bilinear2d, align_corners = False, in float32; torchvision rounds the result to a byte
    const float scale = (float)b / (float)T;
    for (int p = tid; p < T * T; p += 256) {
        const int oy = p / T, ox = p - oy * T;
        float sy = scale * ((float)oy + 0.5f) - 0.5f, sx = scale * ((float)ox + 0.5f) - 0.5f;
        sy = sy < 0.f ? 0.f : sy;
        sx = sx < 0.f ? 0.f : sx;
        const int y0 = min((int)sy, b - 1), x0 = min((int)sx, b - 1);
        const int y1 = min(y0 + 1, b - 1), x1 = min(x0 + 1, b - 1);
        const float ly = sy - (float)y0, lx = sx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
        const float top = hx * (float)img[y0 * b + x0] + lx * (float)img[y0 * b + x1];
        const float bot = hx * (float)img[y1 * b + x0] + lx * (float)img[y1 * b + x1];
        float r = rintf(hy * top + ly * bot);
        r = r < 0.f ? 0.f : (r > 255.f ? 255.f : r);
        out[k * T * T + p] = (unsigned char)(int)r;
    }
}

// one block per pick: Normalize(min, max) of channel 0 in float32, index floor(256 t) capped at 255, the table's byte
__global__ __launch_bounds__(256) void plot_patch_bytes_kernel(const float* __restrict__ patches, long long stride, int bb,
                                                               const unsigned char* __restrict__ lut,
                                                               unsigned char* __restrict__ out) {
    __shared__ float red[8];
    const long long k = blockIdx.x;
    const float* x = patches + k * stride;
    const int tid = threadIdx.x;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = tid; i < bb; i += 256) {
        const float v = x[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    mn = -wave_max(-mn);
    mx = wave_max(mx);
    if ((tid & 63) == 0) { red[tid >> 6] = mn; red[4 + (tid >> 6)] = mx; }
    __syncthreads();
    mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    const float range = __fsub_rn(mx, mn);
    const bool flat = !(range > 0.f);
    for (int i = tid; i < bb; i += 256) {
        int idx = 0;
        if (!flat) {
            const float t = __fmul_rn(__fdiv_rn(__fsub_rn(x[i], mn), range), 256.f);
            idx = t >= 255.f ? 255 : (t > 0.f ? (int)t : 0);
        }
        out[k * bb + i] = lut[idx];
    }
}

struct Centre { int col, row; };

// the pixel of a map point: column M + rne(u S), row M + rne((1 - v) S), in double; v points up
__device__ __forceinline__ Centre centre_of(const float* __restrict__ y01, long long id, const mi_plot_layout& L) {
    const double S = (double)(L.P - 1 - 2 * L.M);
    double c = rint((double)y01[2 * id] * S), r = rint((1.0 - (double)y01[2 * id + 1]) * S);
    const double far = 1.0e9;                              // (a point that far out draws nothing; a NaN goes there too)
    c = c >= -far && c <= far ? c : far;
    r = r >= -far && r <= far ? r : far;
    Centre o;
    o.col = L.M + (int)c;
    o.row = L.M + (int)r;
    return o;
}

__device__ __forceinline__ int digits_of(int label) {
    unsigned v = label > 0 ? (unsigned)label : 0u;
    int nd = 1;
    while (v >= 10u) { v /= 10u; ++nd; }
    return nd;
}

__device__ __forceinline__ int box_width(int nd, const mi_plot_layout& L) {
    return nd * 5 * L.glyph_px + (nd - 1) * L.glyph_gap + 2 * (L.box_pad + L.box_border);
}
__device__ __forceinline__ int box_height(const mi_plot_layout& L) { return 7 * L.glyph_px + 2 * (L.box_pad + L.box_border); }

// primitive number -> (kind: 0 disc, 1 framed thumbnail, 2 class box; shown pick).  mode 0 ("out"): discs 0..n-1, then
// thumbnails n..2n-1.  mode 1 ("labels"): thumbnail k at 2k, box k at 2k + 1.
__device__ __forceinline__ void prim_of(long long q, long long n, int mode, int& kind, long long& k) {
    if (mode == 0) { kind = q < n ? 0 : 1; k = q < n ? q : q - n; }
    else { kind = 1 + (int)(q & 1); k = q >> 1; }
}

// blocks_per_prim blocks per primitive, each thread a pixel of the primitive's bounding box
__global__ __launch_bounds__(256) void plot_raster_index_kernel(const float* __restrict__ y01, const int* __restrict__ idx,
                                                                long long n, long long N, const int* __restrict__ labels,
                                                                mi_plot_layout L, int mode, int blocks_per_prim,
                                                                int* __restrict__ prio) {
    const long long q = blockIdx.x / blocks_per_prim;
    if (q >= 2 * n) return;
    int kind;
    long long k;
    prim_of(q, n, mode, kind, k);
    const long long id = idx[k];
    if (id < 0 || id >= N) return;
    const Centre c = centre_of(y01, id, L);
    int x0, y0, w, h;
    if (kind == 0) { x0 = c.col - L.R; y0 = c.row - L.R; w = h = 2 * L.R + 1; }
    else if (kind == 1) { x0 = c.col - L.T / 2 - 1; y0 = c.row - L.T / 2 - 1; w = h = L.T + 2; }
    else {
        w = box_width(digits_of(labels[id]), L);
        h = box_height(L);
        x0 = c.col - L.label_dx;
        y0 = c.row - L.label_dy - h + 1;
    }
    const int t = (blockIdx.x % blocks_per_prim) * 256 + threadIdx.x;
    if (t >= w * h) return;
    const int dy = t / w, dx = t - dy * w;
    const long long col = (long long)x0 + dx, row = (long long)y0 + dy;
    if (col < 0 || col >= L.P || row < 0 || row >= L.P) return;
    if (kind == 0) {
        const int ex = dx - L.R, ey = dy - L.R;
        if (ex * ex + ey * ey > L.R * L.R) return;
    }
    atomicMax(prio + row * L.P + col, (int)(q + 1));
}

__global__ __launch_bounds__(256) void plot_raster_colour_kernel(const int* __restrict__ prio, const float* __restrict__ y01,
                                                                 const int* __restrict__ idx, long long n, long long N,
                                                                 const unsigned char* __restrict__ thumbs,
                                                                 const unsigned char* __restrict__ colours,
                                                                 const int* __restrict__ labels,
                                                                 const unsigned char* __restrict__ glyphs, mi_plot_layout L,
                                                                 int mode, unsigned char* __restrict__ out) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)L.P * L.P) return;
    const int row = (int)(p / L.P), col = (int)(p - (long long)row * L.P);
    unsigned char r = 255, g = 255, b = 255;
    const long long w = prio[p];
    if (w > 0 && w <= 2 * n) {
        int kind;
        long long k;
        prim_of(w - 1, n, mode, kind, k);
        const long long id = idx[k];
        const Centre c = centre_of(y01, id, L);
        if (kind == 0) {
            r = colours[3 * id]; g = colours[3 * id + 1]; b = colours[3 * id + 2];
        } else if (kind == 1) {
            const int tx = col - (c.col - L.T / 2), ty = row - (c.row - L.T / 2);
            r = g = b = tx >= 0 && tx < L.T && ty >= 0 && ty < L.T ? thumbs[(k * L.T + ty) * L.T + tx] : (unsigned char)0;
        } else {
            const int label = labels[id];
            const int nd = digits_of(label), bw = box_width(nd, L), bh = box_height(L);
            const int bx = col - (c.col - L.label_dx), by = row - (c.row - L.label_dy - bh + 1);
            bool blue = bx < L.box_border || by < L.box_border || bx >= bw - L.box_border || by >= bh - L.box_border;
            const int tx = bx - L.box_border - L.box_pad, ty = by - L.box_border - L.box_pad;
            const int pitch = 5 * L.glyph_px + L.glyph_gap;
            if (!blue && tx >= 0 && ty >= 0 && ty < 7 * L.glyph_px && tx < nd * pitch - L.glyph_gap) {
                const int d = tx / pitch, gx = (tx - d * pitch) / L.glyph_px, gy = ty / L.glyph_px;
                if (gx < 5) {
                    unsigned v = label > 0 ? (unsigned)label : 0u;
                    for (int s = nd - 1 - d; s > 0; --s) v /= 10u;
                    blue = (glyphs[(v % 10u) * 7 + gy] >> (4 - gx)) & 1;        // bit 4 of a row is its left pixel
                }
            }
            r = g = blue ? 0 : 255;
            b = 255;
        }
    }
    out[3 * p] = r; out[3 * p + 1] = g; out[3 * p + 2] = b;
}

bool layout_ok(const mi_plot_layout& L) {
    return L.P >= 8 && L.P <= 16384 && L.M >= 0 && 2 * L.M < L.P - 1 && L.R >= 0 && L.R <= 4096 && L.T >= 1 && L.T <= 1024 &&
           L.label_dx >= -65536 && L.label_dx <= 65536 && L.label_dy >= -65536 && L.label_dy <= 65536 && L.glyph_px >= 1 &&
           L.glyph_px <= 16 && L.glyph_gap >= 0 && L.glyph_gap <= 64 && L.box_pad >= 0 && L.box_pad <= 64 && L.box_border >= 0 &&
           L.box_border <= 64;
}

}  // namespace

extern "C" size_t mi_plot_select_workspace_bytes(long n, float thr) {
    if (n <= 0 || n > SELECT_MAX_N) return 0;
    const size_t g = (size_t)select_grid(n, thr);
    return mi_align_up(sizeof(int32_t) * (g * g + (size_t)n), 16);
}

extern "C" int mi_plot_select(const float* y01, long n, float thr, int32_t* shown_idx, int32_t* count, void* ws, size_t ws_bytes,
                              mi_stream_t stream) {
    if (!count || n < 0 || (n > 0 && (!y01 || !shown_idx))) return MI_E_ARG;
    if (n > SELECT_MAX_N) return MI_E_UNSUPPORTED;
    const hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        MI_HIP(hipMemsetAsync(count, 0, sizeof(int32_t), s));
        return MI_OK;
    }
    const int G = select_grid(n, thr);
    if (G == 0) {
        hipLaunchKernelGGL(plot_select_all_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (int)n, (int*)shown_idx,
                           (int*)count);
        MI_RETURN_IF_LAUNCH_FAILED();
        return MI_OK;
    }
    if (!ws || ws_bytes < mi_plot_select_workspace_bytes(n, thr)) return MI_E_WORKSPACE;
    int* head = (int*)ws;
    int* next = head + (size_t)G * G;
    MI_HIP(hipMemsetAsync(head, 0xff, sizeof(int) * (size_t)G * G, s));
    hipLaunchKernelGGL(plot_select_kernel, dim3(1), dim3(64), 0, s, y01, (int)n, thr, G, head, next, (int*)shown_idx, (int*)count);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_plot_thumbs(const float* patches, long N, int C, int b, const int32_t* idx, long n_shown, int T, uint8_t* out,
                              uint8_t* pre, mi_stream_t stream) {
    if (n_shown == 0) return MI_OK;
    if (!patches || !idx || !out || N <= 0 || n_shown < 0 || C <= 0 || b <= 0 || T <= 0) return MI_E_ARG;
    if (b > THUMB_MAX_SIDE || T > 1024 || (long long)C * b * b > 0x7fffffffLL || n_shown > 0x7fffffffL) return MI_E_UNSUPPORTED;
    const size_t lds = 8 * sizeof(double) + (size_t)b * b;
    hipLaunchKernelGGL(plot_thumbs_kernel, dim3((unsigned)n_shown), dim3(256), lds, (hipStream_t)stream, patches, (long long)N,
                       (const int*)idx, C, b, T, out, pre);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_plot_patch_bytes(const float* patches, long N, int C, int b, const uint8_t* lut256, uint8_t* out,
                                   mi_stream_t stream) {
    if (N == 0) return MI_OK;
    if (!patches || !lut256 || !out || N < 0 || C <= 0 || b <= 0) return MI_E_ARG;
    if ((long long)C * b * b > 0x7fffffffLL || N > 0x7fffffffL) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(plot_patch_bytes_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, patches,
                       (long long)C * b * b, b * b, lut256, out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" size_t mi_plot_raster_workspace_bytes(int P) {
    return P > 0 && P <= 16384 ? sizeof(int32_t) * (size_t)P * (size_t)P : 0;
}

extern "C" int mi_plot_raster(const float* y01, long N, const int32_t* idx, long n_shown, const uint8_t* thumbs,
                              const uint8_t* colours, const int32_t* labels, const uint8_t* glyphs, const mi_plot_layout* layout,
                              int mode, uint8_t* out, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (!layout || !out || N < 0 || n_shown < 0 || (mode != 0 && mode != 1)) return MI_E_ARG;
    const mi_plot_layout L = *layout;
    if (!layout_ok(L)) return MI_E_ARG;
    if (n_shown > 0 && (!y01 || !idx || !thumbs || N == 0 || (mode == 0 ? !colours : (!labels || !glyphs)))) return MI_E_ARG;
    if (!ws || ws_bytes < mi_plot_raster_workspace_bytes(L.P)) return MI_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const long long disc = (long long)(2 * L.R + 1) * (2 * L.R + 1), thumb = (long long)(L.T + 2) * (L.T + 2);
    const long long box = (long long)(10 * 5 * L.glyph_px + 9 * L.glyph_gap + 2 * (L.box_pad + L.box_border)) *
                          (7 * L.glyph_px + 2 * (L.box_pad + L.box_border));      // ten digits: any int32
    const long long per = std::max(thumb, mode == 0 ? disc : box);
    const long long bpp = (per + 255) / 256;
    if (2 * (long long)n_shown * bpp > 0x7fffffffLL) return MI_E_UNSUPPORTED;
    MI_HIP(hipMemsetAsync(ws, 0, sizeof(int32_t) * (size_t)L.P * (size_t)L.P, s));
    if (n_shown > 0) {
        hipLaunchKernelGGL(plot_raster_index_kernel, dim3((unsigned)(2 * n_shown * bpp)), dim3(256), 0, s, y01, (const int*)idx,
                           (long long)n_shown, (long long)N, (const int*)labels, L, mode, (int)bpp, (int*)ws);
        MI_RETURN_IF_LAUNCH_FAILED();
    }
    const long long pixels = (long long)L.P * L.P;
    hipLaunchKernelGGL(plot_raster_colour_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, (const int*)ws, y01,
                       (const int*)idx, (long long)n_shown, (long long)N, thumbs, colours, (const int*)labels, glyphs, L, mode, out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

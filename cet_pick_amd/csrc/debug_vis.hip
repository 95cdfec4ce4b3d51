// The slice pictures that the detector's validation leaves under --debug 4 (the reference's trains/tomo_cr_semi_trainer.py:123-186
// with utils/debugger.py, there cv2 on the host, slice by slice), DESIGN.md 4.19:
//   mi_dbgvis_minmax   min and max of every slice of a slab (cv2.normalize NORM_MINMAX needs them)
//   mi_dbgvis_render   the four pictures pred_hm, gt_hm, pred_out, gt_out of every slice of a slab, one launch
//
// Every output pixel is computed by the thread that owns it, as a gather: the grey byte from the tomogram, the two heat-maps
// enlarged 2 x from their four nearest source pixels, and "is this pixel on a ring" as a test of the pixel against the centres
// of its own slice.  Nothing is scattered, so there is no atomic and no write order to depend on; overlapping rings and rings
// cut by the border need no case of their own.
//
// Rings.  The pixel set of the midpoint circle algorithm is made once per call on the host as a bitmask, row dy + r holding
// bit dx + r (r <= 31: one 64-bit word per row), and sits in LDS.  The centres are sorted by slice on the host (CSR: a
// workgroup reads only the list of its slice; the list bounds are wave-uniform, so the centres arrive through scalar loads).
// The index travels in the workspace: [nz + 1] pred_ptr, [nz + 1] gt_ptr, [64] mask rows (64-bit), then (x, y) int32 pairs.
//
// Arithmetic.  No FMA: `t * 255` after `(v - mn) * s` is two roundings in the statement this file restates, so contraction is
// off for the whole file.  The blend of gt_hm runs in float64 as numpy runs it.
// A thread takes 4 consecutive pixels of a row (one float4 of the tomogram, three 32-bit words per picture) when W is a
// multiple of 4 and the buffers are aligned, 2 pixels with byte stores otherwise (W is even: W == 2 w).
#include "common.h"

#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int DBG_MAX_RADIUS = 31, DBG_MASK_ROWS = 64;
constexpr int MINMAX_THREADS = 1024;

__global__ __launch_bounds__(MINMAX_THREADS) void dbgvis_minmax_kernel(const float* __restrict__ vol, long long HW, int z0,
                                                                       float* __restrict__ out) {
    const float* s = vol + (long long)(z0 + (int)blockIdx.x) * HW;
    const int tid = threadIdx.x;
    long long head = (long long)(((16 - ((uintptr_t)s & 15)) & 15) >> 2);     // elements in front of the first 16-byte line
    if (head > HW) head = HW;
    const long long nvec = (HW - head) / 4;
    float mn = INFINITY, mx = -INFINITY;
    for (long long i = tid; i < head; i += MINMAX_THREADS) { mn = fminf(mn, s[i]); mx = fmaxf(mx, s[i]); }
    const float4* v = reinterpret_cast<const float4*>(s + head);
    for (long long i = tid; i < nvec; i += MINMAX_THREADS) {
        const float4 q = v[i];
        mn = fminf(fminf(mn, q.x), fminf(q.y, fminf(q.z, q.w)));
        mx = fmaxf(fmaxf(mx, q.x), fmaxf(q.y, fmaxf(q.z, q.w)));
    }
    for (long long i = head + 4 * nvec + tid; i < HW; i += MINMAX_THREADS) { mn = fminf(mn, s[i]); mx = fmaxf(mx, s[i]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    __shared__ float red[2 * MINMAX_THREADS / 64];
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = mn; red[2 * (tid >> 6) + 1] = mx; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < MINMAX_THREADS / 64; ++k) { mn = fminf(mn, red[2 * k]); mx = fmaxf(mx, red[2 * k + 1]); }
        out[2 * blockIdx.x] = mn;
        out[2 * blockIdx.x + 1] = mx;
    }
}

// trunc(min(max(255 v, 0), 255)) in float32 (a NaN goes to 0)
__device__ __forceinline__ int byte_of_unit(float v) { return (int)fminf(fmaxf(v * 255.0f, 0.0f), 255.0f); }

template <int V>
__global__ __launch_bounds__(256) void dbgvis_render_kernel(const float* __restrict__ tomo, const float* __restrict__ hm_pred,
                                                            const float* __restrict__ hm_gt, int H, int W, int h, int w, int z0,
                                                            int nz, const float* __restrict__ minmax,
                                                            const int* __restrict__ index, int radius, long long units,
                                                            unsigned char* __restrict__ out) {
    constexpr int NC = V / 2 + 2;                          // source columns under V output pixels and their outer neighbours
    __shared__ unsigned long long mask[DBG_MASK_ROWS];
    const int tid = threadIdx.x, i = blockIdx.y, z = z0 + i;
    const int* pred_ptr = index;
    const int* gt_ptr = index + (nz + 1);
    const unsigned long long* gmask = reinterpret_cast<const unsigned long long*>(index + 2 * (nz + 1));
    const int* cen = index + 2 * (nz + 1) + 2 * DBG_MASK_ROWS;
    if (tid < DBG_MASK_ROWS) mask[tid] = gmask[tid];
    __syncthreads();
    const long long u = (long long)blockIdx.x * 256 + tid;
    if (u >= units) return;
    const long long HW = (long long)H * W, hw = (long long)h * w;
    const long long p = u * V;                             // first pixel of the unit inside its slice; a unit stays in one row
    const int y = (int)(p / W), x = (int)(p % W);

    // grey
    const float mn = minmax[2 * i], mx = minmax[2 * i + 1];
    const float d = mx - mn;
    const float s = d == 0.0f ? 0.0f : __fdiv_rn(1.0f, d);
    const float* trow = tomo + (long long)z * HW + p;
    float tv[V];
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(trow);
        tv[0] = q.x; tv[1] = q.y; tv[2] = q.z; tv[3] = q.w;
    } else {
#pragma unroll
        for (int m = 0; m < V; ++m) tv[m] = trow[m];
    }
    int g[V];
#pragma unroll
    for (int m = 0; m < V; ++m) {
        const float t = (tv[m] - mn) * s;
        g[m] = byte_of_unit(t);
    }

    // the two heat-maps, 2 x
    const int sy = y >> 1, ny = (y & 1) ? min(sy + 1, h - 1) : max(sy - 1, 0);
    const int sx0 = x >> 1;
    int col[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) col[j] = min(max(sx0 - 1 + j, 0), w - 1);
    int up[2][V];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float* mz = (k == 0 ? hm_pred : hm_gt) + (long long)z * hw;
        const float* r0 = mz + (long long)sy * w;
        const float* r1 = mz + (long long)ny * w;
        int a0[NC], a1[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) { a0[j] = byte_of_unit(r0[col[j]]); a1[j] = byte_of_unit(r1[col[j]]); }
#pragma unroll
        for (int m = 0; m < V; ++m) {
            const int js = 1 + (m >> 1), jn = (m & 1) ? js + 1 : js - 1;        // x is even: pixel m is odd when m is
            up[k][m] = (9 * a0[js] + 3 * a0[jn] + 3 * a1[js] + a1[jn] + 8) >> 4;
        }
    }

    // rings: bit m of hit[k] says that pixel m lies on a ring of list k (0 the picks, 1 the ground truth)
    unsigned hit[2] = {0u, 0u};
    const unsigned span = 2u * (unsigned)radius;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int* ptr = k == 0 ? pred_ptr : gt_ptr;
        const int beg = ptr[i], end = ptr[i + 1];
        for (int c = beg; c < end; ++c) {
            const int cx = cen[2 * c], cy = cen[2 * c + 1];
            const unsigned dy = (unsigned)(y - cy + radius);
            if (dy > span) continue;
            const unsigned long long row = mask[dy];
#pragma unroll
            for (int m = 0; m < V; ++m) {
                const unsigned dx = (unsigned)(x + m - cx + radius);
                if (dx <= span && ((row >> dx) & 1ull)) hit[k] |= 1u << m;
            }
        }
    }

    unsigned rgb[4][V];
#pragma unroll
    for (int m = 0; m < V; ++m) {
        const unsigned grey = (unsigned)g[m] * 0x010101u;
        double b = (double)g[m] * (1.0 - 0.7) + (double)up[1][m] * 0.7;
        b = b < 0.0 ? 0.0 : (b > 255.0 ? 255.0 : b);
        rgb[0][m] = (unsigned)up[0][m] * 0x010101u;
        rgb[1][m] = (unsigned)(int)b * 0x010101u;
        rgb[2][m] = (hit[0] >> m) & 1u ? 0xff0000u : grey;                      // R | G << 8 | B << 16: (0, 0, 255)
        rgb[3][m] = (hit[1] >> m) & 1u ? 0xff0000u : grey;
    }
    const long long pic = (long long)nz * HW * 3;
    unsigned char* o = out + ((long long)i * HW + p) * 3;
#pragma unroll
    for (int k = 0; k < 4; ++k, o += pic) {
        if constexpr (V == 4) {
            unsigned* ow = reinterpret_cast<unsigned*>(o);                      // 12 bytes from a multiple of 12
            ow[0] = rgb[k][0] | (rgb[k][1] << 24);
            ow[1] = (rgb[k][1] >> 8) | (rgb[k][2] << 16);
            ow[2] = (rgb[k][2] >> 16) | (rgb[k][3] << 8);
        } else {
#pragma unroll
            for (int m = 0; m < V; ++m) {
                o[3 * m] = (unsigned char)rgb[k][m];
                o[3 * m + 1] = (unsigned char)(rgb[k][m] >> 8);
                o[3 * m + 2] = (unsigned char)(rgb[k][m] >> 16);
            }
        }
    }
}

// the midpoint circle algorithm: row dy + r of the mask holds bit dx + r
void ring_mask(int r, unsigned long long* rows) {
    for (int k = 0; k < DBG_MASK_ROWS; ++k) rows[k] = 0;
    auto plot = [&](int dx, int dy) { rows[dy + r] |= 1ull << (dx + r); };
    int x = r, y = 0, err = 1 - r;
    while (x >= y) {
        plot(x, y); plot(y, x); plot(-x, y); plot(-y, x); plot(x, -y); plot(y, -x); plot(-x, -y); plot(-y, -x);
        ++y;
        if (err < 0) {
            err += 2 * y + 1;
        } else {
            --x;
            err += 2 * (y - x) + 1;
        }
    }
}

// slice index (0..nz-1) of a row [x, y, z, ...] whose ring can touch the slab's pictures, -1 otherwise; (int) truncates as
// Python's int() does
int slab_slice(const float* r, int H, int W, int z0, int nz) {
    const float x = r[0], y = r[1], z = r[2];
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) return -1;
    const float reach = (float)(DBG_MAX_RADIUS + 2);
    if (!(x > -reach && x < (float)W + reach && y > -reach && y < (float)H + reach)) return -1;
    if (!(z > -1.0f && z < (float)z0 + (float)nz)) return -1;
    const int zi = (int)z;
    return zi >= z0 && zi < z0 + nz ? zi - z0 : -1;
}

size_t index_words(int nz, long n_pred, long n_gt) {
    return 2 * ((size_t)nz + 1) + 2 * DBG_MASK_ROWS + 2 * ((size_t)n_pred + (size_t)n_gt);
}

}  // namespace

extern "C" int mi_dbgvis_minmax(const float* vol, int D, int H, int W, int z0, int nz, float* out_minmax, mi_stream_t stream) {
    if (!vol || !out_minmax || D <= 0 || H <= 0 || W <= 0 || z0 < 0 || nz <= 0 || (long long)z0 + nz > D || nz > 65535 ||
        ((uintptr_t)vol & 3))
        return MI_E_ARG;
    hipLaunchKernelGGL(dbgvis_minmax_kernel, dim3((unsigned)nz), dim3(MINMAX_THREADS), 0, (hipStream_t)stream, vol,
                       (long long)H * W, z0, out_minmax);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" size_t mi_dbgvis_workspace_bytes(int nz, long n_pred, long n_gt) {
    if (nz <= 0 || n_pred < 0 || n_gt < 0 || n_pred + n_gt >= 0x3fffffffL) return 0;
    return mi_align_up(sizeof(int32_t) * index_words(nz, n_pred, n_gt), 16);
}

extern "C" int mi_dbgvis_render(const float* tomo, const float* hm_pred, const float* hm_gt, int D, int H, int W, int h, int w,
                                int z0, int nz, const float* minmax, const float* pred_dets, long n_pred, const float* gt_dets,
                                long n_gt, float conf_thresh, int radius, uint8_t* out, void* ws, size_t ws_bytes,
                                mi_stream_t stream) {
    if (!tomo || !hm_pred || !hm_gt || !minmax || !out || D <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 ||
        (long long)H != 2LL * h || (long long)W != 2LL * w || z0 < 0 || nz <= 0 || (long long)z0 + nz > D || nz > 65535 ||
        n_pred < 0 || n_gt < 0 || n_pred + n_gt >= 0x3fffffffL || (n_pred > 0 && !pred_dets) || (n_gt > 0 && !gt_dets) ||
        radius < 0 || !(conf_thresh == conf_thresh))
        return MI_E_ARG;
    if (radius > DBG_MAX_RADIUS) return MI_E_UNSUPPORTED;
    const size_t need = mi_dbgvis_workspace_bytes(nz, n_pred, n_gt);
    if (!ws || ws_bytes < need || ((uintptr_t)ws & 7)) return MI_E_WORKSPACE;
    const long long HW = (long long)H * W;
    const bool vec = W % 4 == 0 && ((uintptr_t)tomo & 15) == 0 && ((uintptr_t)out & 3) == 0;
    const int V = vec ? 4 : 2;
    const long long units = HW / V;
    if ((units + 255) / 256 > 0x7fffffffLL) return MI_E_UNSUPPORTED;

    // the index of the slab, on the host: lists of centres by slice, picks first, then the ground truth
    std::vector<int32_t> idx(need / sizeof(int32_t), 0);
    int32_t* pred_ptr = idx.data();
    int32_t* gt_ptr = pred_ptr + (nz + 1);
    ring_mask(radius, reinterpret_cast<unsigned long long*>(gt_ptr + (nz + 1)));
    int32_t* cen = gt_ptr + (nz + 1) + 2 * DBG_MASK_ROWS;
    std::vector<int> where((size_t)(n_pred + n_gt));
    for (long k = 0; k < n_pred; ++k) {
        const float* r = pred_dets + 5 * k;
        where[k] = r[4] > conf_thresh ? slab_slice(r, H, W, z0, nz) : -1;
        if (where[k] >= 0) ++pred_ptr[where[k] + 1];
    }
    for (long k = 0; k < n_gt; ++k) {
        where[n_pred + k] = slab_slice(gt_dets + 3 * k, H, W, z0, nz);
        if (where[n_pred + k] >= 0) ++gt_ptr[where[n_pred + k] + 1];
    }
    for (int i = 0; i < nz; ++i) pred_ptr[i + 1] += pred_ptr[i];
    gt_ptr[0] = pred_ptr[nz];
    for (int i = 0; i < nz; ++i) gt_ptr[i + 1] += gt_ptr[i];
    std::vector<int32_t> fill(2 * (size_t)nz);
    for (int i = 0; i < nz; ++i) { fill[i] = pred_ptr[i]; fill[nz + i] = gt_ptr[i]; }
    for (long k = 0; k < n_pred + n_gt; ++k) {
        if (where[k] < 0) continue;
        const float* r = k < n_pred ? pred_dets + 5 * k : gt_dets + 3 * (k - n_pred);
        const int slot = fill[(k < n_pred ? 0 : nz) + where[k]]++;
        cen[2 * slot] = (int)r[0];
        cen[2 * slot + 1] = (int)r[1];
    }
    // the source is pageable: the copy has taken it when the call returns
    const hipStream_t s = (hipStream_t)stream;
    MI_HIP(hipMemcpyAsync(ws, idx.data(), need, hipMemcpyHostToDevice, s));

    const dim3 grid((unsigned)((units + 255) / 256), (unsigned)nz);
    if (vec)
        hipLaunchKernelGGL(dbgvis_render_kernel<4>, grid, dim3(256), 0, s, tomo, hm_pred, hm_gt, H, W, h, w, z0, nz, minmax,
                           (const int*)ws, radius, units, out);
    else
        hipLaunchKernelGGL(dbgvis_render_kernel<2>, grid, dim3(256), 0, s, tomo, hm_pred, hm_gt, H, W, h, w, z0, nz, minmax,
                           (const int*)ws, radius, units, out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

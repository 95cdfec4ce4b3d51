// Random 3-D views of the MoCo training (task `moco`), on the device: both views of a batch are three launches.
//
// Replaces the torchio / numpy chain the reference runs per sample in DataLoader workers
//   datasets/tomo_pre.py:53-62       tio.Compose([RandomBlur(p=0.15), RandomNoise(p=0.5), RandomAffine(scales=(1, 1),
//        degrees=(0, 60, 0, 0, 0, 0), p=0.75), Crop(size // 8), ZNormalization, RescaleIntensity((-3, 3)), ZNormalization])
//   datasets/particle_pre.py:48-87   per view: flip_ud | flip_lr | none, then drop_out | center_out | swap_out | none
//   utils/image.py:481-536           the three erasures and the two flips
// on the S^3 box around a crop centre (S = c + 2 (c / 6): what Crop(S // 8) cuts down to the served c^3).
//
// The box (296 KB at c = 32) does not fit LDS, so aug3d_box_kernel marches z with one S x S plane in LDS - z taps of the
// separable blur straight from the tomogram, y and x passes in LDS, noise added on the way out - and leaves the blurred, noised
// box and its minimum (the rotation's fill value) in the caller's workspace.  aug3d_finish_kernel samples the rotated inner
// crop from that box into LDS, normalises it with the arithmetic of crop_norm.hip's mode 3 (znorm_chain.h) and writes it
// flipped and erased.  Plain f32 vector code; no atomics: every reduction has a fixed order, runs are bit-reproducible.
#include "common.h"
#include "philox.h"
#include "znorm_chain.h"

namespace {

// record layout (16 x 32 bit), counters and keys: see include/cetpick_hip.h
constexpr int R_WORDS = 16;
constexpr int A3_BOX_T = 1024, A3_FIN_T = 256, A3_MIN_C = 6, A3_MAX_C = 32, A3_MAX_R = 4;
constexpr uint32_t PARAM_TAG = 0x3D3D0000u, NOISE_TAG = 0x3D3E0000u;     // apart from mi_aug2d_params' and mi_aug2d3d_params' counters
enum { F_BLUR = 1, F_NOISE = 2, F_ROT = 4 };
enum { FLIP_NONE = 0, FLIP_Z = 1, FLIP_Y = 2 };
enum { ERASE_NONE = 0, ERASE_DROP = 1, ERASE_CENTRE = 2, ERASE_SWAP = 3 };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__host__ __device__ __forceinline__ int margin_of(int c) { return c / 6; }

// k-th entry of the corner set [0, c/2 - 2e) U [c/2 + e, c - e) (both halves hold c/2 - 2e entries)
__device__ __forceinline__ int corner_of(int k, int c, int e) {
    const int half = c / 2 - 2 * e;
    return k < half ? k : c / 2 + e + (k - half);
}

__global__ __launch_bounds__(256) void aug3d_params_kernel(const long long* __restrict__ ids, long long n,
                                                          unsigned long long seed, int epoch, int view0, int c,
                                                          mi_aug3d_ranges rg, int* __restrict__ table) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int view = view0 + blockIdx.y;
    const long long sid = ids[t];
    const uint32_t c0 = (uint32_t)sid, c1 = (uint32_t)((unsigned long long)sid >> 32), c2 = (uint32_t)epoch;
    const uint32_t c3 = (uint32_t)view | PARAM_TAG;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const u32x4 a = philox4x32_10(c0, c1, c2, c3, k0, k1);
    const u32x4 b = philox4x32_10(c0, c1, c2, c3 | (1u << 8), k0, k1);
    const u32x4 d = philox4x32_10(c0, c1, c2, c3 | (2u << 8), k0, k1);
    const u32x4 e0 = philox4x32_10(c0, c1, c2, c3 | (3u << 8), k0, k1);
    const u32x4 e1 = philox4x32_10(c0, c1, c2, c3 | (4u << 8), k0, k1);
    int flags = 0;
    if (unit_float(a.v[0]) < rg.blur_p) flags |= F_BLUR;
    if (unit_float(b.v[0]) < rg.noise_p) flags |= F_NOISE;
    if (unit_float(b.v[2]) < rg.rot_p) flags |= F_ROT;
    const float uf = unit_float(d.v[0]), ue = unit_float(d.v[1]);
    const int flip = uf < rg.flip_z_below ? FLIP_Z : (uf > rg.flip_y_above ? FLIP_Y : FLIP_NONE);
    const int erase = ue < rg.drop_below ? ERASE_DROP : (ue < rg.centre_below ? ERASE_CENTRE : (ue < rg.swap_below ? ERASE_SWAP : ERASE_NONE));
    const float sz = rg.sigma_lo + (rg.sigma_hi - rg.sigma_lo) * unit_float(a.v[1]);
    const float sy = rg.sigma_lo + (rg.sigma_hi - rg.sigma_lo) * unit_float(a.v[2]);
    const float sx = rg.sigma_lo + (rg.sigma_hi - rg.sigma_lo) * unit_float(a.v[3]);
    const float sn = rg.noise_lo + (rg.noise_hi - rg.noise_lo) * unit_float(b.v[1]);
    const float deg = rg.angle_lo + (rg.angle_hi - rg.angle_lo) * unit_float(b.v[3]);
    const double th = (double)deg * (3.14159265358979323846 / 180.0);
    // the two corners of an axis: one of the set, then one of the others (random.sample(set, 2))
    const int S = c + 2 * margin_of(c), e = S / 8, n_set = 2 * (c / 2 - 2 * e);
    int k0c[3], k1c[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        k0c[ax] = below(e0.v[ax], n_set);
        const int k = below(e1.v[ax], n_set - 1);
        k1c[ax] = k + (k >= k0c[ax] ? 1 : 0);
    }
    int4* o = reinterpret_cast<int4*>(table + ((long long)blockIdx.y * n + t) * R_WORDS);
    o[0] = make_int4(flags | (flip << 4) | (erase << 8), __float_as_int(sz), __float_as_int(sy), __float_as_int(sx));
    o[1] = make_int4(__float_as_int(sn), __float_as_int(deg), __float_as_int((float)cos(th)), __float_as_int((float)sin(th)));
    o[2] = make_int4(corner_of(k0c[0], c, e), corner_of(k0c[1], c, e), corner_of(k0c[2], c, e), corner_of(k1c[0], c, e));
    o[3] = make_int4(corner_of(k1c[1], c, e), corner_of(k1c[2], c, e), (int)d.v[2], (int)d.v[3]);
}

// ---- the chain -----------------------------------------------------------------------------------------------------
// scipy's `reflect` (d c b a | a b c d) for an index at most A3_MAX_R outside [0, S), S >= 2 A3_MAX_R
__device__ __forceinline__ int reflect(int i, int S) { return i < 0 ? -i - 1 : (i >= S ? 2 * S - 1 - i : i); }

// N(0, 1) of voxel `idx` of the box: Box-Muller on two words of Philox(counter (idx, 0, 0, NOISE_TAG), the record's key)
__device__ __forceinline__ float normal_of(uint32_t idx, uint32_t k0, uint32_t k1) {
    const u32x4 r = philox4x32_10(idx, 0u, 0u, NOISE_TAG, k0, k1);
    const float u1 = (float)((r.v[0] >> 8) + 1u) * (1.0f / 16777216.0f);            // (0, 1]
    const float u2 = unit_float(r.v[1]);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

struct Source {
    const mi_vol_desc* vols; const int* owner; const int* centres; const long long* ids; long long n_samples;
};

// grid (n, views).  Workspace of record r: S^3 floats of the blurred, noised box, then its minimum.
__global__ __launch_bounds__(A3_BOX_T) void aug3d_box_kernel(Source src, const int* __restrict__ table, long long n, int c,
                                                            long long ws_stride, float* __restrict__ ws) {
    extern __shared__ float planes[];                          // two S x S planes
    __shared__ float wgt[3][2 * A3_MAX_R + 1];
    __shared__ float red[A3_BOX_T / 64];
    const int tid = threadIdx.x;
    const long long t = blockIdx.x, rec = (long long)blockIdx.y * n + t;
    const long long sid = src.ids[t];
    if (sid < 0 || sid >= src.n_samples) return;               // (aug3d_finish_kernel writes the NaN rows)
    const int S = c + 2 * margin_of(c), pix = S * S;
    const int4 r0 = reinterpret_cast<const int4*>(table + rec * R_WORDS)[0];
    const int4 r1 = reinterpret_cast<const int4*>(table + rec * R_WORDS)[1];
    const int4 r3 = reinterpret_cast<const int4*>(table + rec * R_WORDS)[3];
    const int blur = r0.x & F_BLUR, noise = r0.x & F_NOISE;
    const float sigma_n = __int_as_float(r1.x);
    const uint32_t nk0 = (uint32_t)r3.z, nk1 = (uint32_t)r3.w;
    // gaussian_filter's taps per axis: radius int(4 sigma + 0.5) (at most A3_MAX_R whatever the record holds), normalised
    int rad[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const double sg = (double)__int_as_float(ax == 0 ? r0.y : (ax == 1 ? r0.z : r0.w));
        const double rr = 4.0 * sg + 0.5;
        rad[ax] = (blur && rr >= 1.0) ? (rr < (double)(A3_MAX_R + 1) ? (int)rr : A3_MAX_R) : 0;      // (NaN: 0)
        if (tid == ax) {
            double w[2 * A3_MAX_R + 1], sum = 0.0;
            for (int k = -rad[ax]; k <= rad[ax]; ++k) {
                w[k + rad[ax]] = rad[ax] ? exp(-0.5 * (double)(k * k) / (sg * sg)) : 1.0;
                sum += w[k + rad[ax]];
            }
            for (int k = 0; k <= 2 * rad[ax]; ++k) wgt[ax][k] = (float)(w[k] / sum);
        }
    }
    const mi_vol_desc d = src.vols[src.owner ? src.owner[sid] : 0];
    const int x0 = src.centres[3 * sid + 0] - S / 2, y0 = src.centres[3 * sid + 1] - S / 2, z0 = src.centres[3 * sid + 2] - S / 2;
    const long HW = (long)d.H * d.W;
    float* p0 = planes;
    float* p1 = planes + pix;
    float* box = ws + rec * ws_stride;
    float mn = INFINITY;
    __syncthreads();
    for (int z = 0; z < S; ++z) {
        for (int p = tid; p < pix; p += A3_BOX_T) {            // z taps, from the tomogram (a box that leaves it repeats the edge)
            const int y = p / S, x = p - y * S;
            const long off = (long)clampi(y0 + y, 0, d.H - 1) * d.W + clampi(x0 + x, 0, d.W - 1);
            float acc = wgt[0][0] * d.vol[(long)clampi(z0 + reflect(z - rad[0], S), 0, d.D - 1) * HW + off];
            for (int k = 1; k <= 2 * rad[0]; ++k)
                acc = fmaf(wgt[0][k], d.vol[(long)clampi(z0 + reflect(z - rad[0] + k, S), 0, d.D - 1) * HW + off], acc);
            p0[p] = acc;
        }
        __syncthreads();
        for (int p = tid; p < pix; p += A3_BOX_T) {            // y taps
            const int y = p / S, x = p - y * S;
            float acc = wgt[1][0] * p0[reflect(y - rad[1], S) * S + x];
            for (int k = 1; k <= 2 * rad[1]; ++k) acc = fmaf(wgt[1][k], p0[reflect(y - rad[1] + k, S) * S + x], acc);
            p1[p] = acc;
        }
        __syncthreads();                                       // (also: p0 is free for the next plane)
        for (int p = tid; p < pix; p += A3_BOX_T) {            // x taps, noise
            const int y = p / S, x = p - y * S;
            float acc = wgt[2][0] * p1[y * S + reflect(x - rad[2], S)];
            for (int k = 1; k <= 2 * rad[2]; ++k) acc = fmaf(wgt[2][k], p1[y * S + reflect(x - rad[2] + k, S)], acc);
            if (noise) acc += sigma_n * normal_of((uint32_t)(z * pix + p), nk0, nk1);
            box[(long)z * pix + p] = acc;
            mn = fminf(mn, acc);
        }
        // (p1 is written again only behind the next plane's first barrier)
    }
    mn = -wave_max(-mn);
    if ((tid & 63) == 0) red[tid >> 6] = mn;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < A3_BOX_T / 64; ++w) mn = fminf(mn, red[w]);
        box[(long)S * pix] = mn;
    }
}

// is (z, y, x) inside the e^3 box at corner (bz, by, bx)?
__device__ __forceinline__ bool in_box(int z, int y, int x, int bz, int by, int bx, int e) {
    return z >= bz && z < bz + e && y >= by && y < by + e && x >= bx && x < bx + e;
}

// grid (n, views); out is (views, n, c, c, c)
__global__ __launch_bounds__(A3_FIN_T) void aug3d_finish_kernel(const long long* __restrict__ ids, long long n_samples,
                                                               const int* __restrict__ table, long long n, int c,
                                                               long long ws_stride, const float* __restrict__ ws,
                                                               float* __restrict__ out) {
    extern __shared__ float buf[];                             // the c^3 crop
    const int tid = threadIdx.x, vox = c * c * c, cc = c * c;
    const long long t = blockIdx.x, rec = (long long)blockIdx.y * n + t;
    const long long sid = ids[t];
    float* o = out + rec * vox;
    if (sid < 0 || sid >= n_samples) {                         // a sample id outside the table: no read, a result nobody can miss
        for (int i = tid; i < vox; i += A3_FIN_T) o[i] = NAN;
        return;
    }
    const int m = margin_of(c), S = c + 2 * m, pix = S * S, e = S / 8, q = S / 4;
    const int4* rp = reinterpret_cast<const int4*>(table + rec * R_WORDS);
    const int4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
    const int rot = r0.x & F_ROT, flip = (r0.x >> 4) & 3, erase = (r0.x >> 8) & 3;
    const float cs = __int_as_float(r1.z), sn = __int_as_float(r1.w);
    // (a table may come from the caller: the erased boxes are kept inside the crop whatever it holds)
    const int az = clampi(r2.x, 0, c - e), ay = clampi(r2.y, 0, c - e), ax = clampi(r2.z, 0, c - e);
    const int bz = clampi(r2.w, 0, c - e), by = clampi(r3.x, 0, c - e), bx = clampi(r3.y, 0, c - e);
    const float* box = ws + rec * ws_stride;
    const float fill = box[(long)S * pix];
    const float ctr = 0.5f * (float)(S - 1), hi = (float)(S - 1);

    // Crop(m) of the rotated box: only these voxels are sampled.  Output (z, y, x) of the box reads plane z at
    // (ctr + cos (y - ctr) - sin (x - ctr), ctr + sin (y - ctr) + cos (x - ctr)), bilinear; outside [0, S - 1]: the minimum
    for (int i = tid; i < vox; i += A3_FIN_T) {
        const int z = i / cc, y = (i / c) % c, x = i % c;
        const float* pl = box + (long)(z + m) * pix;
        float v;
        if (!rot) {
            v = pl[(y + m) * S + (x + m)];
        } else {
            const float dy = (float)(y + m) - ctr, dx = (float)(x + m) - ctr;
            const float fy = ctr + (cs * dy - sn * dx), fx = ctr + (sn * dy + cs * dx);
            if (!(fy >= 0.0f && fy <= hi && fx >= 0.0f && fx <= hi)) {
                v = fill;
            } else {
                const int ya = (int)fy, xa = (int)fx;                                 // floor: fy, fx >= 0
                const int yb = ya + 1 > S - 1 ? S - 1 : ya + 1, xb = xa + 1 > S - 1 ? S - 1 : xa + 1;
                const float wy = fy - (float)ya, wx = fx - (float)xa;
                const float v00 = pl[ya * S + xa], v01 = pl[ya * S + xb], v10 = pl[yb * S + xa], v11 = pl[yb * S + xb];
                const float top = v00 + wx * (v01 - v00), bot = v10 + wx * (v11 - v10);
                v = top + wy * (bot - top);
            }
        }
        buf[i] = v;
    }
    const ZnormTail tail = znorm_rescale_in_lds(buf, vox);

    // flip, then erasure, as a gather: output voxel p of the erased array <- voxel (sz, sy, sx) of the flipped one
    for (int p = tid; p < vox; p += A3_FIN_T) {
        const int z = p / cc, y = (p / c) % c, x = p % c;
        int sz = z, sy = y, sx = x;
        bool zero = false;
        if (erase == ERASE_DROP) {
            zero = in_box(z, y, x, az, ay, ax, e);
        } else if (erase == ERASE_CENTRE) {
            zero = y < c / 2 - q || y >= c / 2 + q || x < c / 2 - q || x >= c / 2 + q;
        } else if (erase == ERASE_SWAP) {                      // box 0 is written first, box 1 over it: box 1 wins where they overlap
            if (in_box(z, y, x, bz, by, bx, e)) { sz = z - bz + az; sy = y - by + ay; sx = x - bx + ax; }
            else if (in_box(z, y, x, az, ay, ax, e)) { sz = z - az + bz; sy = y - ay + by; sx = x - ax + bx; }
        }
        if (flip == FLIP_Z) sz = c - 1 - sz;
        if (flip == FLIP_Y) sy = c - 1 - sy;
        o[p] = zero ? 0.0f : znorm_tail_value(buf[(sz * c + sy) * c + sx], tail);
    }
}

bool ranges_ok(const mi_aug3d_ranges* r) {
    if (!r) return false;
    const float ps[] = {r->blur_p, r->noise_p, r->rot_p, r->flip_z_below, r->flip_y_above, r->drop_below, r->centre_below, r->swap_below};
    for (float p : ps)
        if (!(p >= 0.f && p <= 1.f)) return false;
    if (!(r->drop_below <= r->centre_below) || !(r->centre_below <= r->swap_below)) return false;
    if (!(r->sigma_lo >= 0.f) || !(r->sigma_lo <= r->sigma_hi) || !(r->sigma_hi <= 1.f)) return false;      // radius <= A3_MAX_R
    if (!(r->noise_lo >= 0.f) || !(r->noise_lo <= r->noise_hi) || !(r->noise_hi < INFINITY)) return false;
    if (!(r->angle_lo <= r->angle_hi) || !(r->angle_lo >= -360.f) || !(r->angle_hi <= 360.f)) return false;
    return true;
}

// even c in 6..32 (the crop sits in LDS) whose erasure corner set has two entries per axis
bool crop_ok(int c) {
    if (c < A3_MIN_C || c > A3_MAX_C || (c & 1)) return false;
    const int e = (c + 2 * margin_of(c)) / 8;
    return e >= 1 && 2 * (c / 2 - 2 * e) >= 2;
}

size_t record_floats(int c) {
    const size_t S = (size_t)(c + 2 * margin_of(c));
    return mi_align_up(S * S * S + 1, 4);                      // 16-byte multiples
}

}  // namespace

extern "C" int mi_aug3d_params(const int64_t* sample_ids, int64_t n, uint64_t seed, int epoch, int view, int n_views, int crop,
                               const mi_aug3d_ranges* ranges, int32_t* table, mi_stream_t stream) {
    if (n == 0) return MI_OK;
    if (!sample_ids || !table || n < 0 || view < 0 || n_views < 1 || view + n_views > 256) return MI_E_ARG;
    if (!crop_ok(crop)) return MI_E_UNSUPPORTED;
    if (!ranges_ok(ranges)) return MI_E_ARG;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0xffffffffLL / 256) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(aug3d_params_kernel, dim3((unsigned)blocks, (unsigned)n_views), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)sample_ids, (long long)n, (unsigned long long)seed, epoch, view, crop, *ranges,
                       (int*)table);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" size_t mi_aug3d_workspace_bytes(int64_t n, int n_views, int crop) {
    if (n < 0 || n_views < 1 || !crop_ok(crop)) return 0;
    return (size_t)n * (size_t)n_views * record_floats(crop) * sizeof(float);
}

extern "C" int mi_aug3d_apply(const mi_vol_desc* vols, const int32_t* owner, const int32_t* centres_xyz, int64_t n_samples,
                              const int64_t* sample_ids, const int32_t* table, int64_t n, int n_views, int crop, float* out,
                              void* workspace, size_t workspace_bytes, mi_stream_t stream) {
    if (n == 0) return MI_OK;
    if (!vols || !centres_xyz || !sample_ids || !table || !out || n < 0 || n_samples < 1 || n_views < 1 || n_views > 256)
        return MI_E_ARG;
    if (((uintptr_t)table & 15) || ((uintptr_t)workspace & 15)) return MI_E_ARG;
    if (!crop_ok(crop)) return MI_E_UNSUPPORTED;
    if (n > 0xffffffffLL / A3_BOX_T) return MI_E_UNSUPPORTED;            // one workgroup per (sample, view)
    if (!workspace || workspace_bytes < mi_aug3d_workspace_bytes(n, n_views, crop)) return MI_E_WORKSPACE;
    const int S = crop + 2 * margin_of(crop);
    const long long stride = (long long)record_floats(crop);
    const size_t crop_bytes = sizeof(float) * (size_t)crop * crop * crop;
    static std::atomic<bool> lds_allowed[64];
    const int ra = mi_allow_dynamic_lds(lds_allowed, 128 * 1024, aug3d_finish_kernel);
    if (ra != MI_OK) return ra;
    const Source src{vols, (const int*)owner, (const int*)centres_xyz, (const long long*)sample_ids, (long long)n_samples};
    hipLaunchKernelGGL(aug3d_box_kernel, dim3((unsigned)n, (unsigned)n_views), dim3(A3_BOX_T), 2 * sizeof(float) * S * S,
                       (hipStream_t)stream, src, (const int*)table, (long long)n, crop, stride, (float*)workspace);
    MI_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(aug3d_finish_kernel, dim3((unsigned)n, (unsigned)n_views), dim3(A3_FIN_T), crop_bytes, (hipStream_t)stream,
                       (const long long*)sample_ids, (long long)n_samples, (const int*)table, (long long)n, crop, stride,
                       (const float*)workspace, out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

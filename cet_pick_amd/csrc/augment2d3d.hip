// Random views of the 2d3d exploration training (task `simsiam2d3d`), on the device: a batch of both views and both
// channels is two launches.
//
// Replaces the torchvision / PIL chains of the reference's 2d3d dataset
//   datasets/tomo_pre_proj_angle_select_new2d3d.py:49-82   strong: T.Compose([ToPILImage, RandomHorizontalFlip(0.5),
//        RandomVerticalFlip(0.5), RandomRotation(30), CenterCrop(bbox), ToTensor, CornerErasing(0.5, (0.01, 0.02), (0.5, 1.5)),
//        FixedRotation, Normalize((mean2d, mean3d), (std2d, std3d))]); weak: the same without the rotation
//   datasets/particle_pre_2d_proj_new2d3d.py:70-91         view 1 = strong(the pick's pair), view 2 = weak(a shifted variant's)
//   utils/image.py:195-201, 249-321                        FixedRotation, CornerErasing
// on a two-channel image (tilt patch, tomogram patch): both channels go through ONE set of random parameters.  The whole chain
// is a gather of 8-bit levels - flips, the library's nearest-neighbour rotation (an affine map in 16.16 fixed point), the
// erased rectangle, the quarter turn - so mi_aug2d3d_apply computes every output pixel from one bank read per channel, with no
// intermediate image.  mi_aug2d3d_params draws the records (Philox-4x32-10: pure functions of seed, epoch, sample id, view).
#include "common.h"
#include "philox.h"

namespace {

// record layout (16 x 32 bit): see include/cetpick_hip.h
constexpr int R_WORDS = 16;
constexpr int AUG_T = 256, AUG_MAX_BBOX = 128;
// keeps this stream of counters apart from mi_aug2d_params's (whose fourth counter word is view | draw << 8, below 2^16)
constexpr uint32_t STREAM_TAG = 0x2D3D0000u;

struct Ranges { float flip_p, a_lo, a_hi, erase_p, s_lo, s_hi, l_lo, l_hi; };      // l_*: log of the aspect ratio's ends

// FIX of the imaging library's affine transform: floor(65536 v + 0.5)
__device__ __forceinline__ int fix16(double v) {
#pragma clang fp contract(off)
    return (int)floor(v * 65536.0 + 0.5);
}
// round(v, 15) for |v| <= 1
__device__ __forceinline__ double round15(double v) {
#pragma clang fp contract(off)
    return rint(v * 1e15) / 1e15;
}

// the 16.16 coefficients of rotate(angle, NEAREST, expand=False, center=None) on a bbox x bbox image: output (y, x) reads
// input row (a5 + a4 y + a3 x) >> 16, column (a2 + a1 y + a0 x) >> 16
__device__ __forceinline__ void rotation_coefficients(float angle, int bbox, int* a) {
#pragma clang fp contract(off)
    double deg = fmod((double)angle, 360.0);
    if (deg < 0.0) deg += 360.0;
    const double th = -(deg * (3.14159265358979323846 / 180.0));
    const double m0 = round15(cos(th)), m1 = round15(sin(th)), m3 = round15(-sin(th)), m4 = m0;
    const double c = 0.5 * (double)bbox;
    const double m2 = (m0 * -c + m1 * -c) + c, m5 = (m3 * -c + m4 * -c) + c;
    a[0] = fix16(m0); a[1] = fix16(m1); a[3] = fix16(m3); a[4] = fix16(m4);
    a[2] = fix16((m2 + m0 * 0.5) + m1 * 0.5);
    a[5] = fix16((m5 + m3 * 0.5) + m4 * 0.5);
}

// CornerErasing's row (or column) for an extent e: [0, max(1, mid - e - 6)) above the centre, else
// [mid + 6, max(mid + 7, bbox - e + 6))
__device__ __forceinline__ int corner_start(int near, uint32_t r, int e, int bbox) {
    const int mid = bbox >> 1;
    if (near) { const int n = mid - e - 6; return below(r, n < 1 ? 1 : n); }
    const int lo = mid + 6, hi = bbox - e + 6;
    return lo + below(r, (hi < lo + 1 ? lo + 1 : hi) - lo);
}

// `get_params` of every random transform of the chain for one (sample, view).  Counter = (sample id, epoch,
// view | draw << 8 | tag), key = seed: three Philox draws per record.
__global__ __launch_bounds__(256) void aug2d3d_params_kernel(const long long* __restrict__ ids, long long n,
                                                            unsigned long long seed, int epoch, int bbox, Ranges strong,
                                                            Ranges weak, int* __restrict__ table) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int view = blockIdx.y;
    const Ranges rg = view ? weak : strong;
    const long long sid = ids[t];
    const uint32_t c0 = (uint32_t)sid, c1 = (uint32_t)((unsigned long long)sid >> 32), c2 = (uint32_t)epoch;
    const uint32_t c3 = (uint32_t)view | STREAM_TAG;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const u32x4 a = philox4x32_10(c0, c1, c2, c3, k0, k1);
    const u32x4 b = philox4x32_10(c0, c1, c2, c3 | (1u << 8), k0, k1);
    const u32x4 c = philox4x32_10(c0, c1, c2, c3 | (2u << 8), k0, k1);
    const int hflip = unit_float(a.v[0]) < rg.flip_p, vflip = unit_float(a.v[1]) < rg.flip_p;
    const float angle = rg.a_lo + (rg.a_hi - rg.a_lo) * unit_float(a.v[2]);        // RandomRotation: uniform_(lo, hi)
    const int erase = unit_float(a.v[3]) < rg.erase_p;
    const float share = rg.s_lo + (rg.s_hi - rg.s_lo) * unit_float(b.v[0]);
    const float aspect = expf(rg.l_lo + (rg.l_hi - rg.l_lo) * unit_float(b.v[1]));
    const float area = (float)(bbox * bbox) * share;
    const int mid = bbox >> 1;
    int h = (int)rintf(sqrtf(area * aspect)), w = (int)rintf(sqrtf(area / aspect));
    h = h < 0 ? 0 : (h > mid - 1 ? mid - 1 : h);                                    // (the entry refused ranges that reach mid)
    w = w < 0 ? 0 : (w > mid - 1 ? mid - 1 : w);
    const int i = corner_start(unit_float(b.v[2]) > 0.5f, c.v[0], h, bbox);
    const int j = corner_start(unit_float(b.v[3]) > 0.5f, c.v[1], w, bbox);
    int co[6];
    rotation_coefficients(angle, bbox, co);
    int4* o = reinterpret_cast<int4*>(table + ((long long)view * n + t) * R_WORDS);
    o[0] = make_int4(hflip | (vflip << 1) | (erase << 2), (int)(c.v[2] >> 30), i, j);
    o[1] = make_int4(h, w, __float_as_int(angle), 0);
    o[2] = make_int4(co[0], co[1], co[2], co[3]);
    o[3] = make_int4(co[4], co[5], 0, 0);
}

// clip the extent [start, start + len) of a record to [0, bbox) -> [lo, hi), empty when it lies outside
__device__ __forceinline__ void clip_extent(int start, int len, int bbox, int& lo, int& hi) {
    const int s = start < -bbox ? -bbox : (start > bbox ? bbox : start);
    const int l = len < 0 ? 0 : (len > bbox ? bbox : len);
    lo = s < 0 ? 0 : s;
    hi = s + l > bbox ? bbox : s + l;
}

struct PairStats { float mean2d, std2d, mean3d, std3d; };

// grid (B, 2 views); a workgroup makes both channels of one view of one sample.  out is (4, B, bbox, bbox): input, input_3d,
// input_aug, input_aug_3d.
__global__ __launch_bounds__(AUG_T) void aug2d3d_apply_kernel(const float* __restrict__ bank2d, const float* __restrict__ bank3d,
                                                             long long n_samples, int n_variants,
                                                             const long long* __restrict__ ids,
                                                             const long long* __restrict__ variants,
                                                             const int* __restrict__ table0, const int* __restrict__ table1,
                                                             long long B, int bbox, PairStats st, float* __restrict__ out) {
    const int tid = threadIdx.x, pix = bbox * bbox, view = blockIdx.y;
    const long long n = blockIdx.x;
    const long long sid = ids[n], var = view ? variants[n] : 0;
    float* o2 = out + ((long long)(2 * view) * B + n) * pix;
    float* o3 = out + ((long long)(2 * view + 1) * B + n) * pix;
    if (sid < 0 || sid >= n_samples || var < 0 || var >= n_variants) {       // outside the banks: no read, a result nobody can miss
        for (int p = tid; p < pix; p += AUG_T) { o2[p] = NAN; o3[p] = NAN; }
        return;
    }
    const int4* rec = reinterpret_cast<const int4*>((view ? table1 : table0) + n * R_WORDS);
    const int4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    const int hflip = r0.x & 1, vflip = (r0.x >> 1) & 1, erase = (r0.x >> 2) & 1, k = r0.y & 3;
    // (a table may come from the caller: the rectangle is clipped to the image, and a source index is used only inside it)
    int i0, i1, j0, j1;
    clip_extent(r0.z, r1.x, bbox, i0, i1);
    clip_extent(r0.w, r1.y, bbox, j0, j1);
    if (!erase) i1 = i0;
    const unsigned a0 = (unsigned)r2.x, a1 = (unsigned)r2.y, a2 = (unsigned)r2.z, a3 = (unsigned)r2.w, a4 = (unsigned)r3.x,
                   a5 = (unsigned)r3.y;
    const long long src = (sid * n_variants + var) * pix;
    const float* s2 = bank2d + src;
    const float* s3 = bank3d + src;
    // lanes run along the output x: the stores are coalesced whatever k is
    for (int p = tid; p < pix; p += AUG_T) {
        const int oy = p / bbox, ox = p - oy * bbox;
        int ry, rx;                                             // undo rot90(k): pixel of the erased image
        switch (k) {
            case 0: ry = oy; rx = ox; break;
            case 1: ry = ox; rx = bbox - 1 - oy; break;
            case 2: ry = bbox - 1 - oy; rx = bbox - 1 - ox; break;
            default: ry = bbox - 1 - ox; rx = oy; break;
        }
        float g2, g3;
        if (ry >= i0 && ry < i1 && rx >= j0 && rx < j1) {
            g2 = g3 = 255.0f;                                   // CornerErasing: value 1 after ToTensor
        } else {
            // the rotation's source pixel (unsigned arithmetic: whatever a caller's record holds, the sums wrap; the shift is
            // arithmetic)
            const int sy = (int)(a5 + a4 * (unsigned)ry + a3 * (unsigned)rx) >> 16;
            const int sx = (int)(a2 + a1 * (unsigned)ry + a0 * (unsigned)rx) >> 16;
            if (sy < 0 || sy >= bbox || sx < 0 || sx >= bbox) {
                g2 = g3 = 0.0f;                                 // fill
            } else {
                const int q = (vflip ? bbox - 1 - sy : sy) * bbox + (hflip ? bbox - 1 - sx : sx);       // undo the flips
                g2 = floorf(fminf(fmaxf(s2[q] * 255.0f, 0.0f), 255.0f));                               // ToPILImage
                g3 = floorf(fminf(fmaxf(s3[q] * 255.0f, 0.0f), 255.0f));
            }
        }
        o2[p] = (g2 / 255.0f - st.mean2d) / st.std2d;
        o3[p] = (g3 / 255.0f - st.mean3d) / st.std3d;
    }
}

bool ranges_ok(const mi_aug2d3d_ranges* r, int bbox, Ranges* out) {
    if (!r) return false;
    if (!(r->flip_p >= 0.f && r->flip_p <= 1.f) || !(r->erase_p >= 0.f && r->erase_p <= 1.f)) return false;
    if (!(r->angle_lo <= r->angle_hi) || !(r->angle_lo >= -360.f) || !(r->angle_hi <= 360.f)) return false;
    if (!(r->scale_lo > 0.f) || !(r->scale_lo <= r->scale_hi) || !(r->scale_hi <= 1.f)) return false;
    if (!(r->ratio_lo > 0.f) || !(r->ratio_lo <= r->ratio_hi) || !(r->ratio_hi < INFINITY)) return false;
    // CornerErasing retries while h >= mid or w >= mid: refuse ranges whose largest h or w could get there
    const double area = (double)bbox * bbox * r->scale_hi, mid = bbox / 2;
    if (rint(sqrt(area * r->ratio_hi) * (1.0 + 1e-6)) >= mid || rint(sqrt(area / r->ratio_lo) * (1.0 + 1e-6)) >= mid) return false;
    *out = Ranges{r->flip_p, r->angle_lo, r->angle_hi, r->erase_p, r->scale_lo, r->scale_hi,
                  (float)log((double)r->ratio_lo), (float)log((double)r->ratio_hi)};
    return true;
}

}  // namespace

extern "C" int mi_aug2d3d_params(const int64_t* sample_ids, int64_t n, uint64_t seed, int epoch, int bbox,
                                 const mi_aug2d3d_ranges* strong, const mi_aug2d3d_ranges* weak, int32_t* table,
                                 mi_stream_t stream) {
    if (n == 0) return MI_OK;
    if (!sample_ids || !table || n < 0) return MI_E_ARG;
    if (bbox < 8 || bbox > AUG_MAX_BBOX || (bbox & 1)) return MI_E_UNSUPPORTED;
    Ranges rs, rw;
    if (!ranges_ok(strong, bbox, &rs) || !ranges_ok(weak, bbox, &rw)) return MI_E_ARG;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0xffffffffLL / 256) return MI_E_UNSUPPORTED;           // grid x block stays below 2^32 threads
    hipLaunchKernelGGL(aug2d3d_params_kernel, dim3((unsigned)blocks, 2), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)sample_ids, (long long)n, (unsigned long long)seed, epoch, bbox, rs, rw, (int*)table);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_aug2d3d_apply(const float* patches_2d, const float* patches_3d, int64_t n_samples, int n_variants,
                                const int64_t* sample_ids, const int64_t* variants, const int32_t* table_strong,
                                const int32_t* table_weak, int64_t n, int bbox, float mean_2d, float std_2d, float mean_3d,
                                float std_3d, float* out, mi_stream_t stream) {
    if (n == 0) return MI_OK;
    if (!patches_2d || !patches_3d || !sample_ids || !variants || !table_strong || !table_weak || !out || n < 0 ||
        n_samples < 1 || n_variants < 1 || !(std_2d > 0.f) || !(std_3d > 0.f))
        return MI_E_ARG;
    if (bbox < 8 || bbox > AUG_MAX_BBOX || (bbox & 1)) return MI_E_UNSUPPORTED;
    if (n > 0xffffffffLL / AUG_T) return MI_E_UNSUPPORTED;               // one workgroup per (sample, view)
    hipLaunchKernelGGL(aug2d3d_apply_kernel, dim3((unsigned)n, 2), dim3(AUG_T), 0, (hipStream_t)stream, patches_2d, patches_3d,
                       (long long)n_samples, n_variants, (const long long*)sample_ids, (const long long*)variants,
                       (const int*)table_strong, (const int*)table_weak, (long long)n, bbox,
                       PairStats{mean_2d, std_2d, mean_3d, std_3d}, out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

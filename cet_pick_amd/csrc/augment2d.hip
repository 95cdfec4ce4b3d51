// Random view augmentation of the SimSiam exploration training, on the device (one workgroup per sample).
//
// Replaces the torchvision / PIL chains of the reference's `simsiam3d` dataset
//   datasets/tomo_pre_proj_angle_select_new3d_vol.py:49-89   T.Compose([ToPILImage, RandomHorizontalFlip(0.5),
//        RandomVerticalFlip(0.5), ColorJitter(0.5, 0.2, 0.3, 0.1), RandomResizedCrop(bbox, (0.8 | 0.9, 1), (1, 1)),
//        ToTensor, FixedRotation, Normalize(mean, std)])
//   datasets/particle_pre_3d_vol.py:70-85                    view 1 = strong(crop), view 2 = weak(random neighbour crop)
//   utils/image.py:195-201                                   FixedRotation = torch.rot90(img, k, dims=[1, 2])
// which run per sample in DataLoader workers there.  Here the crops already sit in HBM; a batch of one view is two
// launches: mi_aug2d_params draws the parameter records, mi_aug2d_apply runs the chain.
//
// The records come from a counter-based generator (Philox-4x32-10, Salmon et al., SC'11): a record is a pure function of
// (seed, epoch, sample id, view) - no state between launches, nothing that depends on the batch a sample lands in.
#include "common.h"
#include "philox.h"

namespace {

struct AugRanges { float flip_p, b_lo, b_hi, c_lo, c_hi, a_lo, a_hi; };

// record layout (8 x 32 bit): see include/cetpick_hip.h
constexpr int R_WORDS = 8;

struct AugRecord {
    int hflip, vflip, bright_first, s, i, j, k, nbr;
    float brightness, contrast;
};

// `get_params` of the reference's chain for one (sample, view).  Counter = (sample id, epoch, view | draw << 8),
// key = seed: two Philox draws per record.
__device__ __forceinline__ AugRecord draw_record(long long sid, unsigned long long seed, int epoch, int view, int bbox,
                                                 const AugRanges& rg) {
    const uint32_t c0 = (uint32_t)sid, c1 = (uint32_t)((unsigned long long)sid >> 32), c2 = (uint32_t)epoch;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const u32x4 a = philox4x32_10(c0, c1, c2, (uint32_t)view, k0, k1);
    const u32x4 b = philox4x32_10(c0, c1, c2, (uint32_t)view | (1u << 8), k0, k1);
    AugRecord r;
    r.hflip = unit_float(a.v[0]) < rg.flip_p;                           // RandomHorizontalFlip: rand() < p
    r.vflip = unit_float(b.v[2]) < rg.flip_p;
    r.bright_first = (int)(b.v[3] >> 31);                               // of the jitter's random order only this bit acts
    r.k = (int)((b.v[3] >> 16) & 3u);                                   // FixedRotation: np.random.choice(4)
    r.nbr = (int)((b.v[3] >> 8) & 3u);                                  // np.random.randint(1, 5) - 1
    r.brightness = rg.b_lo + (rg.b_hi - rg.b_lo) * unit_float(a.v[1]);
    r.contrast = rg.c_lo + (rg.c_hi - rg.c_lo) * unit_float(a.v[2]);
    const float u = rg.a_lo + (rg.a_hi - rg.a_lo) * unit_float(a.v[3]); // RandomResizedCrop: area share, aspect 1
    int s = (int)rintf((float)bbox * sqrtf(u));
    r.s = s < 1 ? 1 : (s > bbox ? bbox : s);
    r.i = below(b.v[0], bbox - r.s + 1);                                // randint(0, bbox - s + 1): top row, left column
    r.j = below(b.v[1], bbox - r.s + 1);
    return r;
}

__global__ __launch_bounds__(256) void aug2d_params_kernel(const long long* __restrict__ ids, long long n,
                                                          unsigned long long seed, int epoch, int view, int bbox,
                                                          AugRanges rg, int* __restrict__ table) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const AugRecord r = draw_record(ids[t], seed, epoch, view, bbox, rg);
    int4 lo, hi;
    lo.x = r.hflip | (r.vflip << 1) | (r.bright_first << 2);
    lo.y = __float_as_int(r.brightness);
    lo.z = __float_as_int(r.contrast);
    lo.w = r.s;
    hi.x = r.i; hi.y = r.j; hi.z = r.k; hi.w = r.nbr;
    int4* o = reinterpret_cast<int4*>(table + t * R_WORDS);
    o[0] = lo; o[1] = hi;
}

// ---- the chain -----------------------------------------------------------------------------------------------------
// 8-bit image blend as the imaging library performs it: out = (uint8)(d + f * (g - d)) in single precision, product and
// sum each rounded on their own (HIP contracts into an FMA by default), clipped, truncated
__device__ __forceinline__ int blend_level(int d, int g, float f) {
#pragma clang fp contract(off)
    const float prod = f * (float)(g - d);
    const float t = (float)d + prod;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// source coordinate of output pixel r of a resize from s to bbox pixels, half-pixel centres
__device__ __forceinline__ float src_coord(int r, float scale) {
#pragma clang fp contract(off)
    const float c = ((float)r + 0.5f) * scale;
    return c - 0.5f;
}

constexpr int AUG_T = 256, AUG_MAX_BBOX = 128;

__global__ __launch_bounds__(AUG_T) void aug2d_apply_kernel(const float* __restrict__ bank, long long n_samples, int n_banks,
                                                           const long long* __restrict__ ids, const int* __restrict__ table,
                                                           int bbox, float mean, float std, float* __restrict__ out) {
    extern __shared__ unsigned char img[];                  // bbox * bbox grey levels, flipped and jittered
    __shared__ int red[AUG_T / 64];
    const int tid = threadIdx.x, pix = bbox * bbox;
    const long long n = blockIdx.x;
    const long long sid = ids[n];
    float* o = out + n * pix;
    if (sid < 0 || sid >= n_samples) {                      // a sample id outside the bank: no read, a result nobody can miss
        for (int p = tid; p < pix; p += AUG_T) o[p] = NAN;
        return;
    }
    const int4 lo = reinterpret_cast<const int4*>(table + n * R_WORDS)[0];
    const int4 hi = reinterpret_cast<const int4*>(table + n * R_WORDS)[1];
    const int hflip = lo.x & 1, vflip = (lo.x >> 1) & 1, bright_first = (lo.x >> 2) & 1;
    const float fb = __int_as_float(lo.y), fc = __int_as_float(lo.z);
    // (a table may come from the caller: keep the window inside the crop whatever it holds)
    const int s = lo.w < 1 ? 1 : (lo.w > bbox ? bbox : lo.w);
    const int ci = hi.x < 0 ? 0 : (hi.x > bbox - s ? bbox - s : hi.x);
    const int cj = hi.y < 0 ? 0 : (hi.y > bbox - s ? bbox - s : hi.y);
    const int k = hi.z & 3;
    const int nb = n_banks > 1 ? (hi.w < 0 ? 0 : (hi.w >= n_banks ? n_banks - 1 : hi.w)) : 0;
    const float* src = bank + ((long long)nb * n_samples + sid) * pix;

    // ToPILImage: floor(255 x); flips; brightness when it is drawn first; the grey-level sum for the contrast's mean
    int sum = 0;
    for (int p = tid; p < pix; p += AUG_T) {
        const int y = p / bbox, x = p - y * bbox;
        int g = (int)floorf(fminf(fmaxf(src[p] * 255.0f, 0.0f), 255.0f));
        if (bright_first) g = blend_level(0, g, fb);
        img[(vflip ? bbox - 1 - y : y) * bbox + (hflip ? bbox - 1 - x : x)] = (unsigned char)g;
        sum += g;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    sum = 0;
#pragma unroll
    for (int w = 0; w < AUG_T / 64; ++w) sum += red[w];
    const int m = (2 * sum + pix) / (2 * pix);              // int(mean + 0.5)
    // contrast blends with the mean level, then brightness with black when it is drawn second (a thread revisits the pixels
    // it wrote itself: same p, same flipped position)
    for (int p = tid; p < pix; p += AUG_T) {
        const int y = p / bbox, x = p - y * bbox;
        const int q = (vflip ? bbox - 1 - y : y) * bbox + (hflip ? bbox - 1 - x : x);
        int g = blend_level(m, (int)img[q], fc);
        if (!bright_first) g = blend_level(0, g, fb);
        img[q] = (unsigned char)g;
    }
    __syncthreads();

    // crop [ci : ci + s, cj : cj + s] -> bilinear resize to bbox x bbox (half-pixel centres, taps clamped to the crop) ->
    // grey level -> / 255 -> rot90(k) -> Normalize.  Output pixel (oy, ox) of the rotated image is pixel (ry, rx) of the
    // resized one; lanes run along ox, so the stores are coalesced whatever k is.
    const float scale = (float)s / (float)bbox;
    for (int p = tid; p < pix; p += AUG_T) {
        const int oy = p / bbox, ox = p - oy * bbox;
        int ry, rx;
        switch (k) {
            case 0: ry = oy; rx = ox; break;
            case 1: ry = ox; rx = bbox - 1 - oy; break;
            case 2: ry = bbox - 1 - oy; rx = bbox - 1 - ox; break;
            default: ry = bbox - 1 - ox; rx = oy; break;
        }
        const float fy = src_coord(ry, scale), fx = src_coord(rx, scale);
        const float y0f = floorf(fy), x0f = floorf(fx);
        const float wy = fy - y0f, wx = fx - x0f;
        const int y0 = (int)y0f, x0 = (int)x0f;
        const int ya = ci + (y0 < 0 ? 0 : (y0 > s - 1 ? s - 1 : y0)), yb = ci + (y0 + 1 < 0 ? 0 : (y0 + 1 > s - 1 ? s - 1 : y0 + 1));
        const int xa = cj + (x0 < 0 ? 0 : (x0 > s - 1 ? s - 1 : x0)), xb = cj + (x0 + 1 < 0 ? 0 : (x0 + 1 > s - 1 ? s - 1 : x0 + 1));
        const float v00 = img[ya * bbox + xa], v01 = img[ya * bbox + xb], v10 = img[yb * bbox + xa], v11 = img[yb * bbox + xb];
        const float top = v00 + wx * (v01 - v00), bot = v10 + wx * (v11 - v10);
        const float v = top + wy * (bot - top);
        const float g = fminf(fmaxf(floorf(v + 0.5f), 0.0f), 255.0f);
        o[p] = (g / 255.0f - mean) / std;
    }
}

}  // namespace

extern "C" int mi_aug2d_params(const int64_t* sample_ids, int64_t n, uint64_t seed, int epoch, int view, int bbox, float flip_p,
                               float bright_lo, float bright_hi, float contrast_lo, float contrast_hi, float area_lo,
                               float area_hi, int32_t* table, mi_stream_t stream) {
    if (n == 0) return MI_OK;
    if (!sample_ids || !table || n < 0 || view < 0 || view > 255) return MI_E_ARG;
    if (bbox < 8 || bbox > AUG_MAX_BBOX) return MI_E_UNSUPPORTED;
    if (!(flip_p >= 0.f && flip_p <= 1.f) || !(bright_lo <= bright_hi) || !(contrast_lo <= contrast_hi) || !(bright_lo >= 0.f) ||
        !(contrast_lo >= 0.f) || !(area_lo > 0.f) || !(area_lo <= area_hi) || !(area_hi <= 1.f))
        return MI_E_ARG;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return MI_E_UNSUPPORTED;
    const AugRanges rg{flip_p, bright_lo, bright_hi, contrast_lo, contrast_hi, area_lo, area_hi};
    hipLaunchKernelGGL(aug2d_params_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)sample_ids, (long long)n, (unsigned long long)seed, epoch, view, bbox, rg, (int*)table);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_aug2d_apply(const float* bank, int64_t n_samples, int n_banks, const int64_t* sample_ids,
                              const int32_t* table, int64_t n, int bbox, float mean, float std, float* out,
                              mi_stream_t stream) {
    if (n == 0) return MI_OK;
    if (!bank || !sample_ids || !table || !out || n < 0 || n_samples < 1 || n_banks < 1 || !(std > 0.f)) return MI_E_ARG;
    if (bbox < 8 || bbox > AUG_MAX_BBOX) return MI_E_UNSUPPORTED;
    if (n > 0x7fffffffLL) return MI_E_UNSUPPORTED;                       // one workgroup per sample
    const size_t lds = mi_align_up((size_t)bbox * bbox, 16);
    hipLaunchKernelGGL(aug2d_apply_kernel, dim3((unsigned)n), dim3(AUG_T), lds, (hipStream_t)stream, bank, (long long)n_samples,
                       n_banks, (const long long*)sample_ids, (const int*)table, bbox, mean, std, out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

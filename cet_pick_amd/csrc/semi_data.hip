// Data path of the refinement (detector) training on listed tomograms and coordinate files:
//   mi_semi_labels  the label volume of one tomogram (datasets/tomo_moco.py:77-130 `load_data`: draw_umich_gaussian_3d at
//                   every downscaled particle, np.maximum of the stamps, hm == 0 -> -1 in the train split)
//   mi_semi_pairs   the crop pairs of one training batch (datasets/particle_moco.py:34-163, the non --pn branch: input,
//                   the flipped view and the label crop of every own / partner centre)
//
// Labels: every stamped value is >= 0 (gaussian3D, gaussian3D_discrete with labels 1 / 0), so on a zeroed volume the IEEE
// bits of the floats order like the floats: an unsigned atomic max on the bits is the float max, whatever the arrival
// order.  The stencil is the reference's float64 stencil cast once to float32 on the host; max and float32 rounding commute
// (rounding is monotone), so the result is the reference's np.maximum(float32 map, float64 stencil) bit for bit.
// One thread per (centre, stencil voxel): scatter-bound, a few MB of atomics for thousands of particles.
//
// Pairs: one 256-thread workgroup per crop, lanes along x (rows of 64 / 32 contiguous floats), 64-bit offsets.  The input
// crop is written twice, as is and mirrored (x or y) for the second view; the label crop once.
#include "common.h"

namespace {

constexpr int SP_T = 256;
constexpr int SP_CZ = 6, SP_C = 64, SP_CL = 32;                    // (6, 64, 64) input, (6, 32, 32) label at down_ratio 2
constexpr int SP_IN = SP_CZ * SP_C * SP_C, SP_HM = SP_CZ * SP_CL * SP_CL;

__global__ __launch_bounds__(256) void semi_scatter_kernel(float* __restrict__ hm, int D, int H, int W,
                                                           const int* __restrict__ centres, long long n,
                                                           const float* __restrict__ stencil, int r) {
    const int d = 2 * r + 1;
    const long long S = (long long)d * d * d, total = n * S;
    const long long HW = (long long)H * W;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long c = t / S;
        const int k = (int)(t - c * S);
        const float v = stencil[k];
        if (!(v > 0.f)) continue;                                     // (max with 0 on a zeroed volume: nothing to do)
        const int kz = k / (d * d), ky = (k / d) % d, kx = k % d;
        const long long x = (long long)centres[3 * c + 0] + kx - r;
        const long long y = (long long)centres[3 * c + 1] + ky - r;
        const long long z = (long long)centres[3 * c + 2] + kz - r;
        if (x < 0 || x >= W || y < 0 || y >= H || z < 0 || z >= D) continue;     // the box intersection of the reference
        __hip_atomic_fetch_max(reinterpret_cast<unsigned int*>(hm + z * HW + y * W + x), __float_as_uint(v),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void semi_fill_kernel(float* __restrict__ hm, long long total, int vec) {
    const long long n4 = vec ? total / 4 : 0;                        // (16-byte accesses only on a 16-byte aligned volume)
    float4* h4 = reinterpret_cast<float4*>(hm);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 v = h4[i];
        v.x = v.x == 0.f ? -1.f : v.x; v.y = v.y == 0.f ? -1.f : v.y;
        v.z = v.z == 0.f ? -1.f : v.z; v.w = v.w == 0.f ? -1.f : v.w;
        h4[i] = v;
    }
    for (long long i = 4 * n4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
        if (hm[i] == 0.f) hm[i] = -1.f;
}

__global__ __launch_bounds__(SP_T) void semi_pairs_kernel(const mi_vol_desc* __restrict__ tomos,
                                                          const mi_vol_desc* __restrict__ labels, int n_tomos,
                                                          const int* __restrict__ owner, const int* __restrict__ centres,
                                                          long long first, int flip_y, float* __restrict__ input,
                                                          float* __restrict__ input_aug, float* __restrict__ hm) {
    const long long i = blockIdx.x, s = first + i;
    const int tid = threadIdx.x;
    float* o_in = input + i * SP_IN;
    float* o_aug = input_aug + i * SP_IN;
    float* o_hm = hm + i * SP_HM;
    const int t = owner[s];
    const int x = centres[3 * s + 0], y = centres[3 * s + 1], z = centres[3 * s + 2];
    // The host draws only windows inside both volumes; a table entry that is not (or a bad owner) reads nothing.
    bool ok = t >= 0 && t < n_tomos;
    mi_vol_desc tv{}, lv{};
    if (ok) {
        tv = tomos[t];
        lv = labels[t];
        ok = z - SP_CZ / 2 >= 0 && z + SP_CZ / 2 <= tv.D && z + SP_CZ / 2 <= lv.D &&
             2 * y - SP_C / 2 >= 0 && 2 * y + SP_C / 2 <= tv.H && 2 * x - SP_C / 2 >= 0 && 2 * x + SP_C / 2 <= tv.W &&
             y - SP_CL / 2 >= 0 && y + SP_CL / 2 <= lv.H && x - SP_CL / 2 >= 0 && x + SP_CL / 2 <= lv.W;
    }
    if (!ok) {
        for (int p = tid; p < SP_IN; p += SP_T) { o_in[p] = 0.f; o_aug[p] = 0.f; }
        for (int p = tid; p < SP_HM; p += SP_T) o_hm[p] = 0.f;
        return;
    }
    // tomo[z-3 : z+3, 2y-32 : 2y+32, 2x-32 : 2x+32]
    const long long tHW = (long long)tv.H * tv.W;
    const float* src = tv.vol + (long long)(z - SP_CZ / 2) * tHW + (long long)(2 * y - SP_C / 2) * tv.W + (2 * x - SP_C / 2);
    for (int p = tid; p < SP_IN; p += SP_T) {
        const int cz = p / (SP_C * SP_C), cy = (p / SP_C) % SP_C, cx = p % SP_C;
        const float v = src[(long long)cz * tHW + (long long)cy * tv.W + cx];
        o_in[p] = v;
        // flip_ud (np.flip axis 1: y) or flip_lr (axis 2: x) of the (6, 64, 64) crop
        const int q = flip_y ? (cz * SP_C + (SP_C - 1 - cy)) * SP_C + cx : (cz * SP_C + cy) * SP_C + (SP_C - 1 - cx);
        o_aug[q] = v;
    }
    // hm[z-3 : z+3, y-16 : y+16, x-16 : x+16]
    const long long lHW = (long long)lv.H * lv.W;
    const float* lsrc = lv.vol + (long long)(z - SP_CZ / 2) * lHW + (long long)(y - SP_CL / 2) * lv.W + (x - SP_CL / 2);
    for (int p = tid; p < SP_HM; p += SP_T) {
        const int cz = p / (SP_CL * SP_CL), cy = (p / SP_CL) % SP_CL, cx = p % SP_CL;
        o_hm[p] = lsrc[(long long)cz * lHW + (long long)cy * lv.W + cx];
    }
}

}  // namespace

extern "C" int mi_semi_labels(float* hm, int D, int H, int W, const int32_t* centres_xyz, int64_t n, const float* stencil,
                              int r, int fill_unlabeled, mi_stream_t stream) {
    if (!hm || D <= 0 || H <= 0 || W <= 0 || n < 0 || r < 0 || r > 64 || (n > 0 && (!centres_xyz || !stencil)))
        return MI_E_ARG;
    const long long total = (long long)D * H * W;
    const hipStream_t s = (hipStream_t)stream;
    MI_HIP(hipMemsetAsync(hm, 0, sizeof(float) * (size_t)total, s));
    const long long work = n * (long long)(2 * r + 1) * (2 * r + 1) * (2 * r + 1);
    if (work > 0) {
        const long long blocks = (work + 255) / 256;
        hipLaunchKernelGGL(semi_scatter_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, hm, D, H,
                           W, (const int*)centres_xyz, (long long)n, stencil, r);
        MI_RETURN_IF_LAUNCH_FAILED();
    }
    if (fill_unlabeled) {
        const long long blocks = (total / 4 + 255) / 256 + 1;
        hipLaunchKernelGGL(semi_fill_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, s, hm, total,
                           (int)(((uintptr_t)hm & 15) == 0));
        MI_RETURN_IF_LAUNCH_FAILED();
    }
    return MI_OK;
}

extern "C" int mi_semi_pairs(const mi_vol_desc* tomos, const mi_vol_desc* labels, int n_tomos, const int32_t* owner,
                             const int32_t* centres_xyz, int64_t first, int n, int flip_y, float* input, float* input_aug,
                             float* hm, mi_stream_t stream) {
    if (n == 0) return MI_OK;
    if (!tomos || !labels || n_tomos <= 0 || !owner || !centres_xyz || !input || !input_aug || !hm || n < 0 || first < 0)
        return MI_E_ARG;
    hipLaunchKernelGGL(semi_pairs_kernel, dim3((unsigned)n), dim3(SP_T), 0, (hipStream_t)stream, tomos, labels, n_tomos,
                       (const int*)owner, (const int*)centres_xyz, (long long)first, flip_y, input, input_aug, hm);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

// Tilt-series patches of the 2d3d exploration mode, one workgroup per centre (mi_tilt_patches).
//
// Replaces the per-pick, per-tilt Python double loop of the reference dataset
//   datasets/tomo_pre_proj_angle_select_new2d3d.py:91-96   `convert_tomo_to_tilt`  (tomogram -> tilt x of each tilt)
//                                                 :110-133  `extract_patches`       (sum the tilt windows, min-max)
// run there five times per DoG pick in training (the pick and four shifted copies).  Every (pick, variant) of a dataset is
// one workgroup of one launch.
//
// Layout: the projected x of every tilt depends on the centre only, so 256 threads first project a chunk of tilts into LDS
// (the skip decision is then uniform over the workgroup: no divergence), then sweep the cy x cx window - lanes run along x,
// a row of the window is contiguous in the stack - summing the surviving tilts in tilt order into an LDS plane.  Min / max
// go through a wave then an LDS reduction; the normalised patch leaves as coalesced rows.  Gather-bound: each window row is
// read once per (centre, tilt); the stack itself (13 x 1024^2 fp32 = 52 MiB) stays resident in the Infinity Cache.
#include "common.h"

namespace {

constexpr int TP_T = 256;           // threads per workgroup
constexpr int TP_SKIP = INT32_MIN;  // tilt skipped for this centre

// Python evaluates (x - W//2)*cos + (z - Z//2)*sin + W//2 left to right in fp64, every product and sum rounded on its own, and
// int() truncates toward zero.  HIP contracts a*b + c into an FMA by default (and __dmul_rn / __dadd_rn are plain * and + in
// the HIP headers), which rounds once where Python rounds twice and can flip the int() at a boundary: contraction is off here.
__device__ __forceinline__ int project_x(double ax, double az, double w2, double c, double s) {
#pragma clang fp contract(off)
    const double px = ax * c;
    const double pz = az * s;
    return (int)((px + pz) + w2);
}

__global__ __launch_bounds__(TP_T) void tilt_patch_kernel(const mi_tilt_desc* __restrict__ stacks, int n_stacks,
                                                          const int* __restrict__ owner, const int* __restrict__ centres,
                                                          int cy, int cx, double bx, double by, float* __restrict__ out,
                                                          uint8_t* __restrict__ valid) {
    extern __shared__ float plane[];                 // cy * cx partial sums
    __shared__ int s_tx[TP_T];
    __shared__ int s_any;
    __shared__ float red[2][TP_T / 64];
    const long long i = blockIdx.x;
    const int tid = threadIdx.x, pix = cy * cx;
    float* o = out + i * (long long)pix;
    const int s = owner ? owner[i] : 0;
    if (s < 0 || s >= n_stacks) {                    // (a bad owner index: nothing is read)
        for (int p = tid; p < pix; p += TP_T) o[p] = 0.f;
        if (tid == 0) valid[i] = 0;
        return;
    }
    const mi_tilt_desc d = stacks[s];
    const int x = centres[3 * i + 0], y = centres[3 * i + 1], zf = centres[3 * i + 2];
    const long long HW = (long long)d.H * d.W;
    // ty = y for every tilt: the y half of the skip rule is the same for all of them
    const bool y_ok = !((double)y <= by || (double)y >= (double)d.H - by) && y - cy / 2 >= 0 && y + cy / 2 <= d.H;
    const double ax = (double)(x - d.W / 2), az = (double)((d.Zfull - zf) - d.Zfull / 2), w2 = (double)(d.W / 2);
    for (int p = tid; p < pix; p += TP_T) plane[p] = 0.f;
    if (tid == 0) s_any = 0;
    for (int t0 = 0; t0 < d.T; t0 += TP_T) {
        const int nt = min(TP_T, d.T - t0);
        __syncthreads();                             // (s_tx of the previous chunk has been used)
        if (tid < nt) {
            const int t = t0 + tid;
            const int tx = project_x(ax, az, w2, d.cos_sin[t], d.cos_sin[d.T + t]);
            const bool ok = y_ok && !((double)tx <= bx || (double)tx >= (double)d.W - bx) && tx - cx / 2 >= 0 &&
                            tx + cx / 2 <= d.W;
            s_tx[tid] = ok ? tx : TP_SKIP;
            if (ok) s_any = 1;
        }
        __syncthreads();
        const float* base = d.tilts + (long long)t0 * HW + (long long)(y - cy / 2) * d.W - cx / 2;
        for (int p = tid; p < pix; p += TP_T) {
            const int r = p / cx, c = p - r * cx;
            const float* row = base + (long long)r * d.W + c;
            float acc = plane[p];
            for (int k = 0; k < nt; ++k) {
                const int tx = s_tx[k];
                if (tx != TP_SKIP) acc += row[(long long)k * HW + tx];     // fp32, tilt order, as numpy's `patches += patch`
            }
            plane[p] = acc;
        }
    }
    __syncthreads();
    float mn = INFINITY, mx = -INFINITY;
    for (int p = tid; p < pix; p += TP_T) { mn = fminf(mn, plane[p]); mx = fmaxf(mx, plane[p]); }
    mn = -wave_max(-mn); mx = wave_max(mx);
    if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; }
    __syncthreads();
    mn = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    const bool ok = s_any && mn != mx;               // the reference returns None for both
    const float den = mx - mn;
    for (int p = tid; p < pix; p += TP_T) o[p] = ok ? (plane[p] - mn) / den : 0.f;   // a true division, as numpy's
    if (tid == 0) valid[i] = ok ? 1 : 0;
}

}  // namespace

extern "C" int mi_tilt_patches(const mi_tilt_desc* stacks, int n_stacks, const int32_t* owner, const int32_t* centres_xyz,
                               int64_t n, int cy, int cx, double bx, double by, float* out, uint8_t* valid,
                               mi_stream_t stream) {
    if (n == 0) return MI_OK;
    if (!stacks || n_stacks <= 0 || !centres_xyz || !out || !valid || n < 0) return MI_E_ARG;
    if (n > (int64_t)(UINT32_MAX / TP_T)) return MI_E_UNSUPPORTED;   // (gridDim.x * blockDim.x must stay below 2^32)
    if (cy <= 0 || cx <= 0 || (cy & 1) || (cx & 1)) return MI_E_ARG;
    const size_t lds = sizeof(float) * (size_t)cy * cx;
    if (lds > 48 * 1024) return MI_E_UNSUPPORTED;               // (+ the static arrays: within the 64 KiB of a workgroup)
    hipLaunchKernelGGL(tilt_patch_kernel, dim3((unsigned)n), dim3(TP_T), lds, (hipStream_t)stream, stacks, n_stacks,
                       (const int*)owner, (const int*)centres_xyz, cy, cx, bx, by, out, valid);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

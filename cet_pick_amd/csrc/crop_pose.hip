// The pose crops and the pose pooling of the MoCo-3D exploration inference (moco_test_3d.py).
//
//   mi_crop_znorm_poses   the z-normalised crop of mi_crop_normalize's mode 2 in P of the eight in-plane lattice poses of a
//                         cubic-in-plane box: pose p = `p & 3` quarter turns (torch.rot90 over (y, x)), then, with `p & 4`,
//                         the mirror along x.  One workgroup per sample: the source window is read ONCE into LDS (rows along
//                         x: lanes read consecutive floats), the statistics go through one workgroup reduction, the window is
//                         normalised in place, and every pose is a permuted copy of it whose lanes run along the OUTPUT's x - a
//                         quarter turn read straight from global memory would be a gather with a stride of one row per lane.
//                         In LDS that stride is the row pitch, kept odd: 32 consecutive lanes then sit on 32 different banks.
//   mi_embed_pool         F.normalize over every row of (n, P, dim), the mean over P, F.normalize again: one wave per pick.
#include "common.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

constexpr int CP_T = 1024;                           // the thread -> element map and the order of the sums are crop_fast_kernel's
constexpr size_t CP_MAX_LDS = 136 * 1024;            // 32^3 at pitch 33: 132 KiB of the CU's 160

// poses: pose k of the list in bits 3k .. 3k + 2
__global__ __launch_bounds__(CP_T) void crop_poses_kernel(const mi_vol_desc* __restrict__ vols, const int* __restrict__ owner,
                                                         const int* __restrict__ centres, long long first, int cz, int c,
                                                         int lcxp, int pitch, unsigned poses, int P, float* __restrict__ out) {
    extern __shared__ float win[];                   // cz * c rows of `pitch` floats
    __shared__ double rs[2][CP_T / 64];
    const long long i = first + blockIdx.x;
    const mi_vol_desc d = vols[owner ? owner[i] : 0];
    const int D = d.D, H = d.H, W = d.W;
    const int x0 = centres[3 * i + 0] - c / 2, y0 = centres[3 * i + 1] - c / 2, z0 = centres[3 * i + 2] - cz / 2;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cxp = 1 << lcxp, rpw = 64 >> lcxp;     // rows a wave takes per iteration
    const int x = lane & (cxp - 1), sub = lane >> lcxp;
    const int n_rows = cz * c, step = (CP_T / 64) * rpw;
    const bool x_ok = x < c;
    const int sx = clampi(x0 + x, 0, W - 1);
    const long HW = (long)H * W;
    const int row0 = wv * rpw + sub;
    const int z_first = row0 / c, y_first = row0 - z_first * c;       // (one division per thread; the marches below only add)
    const int dz = step / c, dy = step - dz * c;

    double s = 0, ss = 0;
    int z = z_first, y = y_first;
    for (int row = row0; row < n_rows; row += step) {
        if (x_ok) {
            const float v = d.vol[(long)clampi(z0 + z, 0, D - 1) * HW + (long)clampi(y0 + y, 0, H - 1) * W + sx];
            win[row * pitch + x] = v;
            s += v; ss += (double)v * v;
        }
        z += dz; y += dy;
        if (y >= c) { y -= c; ++z; }
    }
    s = wave_sum(s); ss = wave_sum(ss);
    if (lane == 0) { rs[0][wv] = s; rs[1][wv] = ss; }
    __syncthreads();
    double S = 0, SS = 0;
#pragma unroll
    for (int w = 0; w < CP_T / 64; ++w) { S += rs[0][w]; SS += rs[1][w]; }
    const int vox = n_rows * c;
    const double mean = S / vox;
    double var = (SS - vox * mean * mean) / (vox - 1);                // unbiased, as torch.std
    if (var < 0) var = 0;
    const float m = (float)mean, inv = (float)(1.0 / sqrt(var));      // zero variance: crop_fast_kernel's 1 / 0, nothing else
    for (int row = row0; row < n_rows; row += step)                   // (each thread: the elements it stored itself)
        if (x_ok) win[row * pitch + x] = (win[row * pitch + x] - m) * inv;
    __syncthreads();

    for (int k = 0; k < P; ++k) {
        const int p = (poses >> (3 * k)) & 7, r = p & 3;
        // output (yo, xo) of the pose reads window element ky * yo + kx * xs + k0, xs = xo or its mirror image
        const int ky = r == 0 ? pitch : r == 1 ? -1 : r == 2 ? -pitch : 1;
        const int kx = r == 0 ? 1 : r == 1 ? pitch : r == 2 ? -1 : -pitch;
        const int k0 = r == 0 ? 0 : r == 1 ? c - 1 : r == 2 ? (c - 1) * pitch + c - 1 : (c - 1) * pitch;
        const int xs = (p & 4) ? c - 1 - x : x;
        float* o = out + ((long)blockIdx.x * P + k) * vox;
        z = z_first; y = y_first;
        for (int row = row0; row < n_rows; row += step) {
            if (x_ok) o[(long)row * c + x] = win[z * c * pitch + ky * y + kx * xs + k0];
            z += dz; y += dy;
            if (y >= c) { y -= c; ++z; }
        }
    }
}

constexpr int EP_MAXK = 16;                          // dim <= 64 * EP_MAXK

__global__ __launch_bounds__(256) void embed_pool_kernel(const float* __restrict__ x, long n, int P, int dim,
                                                        float* __restrict__ out) {
    const long pick = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pick >= n) return;                           // (wave-uniform; no barrier below)
    const int lane = threadIdx.x & 63;
    float acc[EP_MAXK];
#pragma unroll
    for (int k = 0; k < EP_MAXK; ++k) acc[k] = 0.f;
    for (int p = 0; p < P; ++p) {
        const float* row = x + (pick * P + p) * dim;
        float v[EP_MAXK], ss = 0.f;
#pragma unroll
        for (int k = 0; k < EP_MAXK; ++k) {
            const int e = lane + 64 * k;
            v[k] = e < dim ? row[e] : 0.f;
            ss += v[k] * v[k];
        }
        const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);         // F.normalize: x / max(|x|, eps)
#pragma unroll
        for (int k = 0; k < EP_MAXK; ++k) acc[k] += v[k] / nrm;
    }
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < EP_MAXK; ++k) { acc[k] /= (float)P; ss += acc[k] * acc[k]; }
    const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
    float* o = out + pick * dim;
#pragma unroll
    for (int k = 0; k < EP_MAXK; ++k) {
        const int e = lane + 64 * k;
        if (e < dim) o[e] = acc[k] / nrm;
    }
}

}  // namespace

extern "C" int mi_crop_znorm_poses(const mi_vol_desc* vols, const int32_t* owner, const int32_t* centres_xyz, int64_t first,
                                   int n, int cz, int cy, int cx, const int32_t* poses, int n_poses, float* out,
                                   mi_stream_t stream) {
    if (!vols || !poses || n < 0 || first < 0) return MI_E_ARG;
    if (cz <= 0 || cy <= 0 || cx <= 0 || cy != cx || n_poses < 1 || n_poses > 8) return MI_E_ARG;
    unsigned packed = 0, seen = 0;
    for (int k = 0; k < n_poses; ++k) {
        const int p = poses[k];
        if (p < 0 || p > 7 || (seen >> p & 1)) return MI_E_ARG;
        seen |= 1u << p;
        packed |= (unsigned)p << (3 * k);
    }
    if (cx > 64) return MI_E_UNSUPPORTED;                             // a row is one wave access at most
    const int pitch = cx | 1;
    const size_t bytes = sizeof(float) * (size_t)cz * cy * pitch;
    if (bytes > CP_MAX_LDS) return MI_E_UNSUPPORTED;
    if (n == 0) return MI_OK;                                         // (an empty table or result has no address)
    if (!centres_xyz || !out) return MI_E_ARG;
    int l = 0;
    while ((1 << l) < cx) ++l;
    static std::atomic<bool> lds_allowed[64];
    const int ra = mi_allow_dynamic_lds(lds_allowed, (int)CP_MAX_LDS, crop_poses_kernel);
    if (ra != MI_OK) return ra;
    hipLaunchKernelGGL(crop_poses_kernel, dim3(n), dim3(CP_T), bytes, (hipStream_t)stream, vols, (const int*)owner,
                       (const int*)centres_xyz, (long long)first, cz, cx, l, pitch, packed, n_poses, out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_embed_pool(const float* x, long n, int P, int dim, float* out, mi_stream_t stream) {
    if (n < 0 || P < 1 || dim < 1) return MI_E_ARG;
    if (dim > 64 * EP_MAXK || n > (1l << 31)) return MI_E_UNSUPPORTED;
    if (n == 0) return MI_OK;                                         // (an empty tensor has no address)
    if (!x || !out) return MI_E_ARG;
    hipLaunchKernelGGL(embed_pool_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, n, P, dim, out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

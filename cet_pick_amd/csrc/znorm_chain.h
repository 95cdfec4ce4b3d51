// ZNormalization -> RescaleIntensity(-3, 3) -> ZNormalization of a crop that sits in LDS (datasets/tomo_pre.py:58-60), shared
// by mode 3 of crop_norm.hip and by the random 3-D views of augment3d.hip: one arithmetic, so a view whose random steps are all
// off is bit-identical to the mode-3 crop.  For workgroups of 256 threads; thread t owns voxels t, t + 256, ...
#pragma once
#include "common.h"

// block-wide (sum, sum of squares) in fp64 and (min, max) of per-thread partials; every thread gets the result
__device__ __forceinline__ void block_stats(double s, double ss, float mn, float mx, double* out_s, double* out_ss,
                                            float* out_mn, float* out_mx) {
    __shared__ double rs[2][4];
    __shared__ float rm[2][4];
    s = wave_sum(s); ss = wave_sum(ss);
    mn = -wave_max(-mn); mx = wave_max(mx);
    __syncthreads();                                  // (the buffers may still be read from the previous round)
    if ((threadIdx.x & 63) == 0) {
        rs[0][threadIdx.x >> 6] = s; rs[1][threadIdx.x >> 6] = ss;
        rm[0][threadIdx.x >> 6] = mn; rm[1][threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    *out_s = rs[0][0] + rs[0][1] + rs[0][2] + rs[0][3];
    *out_ss = rs[1][0] + rs[1][1] + rs[1][2] + rs[1][3];
    *out_mn = fminf(fminf(rm[0][0], rm[0][1]), fminf(rm[0][2], rm[0][3]));
    *out_mx = fmaxf(fmaxf(rm[1][0], rm[1][1]), fmaxf(rm[1][2], rm[1][3]));
}

// what the last ZNormalization still has to do to a value of the buffer
struct ZnormTail { float m, inv; };
__device__ __forceinline__ float znorm_tail_value(float v, ZnormTail t) { return (v - t.m) * t.inv; }

// buf[0 .. vox): the raw crop, each voxel written by the thread that owns it.  Two in-place passes (statistics of each pass in
// fp64) leave the rescaled crop in buf and return the last step's mean and 1 / std; every thread has passed a workgroup barrier
// after its last write, so on return any thread may read any voxel.
__device__ __forceinline__ ZnormTail znorm_rescale_in_lds(float* buf, int vox) {
    const int tid = threadIdx.x;
    double s = 0, ss = 0, S, SS;
    float mn = INFINITY, mx = -INFINITY, MN, MX;
    for (int i = tid; i < vox; i += 256) {
        const float v = buf[i];
        s += v; ss += (double)v * v;
    }
    block_stats(s, ss, 0.f, 0.f, &S, &SS, &MN, &MX);
    // ZNormalization: (x - mean) / std, unbiased
    double mean = S / vox, var = (SS - vox * mean * mean) / (vox - 1);
    float m = (float)mean, inv = (float)(1.0 / sqrt(var > 0 ? var : 0.0));
    for (int i = tid; i < vox; i += 256) {
        const float v = (buf[i] - m) * inv;
        buf[i] = v;
        mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
    block_stats(0, 0, mn, mx, &S, &SS, &MN, &MX);
    // RescaleIntensity(out_min_max = (-3, 3)): (x - min) / (max - min) * 6 - 3
    const float sc = 6.0f / (MX - MN);
    s = 0; ss = 0;
    for (int i = tid; i < vox; i += 256) {
        const float v = (buf[i] - MN) * sc - 3.0f;
        buf[i] = v;
        s += v; ss += (double)v * v;
    }
    block_stats(s, ss, 0.f, 0.f, &S, &SS, &MN, &MX);
    mean = S / vox; var = (SS - vox * mean * mean) / (vox - 1);
    return ZnormTail{(float)mean, (float)(1.0 / sqrt(var > 0 ? var : 0.0))};
}

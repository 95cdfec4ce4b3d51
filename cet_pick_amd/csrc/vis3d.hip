// 3-D visualisation of the exploration map (the reference's visualize_3dhm.py and the colour step of its plot_2d.py):
//   mi_vis_sample_colours  colour of every pick at its place on the 2-D map (colormap/colormap_2d.py:98-104 `_sample`)
//   mi_vis_slice_bytes     per slice: z-score, quantize(mi, ma) to a byte (visualize_3dhm.py:19-28,:126-130)
//   mi_vis_gauss_u8        scipy.ndimage.gaussian_filter(sigma 0.8) of the (Z, R, C, 3) uint8 stack of three equal channels (:133)
//   mi_vis_paint           the disc of every pick in the colour of its place on the map, last pick wins (:137-145)
//
// Gaussian.  With uint8 input scipy runs four 1-D passes (axes 0, 1, 2, 3), each accumulated in float64 in the order
//   t = in[0] w[3];  t += (in[-3] + in[3]) w[0];  t += (in[-2] + in[2]) w[1];  t += (in[-1] + in[1]) w[2]
// and truncated to uint8 before the next pass, with `reflect` borders (d c b a | a b c d | d c b a, repeating on an axis
// shorter than the radius).  The truncation forbids merging the weights of two passes, so the passes stay passes: z, rows,
// columns with byte intermediates in a workspace, and the channel pass (three equal values: every tap is the voxel itself, the
// same sum with all taps equal) in the registers of the column pass, which writes the three channels.  No FMA: a contracted
// product would change a truncation, so contraction is off for the whole file.  Per voxel 1 + 1, 1 + 1, 1 + 3 = 8 bytes of
// HBM traffic against 4 for a z-march with a row / column tile on chip (DESIGN.md 4.13 says why this form was built).
// A thread takes 4 consecutive voxels of a row as one 32-bit word when C is a multiple of 4 and the buffers are 4-byte
// aligned (then every row, and every 12-byte group of the output, starts on a word), one voxel with byte accesses otherwise.
// 64-bit voxel offsets: a 512 x 1024 x 1024 tomogram is 1.6 GB of output.
//
// Painter.  "Last pick wins" is made independent of the arrival order as mi_semi_labels does it: an atomic max of
// (pick number + 1) into an int32 index image that covers the slices that hold a pick (`slot_of_slice`), then a pass from
// index to colour over every slice of the slab [z0, z0 + nz); a slice without a slot stays zero.
#include "common.h"

#pragma clang fp contract(off)

namespace {

struct GaussW { double w0, w1, w2, w3; };                 // w[0], w[1], w[2] (the taps at distance 3, 2, 1) and the centre w[3]

// scipy's `reflect` at any distance from the axis: d c b a | a b c d | d c b a | a b c d ...
__device__ __forceinline__ int reflect(int i, int n) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// one output of a pass: c = in[0], s1 = in[-1] + in[1], s2 = in[-2] + in[2], s3 = in[-3] + in[3] (exact as integers)
__device__ __forceinline__ unsigned tap7(int c, int s1, int s2, int s3, const GaussW& w) {
    double t = (double)c * w.w3;
    t += (double)s3 * w.w0;
    t += (double)s2 * w.w1;
    t += (double)s1 * w.w2;
    return (unsigned)(int)t;                              // t >= 0: the cast truncates as scipy's does
}

__device__ __forceinline__ unsigned byte_of(unsigned word, int k) { return (word >> (8 * k)) & 0xffu; }

// A pass along z (stride R C, n = Z) or along the rows (stride C, n = R): the V voxels of a unit share their place on the axis.
template <int V>
__global__ __launch_bounds__(256) void vis_gauss_axis_kernel(const unsigned char* __restrict__ in,
                                                             unsigned char* __restrict__ out, long long units,
                                                             long long stride, int n, GaussW w) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    const long long i = u * V;
    const int pos = (int)((i / stride) % n);
    long long off[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) off[k] = i + (long long)(reflect(pos + k - 3, n) - pos) * stride;
    if (V == 4) {
        unsigned t[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) t[k] = *reinterpret_cast<const unsigned*>(in + off[k]);
        unsigned o = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            o |= tap7((int)byte_of(t[3], m), (int)(byte_of(t[2], m) + byte_of(t[4], m)), (int)(byte_of(t[1], m) + byte_of(t[5], m)),
                      (int)(byte_of(t[0], m) + byte_of(t[6], m)), w) << (8 * m);
        *reinterpret_cast<unsigned*>(out + i) = o;
    } else {
        int t[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) t[k] = in[off[k]];
        out[i] = (unsigned char)tap7(t[3], t[2] + t[4], t[1] + t[5], t[0] + t[6], w);
    }
}

// The pass along the columns, the channel pass on its result, and the three equal channels of the output.
template <int V>
__global__ __launch_bounds__(256) void vis_gauss_cols_kernel(const unsigned char* __restrict__ in,
                                                             unsigned char* __restrict__ out, long long units, int C,
                                                             GaussW w) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    const long long i = u * V;
    const int c = (int)(i % C);
    const unsigned char* row = in + (i - c);
    int b[V + 6];                                          // b[j] = the row at column c - 3 + j
    if (V == 4 && c >= 4 && c + 8 <= C) {
        const unsigned lo = *reinterpret_cast<const unsigned*>(row + c - 4);
        const unsigned mid = *reinterpret_cast<const unsigned*>(row + c);
        const unsigned hi = *reinterpret_cast<const unsigned*>(row + c + 4);
        b[0] = (int)byte_of(lo, 1); b[1] = (int)byte_of(lo, 2); b[2] = (int)byte_of(lo, 3);
#pragma unroll
        for (int m = 0; m < 4; ++m) b[3 + m] = (int)byte_of(mid, m);
        b[7] = (int)byte_of(hi, 0); b[8] = (int)byte_of(hi, 1); b[9] = (int)byte_of(hi, 2);
    } else {
#pragma unroll
        for (int j = 0; j < V + 6; ++j) b[j] = row[reflect(c - 3 + j, C)];
    }
    unsigned v[V];
#pragma unroll
    for (int m = 0; m < V; ++m) {
        const unsigned x = tap7(b[m + 3], b[m + 2] + b[m + 4], b[m + 1] + b[m + 5], b[m] + b[m + 6], w);
        v[m] = tap7((int)x, (int)(x + x), (int)(x + x), (int)(x + x), w);      // the channel axis: every tap is x
    }
    if (V == 4) {
        unsigned* o = reinterpret_cast<unsigned*>(out + 3 * i);                  // 12 bytes from a multiple of 12
        o[0] = v[0] | (v[0] << 8) | (v[0] << 16) | (v[1] << 24);
        o[1] = v[1] | (v[1] << 8) | (v[2] << 16) | (v[2] << 24);
        o[2] = v[2] | (v[3] << 8) | (v[3] << 16) | (v[3] << 24);
    } else {
        out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = (unsigned char)v[0];
    }
}

// visualize_3dhm.py:19-28 behind the z-score of :128-129; a slice of zero (or NaN) deviation gives 0
__global__ __launch_bounds__(256) void vis_slice_bytes_kernel(const float* __restrict__ x, unsigned char* __restrict__ out,
                                                              long long slice_elems, const double* __restrict__ stats,
                                                              double mi, double ma) {
    const long long s = blockIdx.y;
    const double mean = stats[4 * s], std = stats[4 * s + 1], r = ma - mi;
    const bool flat = !(std > 0.0);
    const float* xs = x + s * slice_elems;
    unsigned char* os = out + s * slice_elems;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < slice_elems; i += (long long)gridDim.x * 256) {
        double t = (double)xs[i] - mean;
        t = t / std;
        t = 255.0 * (t - mi) / r;
        t = t < 0.0 ? 0.0 : (t > 255.0 ? 255.0 : t);
        os[i] = flat || t != t ? (unsigned char)0 : (unsigned char)(int)rint(t);       // np.round: half to even
    }
}

// colormap_2d.py:98-104: table[clamp(round(x (W - 1)), 0, W - 1), clamp(round(y (H - 1)), 0, H - 1)], Python's round
// (half to even) on the float64 product
__device__ __forceinline__ int sample_index(float v, int n) {
    const double t = rint((double)v * (double)(n - 1));
    return t >= (double)(n - 1) ? n - 1 : (t > 0.0 ? (int)t : 0);                   // (a NaN goes to 0)
}

__global__ __launch_bounds__(256) void vis_sample_kernel(const float* __restrict__ y01, long long n,
                                                         const unsigned char* __restrict__ table, int W, int H,
                                                         unsigned char* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int ix = sample_index(y01[2 * i], W), iy = sample_index(y01[2 * i + 1], H);
    const unsigned char* t = table + ((long long)ix * H + iy) * 3;
    out[3 * i] = t[0]; out[3 * i + 1] = t[1]; out[3 * i + 2] = t[2];
}

constexpr int VIS_RADIUS = 12, VIS_REACH = 2;            // disc radius at the pick's own slice; slices it reaches above and below
constexpr int VIS_BOX = 2 * VIS_RADIUS + 1, VIS_DEPTH = 2 * VIS_REACH + 1;

// the disc rule (filled cv2.circle; its rim is not pinned)
__device__ __forceinline__ bool in_disc(int dx, int dy, int r) { return dx * dx + dy * dy <= r * r; }

// one thread per (pick, slice offset, pixel of the 25 x 25 box)
__global__ __launch_bounds__(256) void vis_paint_index_kernel(const int* __restrict__ picks, long long n,
                                                              const int* __restrict__ slot_of_slice, int n_slots, int R, int C,
                                                              int z0, int nz, int* __restrict__ index) {
    constexpr long long PER = (long long)VIS_DEPTH * VIS_BOX * VIS_BOX;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * PER) return;
    const long long i = t / PER;
    const int k = (int)(t - i * PER);
    const int dz = k / (VIS_BOX * VIS_BOX) - VIS_REACH, dy = (k / VIS_BOX) % VIS_BOX - VIS_RADIUS, dx = k % VIS_BOX - VIS_RADIUS;
    const long long s = (long long)picks[3 * i + 2] + dz;
    if (s < z0 || s >= (long long)z0 + nz) return;
    const int slot = slot_of_slice[s];
    if (slot < 0 || slot >= n_slots) return;
    if (!in_disc(dx, dy, VIS_RADIUS - (dz < 0 ? -dz : dz))) return;
    const long long col = (long long)picks[3 * i] + dx, row = (long long)picks[3 * i + 1] + dy;
    if (col < 0 || col >= C || row < 0 || row >= R) return;
    atomicMax(index + ((long long)slot * R + row) * C + col, (int)(i + 1));
}

template <int V>
__global__ __launch_bounds__(256) void vis_paint_colour_kernel(const int* __restrict__ index,
                                                               const int* __restrict__ slot_of_slice, int n_slots,
                                                               const unsigned char* __restrict__ colours, long long n,
                                                               long long RC, int z0, long long units,
                                                               unsigned char* __restrict__ out) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    const long long p = u * V;                             // voxel of the slab
    const int z = z0 + (int)(p / RC);
    const int slot = slot_of_slice[z];
    unsigned rgb[V];
#pragma unroll
    for (int m = 0; m < V; ++m) rgb[m] = 0;
    if (slot >= 0 && slot < n_slots) {
        const int* src = index + (long long)slot * RC + p % RC;
#pragma unroll
        for (int m = 0; m < V; ++m) {
            const long long k = src[m];
            if (k > 0 && k <= n) {
                const unsigned char* c = colours + 3 * (k - 1);
                rgb[m] = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
            }
        }
    }
    unsigned char* o = out + 3 * ((long long)z0 * RC + p);
    if (V == 4) {
        unsigned* ow = reinterpret_cast<unsigned*>(o);
        ow[0] = rgb[0] | (rgb[1] << 24);
        ow[1] = (rgb[1] >> 8) | (rgb[2] << 16);
        ow[2] = (rgb[2] >> 16) | (rgb[3] << 8);
    } else {
        o[0] = (unsigned char)rgb[0]; o[1] = (unsigned char)(rgb[0] >> 8); o[2] = (unsigned char)(rgb[0] >> 16);
    }
}

bool word_aligned(const void* p) { return ((uintptr_t)p & 3) == 0; }
bool fits_grid(long long units) { return (units + 255) / 256 <= 0x7fffffffLL; }
unsigned blocks_of(long long units) { return (unsigned)((units + 255) / 256); }

}  // namespace

extern "C" size_t mi_vis_gauss_workspace_bytes(long Z, long R, long C) {
    if (Z <= 0 || R <= 0 || C <= 0) return 0;
    return 2 * mi_align_up((size_t)Z * (size_t)R * (size_t)C, 16);
}

extern "C" int mi_vis_gauss_u8(const uint8_t* in, int Z, int R, int C, const double* weights7, uint8_t* out, void* ws,
                               size_t ws_bytes, mi_stream_t stream) {
    if (!in || !out || !weights7 || Z <= 0 || R <= 0 || C <= 0) return MI_E_ARG;
    if (!ws || ws_bytes < mi_vis_gauss_workspace_bytes(Z, R, C)) return MI_E_WORKSPACE;
    const long long total = (long long)Z * R * C;
    if (!fits_grid(total)) return MI_E_UNSUPPORTED;
    const GaussW w = {weights7[0], weights7[1], weights7[2], weights7[3]};
    unsigned char* t1 = (unsigned char*)ws;
    unsigned char* t2 = t1 + mi_align_up((size_t)total, 16);
    const hipStream_t s = (hipStream_t)stream;
    const bool vec = C % 4 == 0 && word_aligned(in) && word_aligned(out) && word_aligned(ws);
    const long long RC = (long long)R * C;
    if (vec) {
        const long long units = total / 4;
        hipLaunchKernelGGL(vis_gauss_axis_kernel<4>, dim3(blocks_of(units)), dim3(256), 0, s, in, t1, units, RC, Z, w);
        hipLaunchKernelGGL(vis_gauss_axis_kernel<4>, dim3(blocks_of(units)), dim3(256), 0, s, t1, t2, units, (long long)C, R, w);
        hipLaunchKernelGGL(vis_gauss_cols_kernel<4>, dim3(blocks_of(units)), dim3(256), 0, s, t2, out, units, C, w);
    } else {
        hipLaunchKernelGGL(vis_gauss_axis_kernel<1>, dim3(blocks_of(total)), dim3(256), 0, s, in, t1, total, RC, Z, w);
        hipLaunchKernelGGL(vis_gauss_axis_kernel<1>, dim3(blocks_of(total)), dim3(256), 0, s, t1, t2, total, (long long)C, R, w);
        hipLaunchKernelGGL(vis_gauss_cols_kernel<1>, dim3(blocks_of(total)), dim3(256), 0, s, t2, out, total, C, w);
    }
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_vis_slice_bytes(const float* x, long n_slices, long slice_elems, const double* stats, double mi, double ma,
                                  uint8_t* out, mi_stream_t stream) {
    if (!x || !out || !stats || n_slices <= 0 || slice_elems <= 0 || n_slices > 65535 || !(ma > mi)) return MI_E_ARG;
    const unsigned bx = (unsigned)std::max<long>(1, std::min<long>((slice_elems + 255) / 256, n_slices > 1 ? 256 : 4096));
    hipLaunchKernelGGL(vis_slice_bytes_kernel, dim3(bx, (unsigned)n_slices), dim3(256), 0, (hipStream_t)stream, x, out,
                       (long long)slice_elems, stats, mi, ma);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_vis_sample_colours(const float* y01, long n, const uint8_t* table, int W, int H, uint8_t* out,
                                     mi_stream_t stream) {
    if (n == 0) return MI_OK;
    if (!y01 || !table || !out || n < 0 || W <= 0 || H <= 0) return MI_E_ARG;
    if (!fits_grid(n)) return MI_E_UNSUPPORTED;
    hipLaunchKernelGGL(vis_sample_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, y01, (long long)n, table, W, H,
                       out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

extern "C" int mi_vis_paint(const int32_t* picks_xyz, const uint8_t* colours, long n, const int32_t* slot_of_slice, int n_slots,
                            int Z, int R, int C, int z0, int nz, int32_t* index, uint8_t* out, mi_stream_t stream) {
    if (!slot_of_slice || !out || Z <= 0 || R <= 0 || C <= 0 || n < 0 || n >= 0x7fffffffL || n_slots < 0 || z0 < 0 || nz <= 0 ||
        (long long)z0 + nz > Z || (n > 0 && (!picks_xyz || !colours)) || (n_slots > 0 && !index))
        return MI_E_ARG;
    const long long RC = (long long)R * C, slab = (long long)nz * RC;
    const long long work = (long long)n * VIS_DEPTH * VIS_BOX * VIS_BOX;
    if (!fits_grid(slab) || !fits_grid(work)) return MI_E_UNSUPPORTED;
    const hipStream_t s = (hipStream_t)stream;
    if (n_slots > 0) {
        MI_HIP(hipMemsetAsync(index, 0, sizeof(int32_t) * (size_t)n_slots * (size_t)RC, s));
        if (work > 0) {
            hipLaunchKernelGGL(vis_paint_index_kernel, dim3(blocks_of(work)), dim3(256), 0, s, (const int*)picks_xyz,
                               (long long)n, (const int*)slot_of_slice, n_slots, R, C, z0, nz, (int*)index);
            MI_RETURN_IF_LAUNCH_FAILED();
        }
    }
    if (C % 4 == 0 && word_aligned(out) && word_aligned(index))
        hipLaunchKernelGGL(vis_paint_colour_kernel<4>, dim3(blocks_of(slab / 4)), dim3(256), 0, s, (const int*)index,
                           (const int*)slot_of_slice, n_slots, colours, (long long)n, RC, z0, slab / 4, out);
    else
        hipLaunchKernelGGL(vis_paint_colour_kernel<1>, dim3(blocks_of(slab)), dim3(256), 0, s, (const int*)index,
                           (const int*)slot_of_slice, n_slots, colours, (long long)n, RC, z0, slab, out);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}

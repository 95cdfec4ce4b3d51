// Row-by-row products on the matrix cores: scores[i][j] = a_i . b_j for rows a (staged in LDS) against many columns b (an
// operand image in memory), in the bf16x3 arithmetic (bf16x3.h).  What kmeans.hip (best-of-k epilogue) and
// knn.hip (sorted top-k epilogue) share: device helpers, host-inline shapes and the prep kernel; no host state.  DESIGN.md 4.9.
//
// Image of `cols` columns of d features: image[((ct KS + ks) 3 + plane) 64 + lane] (16 bytes) = plane `plane` of the cut of
// column ct 32 + (lane & 31), features 16 ks + 8 (lane >> 5) .. + 7 - the B operand of one v_mfma_f32_32x32x16_bf16 is one
// contiguous 1 KB read.  Behind the planes: the columns' squared norms, KT 32 floats.
// LDS: the cut of 32 RM rows in three planes, row pitch KS 32 + 16 bytes (the 16-byte fragment reads of eight consecutive
// lanes fall on disjoint banks).
// Contract: a score is one fixed MFMA chain and a squared norm one fixed fmaf chain, whoever asks - the squared L2 distance
// of knn_search and the dist of kmeans_assign are the same bytes for the same pair of rows.
#pragma once
#include "common.h"
#include "bf16x3.h"

namespace rowdot {

using namespace bf3;

struct Shape { int KS; long KT; };        // k-steps of 16 features, column tiles of 32
inline Shape shape(long cols, int d) { return {(d + 15) / 16, (cols + 31) / 32}; }
inline size_t planes_bytes(long cols, int d) { const Shape s = shape(cols, d); return (size_t)s.KT * s.KS * 3 * 1024; }
inline size_t image_bytes(long cols, int d) { return planes_bytes(cols, d) + (size_t)shape(cols, d).KT * 32 * 4; }
__host__ __device__ inline int lds_pitch(int KS) { return KS * 32 + 16; }
inline size_t lds_planes_bytes(int rows, int KS) { return (size_t)rows * lds_pitch(KS) * 3; }

// eight consecutive features k8 .. k8 + 7 of one row (zero past d or when the row does not exist)
__device__ __forceinline__ void load8(const float* row, bool ok, int k8, int d, bool vec, float (&v)[8]) {
    if (ok && vec && k8 + 8 <= d) {
        ld8(row + k8, v);
    } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = (ok && k8 + t < d) ? row[k8 + t] : 0.f;
    }
}

// |row|^2 by one wave: lane l adds features l, l + 64, ...
__device__ __forceinline__ float row_sqnorm(const float* row, int d, int lane) {
    float s = 0.f;
    for (int f = lane; f < d; f += 64) s = fmaf(row[f], row[f], s);
    return wave_sum(s);
}

// accumulator register r of row tile m in lane half h = lane >> 5 holds row acc_row(m, r, h) of the workgroup's rows (and
// column lane & 31 of the tile)
__device__ __forceinline__ int acc_row(int m, int r, int h) { return m * 32 + (r & 3) + 8 * (r >> 2) + 4 * h; }

// the cut of rows row0 .. row0 + 32 RM - 1 of src (zeros from row n_rows on) into the three LDS planes; 256 threads
template <int RM>
__device__ __forceinline__ void stage_rows(unsigned char* lds, const float* src, long row0, long n_rows, int d, int KS, int tid) {
    constexpr int RT = 32 * RM;
    const int PITCH = lds_pitch(KS), PLANE = RT * PITCH;
    const bool vec = (d & 3) == 0;
    for (int q = tid; q < RT * 2 * KS; q += 256) {
        const int r = q / (2 * KS), g = q - r * 2 * KS;
        float v[8];
        load8(src + (size_t)(row0 + r) * d, row0 + r < n_rows, g * 8, d, vec, v);
        u32x4 o[3];
        cut8(v, o);
        store_planes(lds + r * PITCH + g * 16, PLANE, o);
    }
}

// acc[m] = the staged rows of row tile m against column tile ct of the image, one wave: per k-step three 1 KB fragment reads
// from the image, then per row tile three LDS fragment reads and the six products.  h = lane >> 5 and l32 = lane & 31 are
// the caller's own values (its epilogue needs them too): folded into the addresses from a private copy they cost the
// k-step loop of RM = 2 seven more vector additions.
template <int RM>
__device__ __forceinline__ void tile_product(f32x16 (&acc)[RM], const unsigned char* lds, const unsigned char* img, long ct, int KS,
                                             int lane, int h, int l32) {
    constexpr int RT = 32 * RM;
    const int PITCH = lds_pitch(KS), PLANE = RT * PITCH;
#pragma unroll
    for (int m = 0; m < RM; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    const unsigned char* bp = img + ((size_t)ct * KS * 3 * 64 + lane) * 16;
    for (int ks = 0; ks < KS; ++ks) {
        bf16x8 bf[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            bf[pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(bp + (size_t)(ks * 3 + pl) * 1024));
#pragma unroll
        for (int m = 0; m < RM; ++m) {
            bf16x8 af[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                af[pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(lds + pl * PLANE + (m * 32 + l32) * PITCH +
                                                                                     ks * 32 + h * 16));
#pragma unroll
            for (int pr = 0; pr < 6; ++pr)
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PA[pr]], bf[PB[pr]], acc[m], 0, 0, 0);
        }
    }
}

// One wave cuts `row` (d features; zeros when !ok) into column j of the image and returns its squared norm in every lane: the
// body of prep_kernel, and of a kernel that gathers its columns in an order of its own (cluster_quality.hip).
__device__ __forceinline__ float cut_column(const float* row, bool ok, long j, int d, int KS, int lane, unsigned char* img) {
    const bool vec = (d & 3) == 0;
    float s = 0.f;
    for (int g = lane; g < 2 * KS; g += 64) {
        float v[8];
        load8(row, ok, g * 8, d, vec, v);
#pragma unroll
        for (int t = 0; t < 8; ++t) s = fmaf(v[t], v[t], s);
        u32x4 o[3];
        cut8(v, o);
        const int ks = g >> 1, h = g & 1, l32 = (int)(j & 31);
        const long ct = j >> 5;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            *reinterpret_cast<u32x4*>(img + ((((size_t)ct * KS + ks) * 3 + pl) * 64 + h * 32 + l32) * 16) = o[pl];
    }
    return wave_sum(s);
}

namespace {     // a kernel of the including file: every code object registers a host stub of its own

// One wave per column j of x (cols, d): its cut into the image and its squared norm, pad_norm for the columns past the end
// (their planes are zeros).  Any whole number of waves per workgroup; the grid covers KT 32 columns.
__global__ __launch_bounds__(256) void prep_kernel(const float* x, long cols, int d, int KS, float pad_norm, unsigned char* img,
                                                   float* norm) {
    const long j = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const bool ok = j < cols;
    const float s = cut_column(x + (size_t)j * d, ok, j, d, KS, lane, img);
    if (lane == 0) norm[j] = ok ? s : pad_norm;
}

}  // namespace

}  // namespace rowdot

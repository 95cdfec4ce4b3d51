// The "bf16x3" arithmetic of every matrix-core kernel here: device helpers only, no kernels, no host state.
//
// An f32 operand is cut EXACTLY into three bf16 planes, a = a0 + a1 + a2, by truncation: a0 = the top 16 bits of a,
// r1 = a - a0 (<= 16 significant bits, so the subtraction is exact), a1 = the top 16 bits of r1, a2 = r1 - a1 (<= 8
// significant bits: a bf16 value).  Of the nine plane products the six of weight <= 2 (a2 b0, a0 b2, a1 b1, a1 b0, a0 b1,
// a0 b0 - smallest first, the order of PA / PB below) are accumulated in f32 by v_mfma_f32_32x32x16_bf16: each product is
// exact in f32, and the three dropped terms (a1 b2, a2 b1, a2 b2) are <= 2^-23 |a b| together, the size of ONE f32
// rounding - the result differs from an f32 fmaf chain by rounding-order noise only
// (tests/test_train_gpu.py::test_conv_bf16x3_is_f32_equivalent measures both against float64).  Caveat: an Inf operand
// becomes NaN (Inf - Inf in the cut) where an f32 multiply would keep Inf.  Six bf16 MFMAs of K = 16 take 192 cycles
// against 512 for the eight f32 MFMAs they replace.
//
// A kernel keeps its own MFMA loop (issue order across accumulator chains is tuned per kernel) and indexes PA / PB:
//   for pr < 6: acc = mfma_f32_32x32x16_bf16(a[PA[pr]], b[PB[pr]], acc)
#pragma once
#include <hip/hip_runtime.h>

namespace bf3 {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;      // operand of the transposing LDS read (ds_read_b64_tr_b16)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// operand planes of the six products, smallest terms first
constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};

constexpr unsigned HI16 = 0xffff0000u;      // the half of an f32 dword that is its bf16 truncation
constexpr unsigned HI2 = 0x07060302u;       // v_perm_b32: the high halves of two dwords -> one dword of two bf16

// Raw buffer descriptor of `bytes` bytes at `base`: a load whose offset falls outside [0, bytes) returns zeros without
// touching memory (zero padding, ragged tiles, a null operand with bytes = 0).  Flags word 0x00020000 (dword 3 of the
// descriptor): DATA_FORMAT (bits 15-18) = 4, a 32-bit element; every other field 0 - stride 0 with no swizzle and no
// index, i.e. raw addressing, the range check made on the byte offset against `bytes`.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
}

// the bf16 truncation of the f32 bits u, as an f32
__device__ __forceinline__ float top(unsigned u) { return __uint_as_float(u & HI16); }
// one step of the cut on bits: u minus its truncation (exact)
__device__ __forceinline__ unsigned rest(unsigned u) { return __float_as_uint(__uint_as_float(u) - top(u)); }
// two cut values -> one dword of two bf16, `lo` the first element
__device__ __forceinline__ unsigned pack2(unsigned hi, unsigned lo) { return __builtin_amdgcn_perm(hi, lo, HI2); }

// cut of one f32: the three bf16 bit patterns
__device__ __forceinline__ void cut3(float a, unsigned& h0, unsigned& h1, unsigned& h2) {
    const unsigned u0 = __float_as_uint(a);
    const float r1 = a - top(u0);
    const unsigned u1 = __float_as_uint(r1);
    const float r2 = r1 - top(u1);
    h0 = u0 >> 16; h1 = u1 >> 16; h2 = __float_as_uint(r2) >> 16;
}
// cut of N consecutive f32: u[plane][element], f32 bits whose high halves are the bf16 values
template <int N>
__device__ __forceinline__ void cut_bits(const float (&v)[N], unsigned (&u)[3][N]) {
#pragma unroll
    for (int t = 0; t < N; ++t) {
        u[0][t] = __float_as_uint(v[t]);
        const float r1 = v[t] - top(u[0][t]);
        u[1][t] = __float_as_uint(r1);
        u[2][t] = __float_as_uint(r1 - top(u[1][t]));
    }
}
// cut of 4 consecutive f32 (one 16-byte chunk): 8 bytes per plane
__device__ __forceinline__ void cut4(const float4 v, uint2 (&o)[3]) {
    const float e[4] = {v.x, v.y, v.z, v.w};
    unsigned u[3][4];
    cut_bits(e, u);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) o[pl] = make_uint2(pack2(u[pl][1], u[pl][0]), pack2(u[pl][3], u[pl][2]));
}
// cut of 8 consecutive f32: 16 bytes per plane, element e in half (e & 1) of dword e / 2 - an MFMA operand of 8 k values
__device__ __forceinline__ void cut8(const float (&v)[8], u32x4 (&o)[3]) {
    unsigned u[3][8];
    cut_bits(v, u);
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) o[pl][d] = pack2(u[pl][2 * d + 1], u[pl][2 * d]);
}
// ... as MFMA operands (written out, not a cast of the form above: the schedule of the contrastive-loss kernels follows it)
__device__ __forceinline__ void cut8(const float (&v)[8], bf16x8 (&o)[3]) {
    unsigned u[3][8];
    cut_bits(v, u);
    u32x4 p0, p1, p2;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        p0[d] = pack2(u[0][2 * d + 1], u[0][2 * d]);
        p1[d] = pack2(u[1][2 * d + 1], u[1][2 * d]);
        p2[d] = pack2(u[2][2 * d + 1], u[2][2 * d]);
    }
    o[0] = __builtin_bit_cast(bf16x8, p0); o[1] = __builtin_bit_cast(bf16x8, p1); o[2] = __builtin_bit_cast(bf16x8, p2);
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// 8 consecutive f32 (32 bytes, 16-byte aligned) as two 16-byte loads
__device__ __forceinline__ void ld8(const float* p, float (&v)[8]) {
    const float4 a = ld4(p), b = ld4(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
// the three planes of a cut, `plane_stride_bytes` apart
__device__ __forceinline__ void store_planes(unsigned char* dst, int plane_stride_bytes, const u32x4 (&o)[3]) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x4*>(dst + pl * plane_stride_bytes) = o[pl];
}

}  // namespace bf3

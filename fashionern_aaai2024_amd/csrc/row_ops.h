// Wave-per-row device arithmetic that more than one translation unit must compute BIT FOR BIT alike: the row registers and
// reductions of the row kernels (elem.hip), F.normalize's arithmetic (l2norm_kernel) and the per-row part of fern_gallery_prepare
// (sweep_bf16.hip).  live.hip writes rows into a prepared store with exactly these functions, which is what makes an upserted row
// indistinguishable from a prepared one.  One wave64 per row, 16-byte accesses.
#pragma once
#include "kernels.h"

namespace fern {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ROWS_PER_BLOCK = 4;   // 4 waves per workgroup, one row each
constexpr int MAXV = 5;             // row width <= 64 lanes * 4 floats * MAXV = 1280 (2 x 640 for the CLIP4Cir Combiner)

// Wave-wide reductions on the DPP network (quad swaps, half-row and row mirrors: every lane then holds its 16-lane row's value) plus
// four readlanes added in a fixed order -- ~10 issue slots, against six dependent ds_bpermute round trips (~100 cycles each) for the
// __shfl_xor butterfly.  The row kernels are one wave per row with two or three reductions each: that latency, not the bytes, was
// most of a LayerNorm launch.  Results are the same for every lane and depend only on the row (batch-invariant).
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }   // (readlane is an int builtin)
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_move<0xB1>(v);       // quad_perm [1,0,3,2]
    v += dpp_move<0x4E>(v);       // quad_perm [2,3,0,1]
    v += dpp_move<0x141>(v);      // row_half_mirror
    v += dpp_move<0x140>(v);      // row_mirror
    return (lane_f(v, 0) + lane_f(v, 16)) + (lane_f(v, 32) + lane_f(v, 48));
}

// A row of width d (d % 4 == 0, d <= 1024) held as up to MAXV float4 per lane: element c = (i*64 + lane)*4.
struct RowRegs {
    f32x4 v[MAXV];
};

// Four consecutive elements of a lane as fp32: one 16-byte load of fp32, or one 8-byte load of bf16 (widened exactly).
__device__ __forceinline__ f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 load4(const unsigned short* p) {
    const uint2 w = *reinterpret_cast<const uint2*>(p);
    return f32x4{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
}
template <class T>      // fp32 rows, or bf16 rows (the block-scaled mode's residual stream)
__device__ __forceinline__ void row_load(RowRegs& r, const T* x, int d, int lane) {
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (c < d) t = load4(x + c);
        r.v[i] = t;
    }
}
__device__ __forceinline__ void row_store(const RowRegs& r, float* y, int d, int lane) {
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < d) *reinterpret_cast<f32x4*>(y + c) = r.v[i];
    }
}
__device__ __forceinline__ float row_sumsq(const RowRegs& r) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) s += r.v[i][0] * r.v[i][0] + r.v[i][1] * r.v[i][1] + r.v[i][2] * r.v[i][2] + r.v[i][3] * r.v[i][3];
    return wave_sum(s);
}

// F.normalize / VisualSR.l2norm on a row in registers: mode 0 = x / max(||x||, eps), otherwise x / (||x|| + eps)
__device__ __forceinline__ void row_l2_normalize(RowRegs& r, float eps, int mode) {
    const float nrm = sqrtf(row_sumsq(r));
    const float den = mode == 0 ? fmaxf(nrm, eps) : nrm + eps;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) r.v[i] = r.v[i] / den;
}

// ---- fern_gallery_prepare, per row --------------------------------------------------------------------------------------------
// A lane visits the 4-float chunks c = lane * 4, lane * 4 + 256, ... of its row in ascending order: gallery_chunk returns the chunk's
// bf16 bits (round to nearest even) and adds the chunk to the lane's three partial sums of squares -- g - bf16(g) is exact in fp32;
// gallery_norms_fold adds the 64 lanes' sums in a fixed order and raises meta[0..2] to ||g - bf16(g)||, ||bf16(g)||, ||g||.  A row's
// bits and norms depend on nothing but the row, so a maximum that is only ever raised (live.hip) stays an upper bound.
struct GalleryNorms {
    float e2 = 0.f, t2 = 0.f, g2 = 0.f;
};
__device__ __forceinline__ ushort4 gallery_chunk(const f32x4 v, GalleryNorms& s) {
    // Roundings written out, contraction off: left to the compiler's fp-contract, WHICH products fuse into an fma depends on the code
    // around the call, and two kernels would disagree in the last bit.  These are the operations gallery_prepare_kernel has always
    // compiled to (pinned by its tests): the error terms are separately rounded squares added in order, the two norms are fma chains.
#pragma clang fp contract(off)
    ushort4 o;
    o.x = f32_to_bf16_bits(v[0]); o.y = f32_to_bf16_bits(v[1]); o.z = f32_to_bf16_bits(v[2]); o.w = f32_to_bf16_bits(v[3]);
    const float r0 = bf16_bits_to_f32(o.x), r1 = bf16_bits_to_f32(o.y), r2 = bf16_bits_to_f32(o.z), r3 = bf16_bits_to_f32(o.w);
    const float d0 = v[0] - r0, d1 = v[1] - r1, d2 = v[2] - r2, d3 = v[3] - r3;
    s.e2 = s.e2 + (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3);
    s.t2 = s.t2 + __builtin_fmaf(r3, r3, __builtin_fmaf(r2, r2, __builtin_fmaf(r0, r0, r1 * r1)));
    s.g2 = s.g2 + __builtin_fmaf(v[3], v[3], __builtin_fmaf(v[2], v[2], __builtin_fmaf(v[0], v[0], v[1] * v[1])));
    return o;
}
// meta[i] = max(meta[i], v) on the float's bit pattern: non-negative floats order like their bits, and NaN / inf rows poison the bound
// upwards (a NaN margin accepts every row).  The slot is only ever raised, so a value it already covers needs no atomic -- a stale read
// costs one atomic, never a miss -- and a million rows no longer queue on three addresses (one atomic per row and slot made the pass
// atomic-bound at ~35 ns per row, a hundredth of its HBM time).
__device__ __forceinline__ void raise_max(float* slot, float v) {
    unsigned* p = reinterpret_cast<unsigned*>(slot);
    const unsigned bits = __float_as_uint(v);
    if (bits > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, bits);
}
__device__ __forceinline__ void gallery_norms_fold(GalleryNorms s, int lane, float* meta) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { s.e2 += __shfl_xor(s.e2, m); s.t2 += __shfl_xor(s.t2, m); s.g2 += __shfl_xor(s.g2, m); }
    if (lane == 0) {
        raise_max(meta + 0, sqrtf(s.e2));
        raise_max(meta + 1, sqrtf(s.t2));
        raise_max(meta + 2, sqrtf(s.g2));
    }
}

}  // namespace fern

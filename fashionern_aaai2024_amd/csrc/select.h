// Ranking policy shared by the select kernels (topk.hip, topk_deep.hip, candidates.hip): the certificate margin of the pre-filter, the
// ranking key's way back to (score, global index), and the fp32 MFMA tile score.  (The wave and workgroup primitives are wave.h, the
// row-key rule is kernels.h, the exact chains of the survivors are rescore.h.)
#pragma once
#include "kernels.h"
#include "wave.h"

namespace fern {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- the certificate margin ------------------------------------------------------------------------------------------------------
// Pre-filter forms (api.hip: fern_sim_topk_prefiltered, the pre-filtered deep ranking): the scores a selection looks at are the bf16
// sweep's APPROXIMATIONS s~ of the exact fp32 scores s.  With q~ = bf16(q), g~ = bf16(g):  s - s~ = q.(g - g~) + (q - q~).g~  (+ the two
// accumulations' rounding), so
//     |s - s~| <= eps_b = ||q_b|| E + ||q_b - q~_b|| G~ + slack,   E = max_n ||g_n - g~_n||, G~ = max_n ||g~_n||   (Cauchy-Schwarz)
// for EVERY gallery row -- E, G~, G = max ||g_n|| come from fern_gallery_prepare (meta = {E, G~, G}), the query's two norms are computed
// here.  If T~ is the K-th best approximate score of the whole gallery, every row of the exact top-K has s~ >= T~ - 2 eps (K rows have
// s >= T~ - eps, so the exact K-th best is >= T~ - eps, and a row at or above it has s~ >= s - eps).  Any lower bound of T~ (a sample's
// K-th best, a wave bound l0) serves in T~'s place: margin = 2 eps_b.  slack covers fp32 accumulation in both dot products
// (D 2^-21 ||q|| max(G, G~): four times the textbook D u bound each, the MFMA's internal adder tree is not specified) and the rounding of
// the norms themselves.
// Two steps, because a kernel that has a score row to walk issues the query loads BEFORE the walk and reduces AFTER it (the row's
// 1-2 us round trips hide the query's):
//   margin_accumulate<NT>   thread t of NT: its strided share of ||q||^2 and ||q - bf16(q)||^2;
//   margin_finish<NWAVES>   wave xor-reduce, exchange through fred (2 * NWAVES floats of LDS; one barrier inside, none behind: a caller
//                           that reuses fred synchronises first), the sums in wave order 0 .. NWAVES - 1, then the eps arithmetic.
// The reduction tree and the order of the sums are part of the result's bits: the sweep's bound and the select kernel's cut must be
// the same number.
struct QueryNorms {
    float a, e;              // partial sums of q^2 and (q - bf16(q))^2
};
template <int NT>
__device__ __forceinline__ QueryNorms margin_accumulate(const float* q, int D) {
    QueryNorms n{0.f, 0.f};
    for (int i = threadIdx.x; i < D; i += NT) {
        const float v = q[i];
        const float d = v - bf16_bits_to_f32(f32_to_bf16_bits(v));      // exact
        n.a += v * v;
        n.e += d * d;
    }
    return n;
}
template <int NWAVES>
__device__ __forceinline__ float margin_finish(QueryNorms n, int D, const float* meta, float* fred) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) { n.a += __shfl_xor(n.a, x); n.e += __shfl_xor(n.e, x); }
    if (lane == 0) { fred[wave] = n.a; fred[NWAVES + wave] = n.e; }
    __syncthreads();
    float a = fred[0], e = fred[NWAVES];
#pragma unroll
    for (int w = 1; w < NWAVES; ++w) { a += fred[w]; e += fred[NWAVES + w]; }
    const float nq = sqrtf(a), eq = sqrtf(e);
    const float E = meta[0], Gt = meta[1], G = meta[2];
    const float eps = (nq * E + eq * Gt) * 1.00390625f + (float)D * 4.76837158203125e-7f * nq * fmaxf(G, Gt);      // (1 + 2^-8); D 2^-21
    return 2.0f * eps * 1.0009765625f;      // NaN (a NaN / inf row or query) makes every compare accept: the exact pass sorts it out
}

// ---- ranking key -> output slot --------------------------------------------------------------------------------------------------
// write_row: the key of a row (never 0: make_key of a row index below 2^32 - 1).  write_key: key 0 = no row: (-inf, -1)
__device__ __forceinline__ void write_row(u64 key, long idx_offset, float* os, int* oi) {
    *os = unorderable((unsigned)(key >> 32));
    *oi = (int)((long)(0xFFFFFFFFu - (unsigned)key) + idx_offset);
}
__device__ __forceinline__ void write_key(u64 key, long idx_offset, float* os, int* oi) {
    float sc = -INFINITY;
    int idx = -1;
    if (key != 0) write_row(key, idx_offset, &sc, &idx);
    *os = sc;
    *oi = idx;
}

// ---- one 32 x 32 fp32 score tile -------------------------------------------------------------------------------------------------
// v_mfma_f32_32x32x2_f32 per 8-group g8 and e = 0..3, lane half lh feeding k = 8 g8 + 4 lh + e (gemm.hip's sweep): THE chain order
// (oracle/chain.c) every bit-identity test pins.  qrow / grow: this lane's A row (query) and B row (gallery row, clamped by the caller).
// Register r of lane (n & 31) + 32 lh holds the score of gallery row n for query (r & 3) + 8 (r >> 2) + 4 lh.  D % 8 == 0.
__device__ __forceinline__ f32x16 score_tile_f32(const float* qrow, const float* grow, int D, int lh) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int g8 = 0; g8 < D / 8; ++g8) {
        const f32x4 af = *reinterpret_cast<const f32x4*>(qrow + g8 * 8 + lh * 4);
        const f32x4 bf = *reinterpret_cast<const f32x4*>(grow + g8 * 8 + lh * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], bf[e], acc, 0, 0, 0);
    }
    return acc;
}

}  // namespace fern

// Exact fp32 chain scoring of gallery rows, shared by the ranking kernels: the chain itself (chain_run), its per-lane stager for 16
// named rows (chain_rows_lane: rank.hip's key producer, candidates.hip) and the ring stager for 32 survivors (rescore_rows /
// rescore_keys: topk.hip, topk_deep.hip, candidates.hip).
#pragma once
#include "kernels.h"
#include "wave.h"

namespace fern {

constexpr int RESC_CH = 32;                     // k per step of the transposing tile
constexpr int RESC_TLD = RESC_CH + 4;           // floats per tile row (+ 4: lane l's ds_read_b128 of row l starts 4 banks after lane l-1's)
constexpr int RESC_ROWS = 32;                   // survivors per wave and round

// One lane continues one row's chain over kn staged k (kn % 8 == 0) in the sweep's order: inside every 8 consecutive k, 0 4 1 5 2 6 3 7
// (oracle/chain.c).  One rounding per product, as v_mfma_f32_32x32x2_f32 does it.  grow / qk: 16-byte aligned, the row's and the query's
// floats of those k.
__device__ __forceinline__ float chain_run(const float* grow, const float* qk, int kn, float acc) {
    for (int k8 = 0; k8 < kn; k8 += 8) {
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(grow + k8), g1 = *reinterpret_cast<const f32x4*>(grow + k8 + 4);
        const f32x4 q0 = *reinterpret_cast<const f32x4*>(qk + k8), q1 = *reinterpret_cast<const f32x4*>(qk + k8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc = __builtin_fmaf(q0[e], g0[e], acc);
            acc = __builtin_fmaf(q1[e], g1[e], acc);
        }
    }
    return acc;
}

// The per-lane form of the chain: one wave, CHAIN_T rows named by row_of(t) (t < CHAIN_T: the row's first float, always a readable
// row) against qrow over D (D % 8 == 0).  A step brings CH k of the 16 rows and of the query into the wave's tile with 16-byte loads --
// CH / 4 lanes per row, 64 / (CH / 4) rows per load instruction, all loads of a step in flight behind one wait -- and lane t < CHAIN_T
// then continues row t's chain over those k.  Returns that chain in lanes 0 .. CHAIN_T - 1.  The chain order does not depend on CH;
// CH decides the tile ((CHAIN_T + 1) x (CH + 4) floats, wave-private) and the loads in flight.
// Synchronisation is WAVE-LOCAL, no workgroup barrier: the tile belongs to one wave, a wave's LDS instructions execute in program
// order (a step's tile writes cannot pass the previous step's chain reads), the s_waitcnt makes the writes land before the chain
// reads them, and the two wave barriers only keep the compiler from moving LDS accesses across those points.  So waves of one
// workgroup may run their rounds independently (candidates.hip), and a one-wave workgroup (rank.hip) needs nothing more.
constexpr int CHAIN_T = 16;
template <int CH>
constexpr int chain_tile_floats() { return (CHAIN_T + 1) * (CH + 4); }      // + 4: lane l's ds_read_b128 of row l starts 4 banks after lane l - 1's
template <int CH, class RowOf>
__device__ __forceinline__ float chain_rows_lane(RowOf row_of, const float* qrow, int D, float* tile) {
    constexpr int LD = CH + 4, LPR = CH / 4, RPL = 64 / LPR, NL = CHAIN_T / RPL;      // lanes per row, rows per load, loads per step
    static_assert(CH == 128 || CH == 256, "a row's step is one 16-byte load of 32 or 64 lanes");
    const int lane = threadIdx.x & 63, lrow = lane / LPR, lcol = (lane % LPR) * 4;
    const float* src[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) src[i] = row_of(RPL * i + lrow);
    float acc = 0.0f;
    for (int k0 = 0; k0 < D; k0 += CH) {
        const int kc = k0 + lcol;
        const bool in = kc < D;
        f32x4 v[NL + 1];
#pragma unroll
        for (int i = 0; i < NL; ++i) v[i] = *reinterpret_cast<const f32x4*>(src[i] + (in ? kc : 0));
        v[NL] = *reinterpret_cast<const f32x4*>(qrow + (in ? kc : 0));
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < NL; ++i) *reinterpret_cast<f32x4*>(tile + (RPL * i + lrow) * LD + lcol) = v[i];
        if (lrow == 0) *reinterpret_cast<f32x4*>(tile + CHAIN_T * LD + lcol) = v[NL];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        if (lane < CHAIN_T) acc = chain_run(tile + lane * LD, tile + CHAIN_T * LD, min(CH, D - k0), acc);
    }
    return acc;
}

// One wave, 32 survivors surv[s0 .. s0 + 32) (rows past ns redo survivor s0): their exact fp32 chains against qrow.  D = 32 nsteps k,
// nsteps % RING == 0.  A step is four load instructions (8 rows x 32 floats each: whole 128-byte lines) whose registers go through
// the wave's LDS tile so that lane l < 32 can continue survivor l's chain over those 32 k.  The loads of the next RING steps are always
// in flight -- a register ring, a slot refilled right after its registers were written to the tile -- and the tile is double buffered:
// step c + 1 is written while step c is read.  The loop body is BRANCH-FREE (loads past the row's end re-read its last step, the
// tile write after the last step is never read): behind `if (c < nsteps)` guards the compiler waited for every load right after
// issuing it (s_waitcnt vmcnt(0..3) in front of each tile write) and the ring was one deep.
template <int RING>
__device__ __forceinline__ float rescore_rows(const unsigned* surv, int s0, int ns, const float* qrow, const float* gallery, int D, float* tl) {
    const int lane = threadIdx.x & 63;
    const int lrow = lane >> 3, lcol = (lane & 7) * 4;       // loader role: row inside a group of 8, float offset inside a 32-float step
    const int l31 = lane & 31;
    const int nsteps = D / RESC_CH;
    const float* src[4];
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
        const int r = s0 + rg * 8 + lrow;
        src[rg] = gallery + (long)surv[r < ns ? r : s0] * D + lcol;
    }
    f32x4 reg[RING][4];
#pragma unroll
    for (int c = 0; c < RING; ++c)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) reg[c][rg] = *reinterpret_cast<const f32x4*>(src[rg] + c * RESC_CH);      // nsteps >= RING
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) *reinterpret_cast<f32x4*>(tl + (rg * 8 + lrow) * RESC_TLD + lcol) = reg[0][rg];      // step 0's tile
    {
        const int cn = RING < nsteps ? RING : nsteps - 1;
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) reg[0][rg] = *reinterpret_cast<const f32x4*>(src[rg] + cn * RESC_CH);
    }
    float acc = 0.0f;
    for (int c0 = 0; c0 < nsteps; c0 += RING) {
#pragma unroll
        for (int cc = 0; cc < RING; ++cc) {
            const int c = c0 + cc;
            constexpr int TS = RESC_ROWS * RESC_TLD;
            const int nslot = (cc + 1) % RING;
            float* nt = tl + ((cc + 1) & 1) * TS;            // RING is even: step c + 1's buffer parity is static
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) *reinterpret_cast<f32x4*>(nt + (rg * 8 + lrow) * RESC_TLD + lcol) = reg[nslot][rg];
            {
                const int cn = c + 1 + RING < nsteps ? c + 1 + RING : nsteps - 1;
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) reg[nslot][rg] = *reinterpret_cast<const f32x4*>(src[rg] + cn * RESC_CH);
            }
            const float* mrow = tl + (cc & 1) * TS + l31 * RESC_TLD;
            const float* qk = qrow + c * RESC_CH;
            f32x4 gg[RESC_CH / 4], qq[RESC_CH / 4];
#pragma unroll
            for (int g4 = 0; g4 < RESC_CH / 4; ++g4) {
                gg[g4] = *reinterpret_cast<const f32x4*>(mrow + g4 * 4);
                qq[g4] = *reinterpret_cast<const f32x4*>(qk + g4 * 4);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this step's reads (and the next step's tile writes) are done
#pragma unroll
            for (int g8 = 0; g8 < RESC_CH / 8; ++g8) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc = __builtin_fmaf(qq[2 * g8][e], gg[2 * g8][e], acc);
                    acc = __builtin_fmaf(qq[2 * g8 + 1][e], gg[2 * g8 + 1][e], acc);
                }
            }
        }
    }
    return acc;
}

// One round of one wave: the exact chains of surv[s0 .. s0 + 32) with the deepest ring D allows, stored as ranking keys keys[s0 ..].
__device__ __forceinline__ void rescore_keys(const unsigned* surv, int s0, int ns, const float* qrow, const float* gallery, int D, float* tl,
                                             unsigned long long* keys) {
    const int lane = threadIdx.x & 63, nsteps = D / RESC_CH;
    float acc;
    if (nsteps % 8 == 0) acc = rescore_rows<8>(surv, s0, ns, qrow, gallery, D, tl);
    else if (nsteps % 10 == 0) acc = rescore_rows<10>(surv, s0, ns, qrow, gallery, D, tl);      // D = 640 (RN50x4): 20 steps, 40 loads in flight
    else if (nsteps % 4 == 0) acc = rescore_rows<4>(surv, s0, ns, qrow, gallery, D, tl);
    else acc = rescore_rows<2>(surv, s0, ns, qrow, gallery, D, tl);
    if (lane < RESC_ROWS && s0 + lane < ns) keys[s0 + lane] = make_key(acc, surv[s0 + lane]);
}

}  // namespace fern

// fp32 MFMA GEMM for gfx950 (CDNA4): C[M,N] = A[M,K] * W[N,K]^T with fused epilogues.
//
// This is the workhorse of the encode -> fuse -> rank path: it replaces every nn.Linear /
// Conv2d(patch-embed) / cosine-similarity matmul the reference issues through cuBLAS/cuDNN
// (SURVEY.md 2.2 rows K1-K6, K8).  The reference evaluates in fp32, so the matrix cores are used
// through v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains, 64 FLOP/clk/SIMD = 157 TFLOP/s peak).
//
// Tiling (wave64, 4 waves per workgroup):
//   * block tile BM x BN x 32, each wave owns a (BM/WAVES_M) x (BN/WAVES_N) sub-tile made of 32x32 MFMA tiles;
//   * A and W tiles are staged global -> registers -> LDS (16-byte loads, issue-early / write-late so the
//     next tile's HBM/L2 latency hides under the current tile's ~4k MFMA cycles);
//   * LDS rows are padded to 36 floats: every ds_read_b128 of an operand fragment is conflict-free
//     (16-lane groups hit 16 distinct 4-bank slots) and stays 16-byte aligned;
//   * the k index inside a 32-wide tile is permuted (lane half h reads k = 8*kk + 4*h + j) so that one
//     ds_read_b128 feeds four MFMAs; both operands use the same permutation, so the sum is unchanged;
//   * workgroup ids are remapped so that each XCD (private L2) owns a contiguous run of tiles.
#include "kernels.h"
#include "gemm_tile.h"
#include "gemm_tuner.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace fern {

// BM x BN block tile, WM x WN per wave (multiples of 32), BKT-wide k tiles, optional LDS double buffering.
template <int BM, int BN, int WM, int WN, int BKT, bool DBUF>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64) void gemm_f32_kernel(GemmParams p) {
    constexpr int WAVES_N = BN / WN;
    constexpr int WAVES_M = BM / WM;
    constexpr int NT = WAVES_M * WAVES_N * 64;          // threads per workgroup
    constexpr int LDS_S = BKT + 4;                      // padded row stride (floats): conflict-free ds_read_b128, 16-B aligned
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int C4 = BKT / 4;                         // float4 columns per k tile
    constexpr int RSTEP = NT / C4;                      // rows covered by one pass of all threads
    constexpr int AJ = BM / RSTEP, WJ = BN / RSTEP;     // float4 loads per thread per tile
    static_assert(BM % RSTEP == 0 && BN % RSTEP == 0, "tile rows must divide evenly over the threads");
    constexpr int NBUF = DBUF ? 2 : 1;

    __shared__ __attribute__((aligned(16))) float As[NBUF][BM * LDS_S];
    __shared__ __attribute__((aligned(16))) float Ws[NBUF][BN * LDS_S];
    if (p.gate && *p.gate == 0) return;
    int kbeg = 0, klen = p.K;
    if (p.ksplit > 1) {      // split-K slice: raw accumulators to kpart[slice]
        klen = p.K / p.ksplit;
        kbeg = blockIdx.y * klen;
        p.C = p.kpart + (long)blockIdx.y * p.M * p.N; p.ldc = p.N; p.epi = EPI_BIAS; p.bias = nullptr;
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int l31 = lane & 31, lh = lane >> 5;

    const TileAt at = tile_at<BM, BN>(blockIdx.x, p.M, p.N);
    const int bm = at.bm, bn = at.bn, nbn = at.nbn;

    // ---- per-thread staging coordinates ----
    const int c4 = tid % C4;     // float4 column inside the k tile
    const int r0 = tid / C4;
    const float* a_base[AJ];
    const float* w_base[WJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        const int row = clamp_row(bm * BM + r0 + RSTEP * j, p.M);
        if (p.aload == ALOAD_IM2COL) {
            const int g2 = p.grid * p.grid;
            const int b = row / g2, pr = row % g2;
            const int py = pr / p.grid, px = pr % p.grid;
            a_base[j] = p.A + ((long)b * 3 * p.img + (long)py * p.patch) * p.img + (long)px * p.patch;
        } else {
            a_base[j] = p.A + (long)row * p.lda;
        }
    }
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
        const int row = clamp_row(bn * BN + r0 + RSTEP * j, p.N);
        w_base[j] = p.W + sample_row(row, p.w_sample) * p.ldw;
    }

    f32x4 a_stage[AJ], w_stage[WJ];
    auto stage_load = [&](int k0) {
        const int k = kbeg + k0 + c4 * 4;
        long a_off = k;
        if (p.aload == ALOAD_IM2COL) {
            const int pp = p.patch * p.patch;
            const int c = k / pp, rem = k % pp;
            const int ky = rem / p.patch, kx = rem % p.patch;
            a_off = ((long)c * p.img + ky) * p.img + kx;
        }
#pragma unroll
        for (int j = 0; j < AJ; ++j) a_stage[j] = *reinterpret_cast<const f32x4*>(a_base[j] + a_off);
#pragma unroll
        for (int j = 0; j < WJ; ++j) w_stage[j] = *reinterpret_cast<const f32x4*>(w_base[j] + k);
    };
    auto stage_write = [&](int buf) {
#pragma unroll
        for (int j = 0; j < AJ; ++j) *reinterpret_cast<f32x4*>(&As[buf][(r0 + RSTEP * j) * LDS_S + c4 * 4]) = a_stage[j];
#pragma unroll
        for (int j = 0; j < WJ; ++j) *reinterpret_cast<f32x4*>(&Ws[buf][(r0 + RSTEP * j) * LDS_S + c4 * 4]) = w_stage[j];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    auto compute = [&](int buf) {
#pragma unroll
        for (int kk = 0; kk < BKT / 8; ++kk) {
            f32x4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i] = *reinterpret_cast<const f32x4*>(&As[buf][(wm * WM + i * 32 + l31) * LDS_S + kk * 8 + 4 * lh]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bf[j] = *reinterpret_cast<const f32x4*>(&Ws[buf][(wn * WN + j * 32 + l31) * LDS_S + kk * 8 + 4 * lh]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
    };

    const int nk = klen / BKT;
    stage_load(0);
    stage_write(0);
    __syncthreads();

    if (DBUF) {
        // one barrier per k tile: tile kt+1 is written into the other buffer while other waves still compute on tile kt
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 1 < nk) stage_load((kt + 1) * BKT);
            compute(kt & 1);
            if (kt + 1 < nk) stage_write((kt + 1) & 1);
            __syncthreads();
        }
    } else {
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 1 < nk) stage_load((kt + 1) * BKT);   // in flight during the MFMA phase below
            compute(0);
            __syncthreads();
            if (kt + 1 < nk) {
                stage_write(0);
                __syncthreads();
            }
        }
    }

    gemm_epilogue<BM, BN, WM, WN, TM, TN, WAVES_N>(p, acc, bm, bn, nbn, wm, wn, l31, lh, tid);
}

// ---- LDS-DMA variant --------------------------------------------------------------------------------------------
// Same tiling, but A / W tiles go HBM/L2 -> LDS with global_load_lds_dwordx4 (no VGPR staging, no ds_write pass):
// 16-wide k tiles, double buffered, one barrier per tile.  One wave-instruction writes 64 lanes x 16 B = 1 KiB =
// 16 consecutive 64-byte tile rows, lane-linear, so the bank-conflict swizzle is applied on the per-lane SOURCE
// address: the 16-byte chunk c of tile row r is stored at chunk position c ^ ((r >> 2) & 3), and the fragment reads
// XOR the same value (conflict-free for the 16-lane groups of ds_read_b128).
// FILT: the cosine sweep of the fused top-K (EPI_TOPK_FILTER epilogue).  A separate instantiation with a looser register
// bound (MINW = 2): compiled into the general kernel, the filter epilogue made the 128-VGPR builds spill.
// The tile body is a device function of (parameters, linear tile id, LDS) so that one kernel can run tiles of several geometries
// (gemm_f32_mixed_kernel below); gemm_f32_glds_kernel is the one-geometry wrapper.
// SPLIT = 3: the "f32x3" arithmetic (FERN_PREC_F32X3) -- fp32 operands split into three bf16 planes in registers, six
// v_mfma_f32_32x32x16_bf16 per k pair of fp32 MFMAs (see the compute step below).
template <int BM, int BN, int WM, int WN, int BKT, bool CONV = false, int SYNC = 0 /* 0: wait+barrier free to sink below the tail MFMAs (fastest), 1: drain copy first, 2: pinned after all MFMAs */,
          int FILT = 0 /* 1: EPI_TOPK_FILTER epilogue, 2: EPI_RANK_COUNT epilogue */, int SPLIT = 0>
__device__ __forceinline__ void glds_tile(GemmParams p, const int bid, float* smem) {
    constexpr int WAVES_N = BN / WN;
    constexpr int WAVES_M = BM / WM;
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int ROWS = BM + BN;                        // A rows then W rows
    using TR = TileRows<BKT * 4>;                        // 64- or 128-byte tile rows
    constexpr int C4 = TR::C4, RPP = TR::RPP;
    constexpr int PIECES = ROWS / RPP;
    constexpr int PPW = (PIECES + NW - 1) / NW;          // pieces per wave per tile (the last ones may not exist: guarded, wave-uniform)

    constexpr int TILE = ROWS * BKT;                     // floats per buffer; smem holds two
    int kbeg = 0, klen = p.K;
    if (p.ksplit > 1) {      // split-K slice: raw accumulators to kpart[slice]
        klen = p.K / p.ksplit;
        kbeg = blockIdx.y * klen;
        p.C = p.kpart + (long)blockIdx.y * p.M * p.N; p.ldc = p.N; p.epi = EPI_BIAS; p.bias = nullptr;
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int l31 = lane & 31, lh = lane >> 5;

    const TileAt at = tile_at<BM, BN>(bid, p.M, p.N);
    int bm = at.bm, bn = at.bn;
    const int nbn = at.nbn;
#ifdef FERN_GEMM_TRACE
    if (const int sw = p.packed >> 8) {        // probe: column stripes of `sw` tiles, rows fastest across a stripe's columns
        const int nbm = (p.M + BM - 1) / BM, swz = bm * nbn + bn;
        const int stripe = sw * nbm, nfull = nbn / sw;
        if (swz < nfull * stripe) { const int r = swz % stripe; bm = r / sw; bn = (swz / stripe) * sw + r % sw; }
        else { const int r = swz - nfull * stripe, w = nbn - nfull * sw; bm = r / w; bn = nfull * sw + r % w; }
    }
#endif

    // per-lane source row pointers (already offset by the swizzled 16-byte chunk) for this wave's pieces
    const float* src[PPW];
    int cb[PPW], cy[PPW], cx[PPW];                             // CONV: (image, y, x) of this lane's output pixel
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int piece = wave + NW * j;                       // wave-uniform
        const int trow = piece * RPP + lane / C4;              // row in the [A; W] tile-row space (BM, BN multiples of 32)
        const int chunk = TR::store_chunk(lane, trow);         // logical chunk stored at position lane % C4
        cb[j] = cy[j] = cx[j] = 0;
        if (trow < BM) {
            const int row = clamp_row(bm * BM + trow, p.M);
            if (CONV) {
                const int hw = p.conv_h * p.conv_w;
                cb[j] = row / hw;
                const int rem = row - cb[j] * hw;
                cy[j] = rem / p.conv_w;
                cx[j] = rem - cy[j] * p.conv_w;
                src[j] = p.A + chunk * 4;
            } else {
                src[j] = p.A + (long)row * p.lda + chunk * 4 + kbeg;
#ifdef FERN_GEMM_TRACE
                if (p.packed & 1) src[j] = p.A + (long)row * 16 + chunk * 4;
#endif
            }
        } else {
            const int row = clamp_row(bn * BN + (trow - BM), p.N);
            src[j] = p.W + sample_row(row, p.w_sample) * p.ldw + chunk * 4 + kbeg;
#ifdef FERN_GEMM_TRACE
            if (p.packed & 1) src[j] = p.W + (long)row * 16 + chunk * 4;
#endif
        }
    }
    auto stage = [&](int buf, int k0) {
        int ky = 0, kx = 0, c0 = 0;
        if (CONV) {                                            // a 16/32-wide k tile lies inside one filter tap (conv_c % BKT == 0)
            const int tap = k0 / p.conv_c;
            c0 = k0 - tap * p.conv_c;
            ky = tap / 3 - 1;
            kx = tap - (tap / 3) * 3 - 1;
        }
#pragma unroll
        for (int j = 0; j < PPW; ++j) {
            const int piece = wave + NW * j;
            if (PIECES % NW != 0 && piece >= PIECES) continue;   // wave-uniform: this wave has no j-th piece (tile rows do not divide over the waves)
            const float* g = src[j] + k0;
#ifdef FERN_GEMM_TRACE
            if (p.packed & 1) g = src[j] + (long)(k0 / 16) * 16 * (piece * RPP < BM ? p.M : p.N);
#endif
            if (CONV && piece * RPP < BM) {                    // wave-uniform: this piece holds A (activation) rows
                const int yy = cy[j] + ky, xx = cx[j] + kx;
                const bool inside = yy >= 0 && yy < p.conv_h && xx >= 0 && xx < p.conv_w;
                g = inside ? src[j] + (((long)cb[j] * p.conv_h + yy) * p.conv_w + xx) * p.conv_c + c0 : p.zeros + (lane & 3) * 4;
            }
            lds_dma16(g, smem + buf * TILE + piece * 256);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int sw = TR::read_swizzle(l31);                       // read-side swizzle of this lane's rows
    // f32x3 (SPLIT = 3): fp32 operands split IN REGISTERS, after the LDS read, into three bf16 planes by truncation (x1 = top 16
    // bits of x -- one v_perm_b32 packs two --, r1 = x - x1 exactly, x2 = top 16 bits of r1, ...: 8 + 8 + 8 mantissa bits), the six
    // products of total order <= 4 on v_mfma_f32_32x32x16_bf16 (32 cycles each against two 64-cycle fp32 MFMAs).  The two 8-groups
    // of a 16-k tile supply the 8 k values a lane feeds to one bf16 MFMA (same k -> slot map for both operands).  The error against
    // exact arithmetic is the fp32 kernel's own (measured 1.7-2.3e-6 of the output rms against 2.0e-6), at 1.4-1.5x its speed; it
    // is NOT the fp32 fma chain, so nothing that must be bit-identical to the sweep's scores may use it.  Every configuration walks
    // k in the same order with the same six products: results are bit-identical across tile shapes and batch-invariant.
    constexpr int NPL = SPLIT > 0 ? SPLIT : 1;
    auto compute_split = [&](int buf) {
        static_assert(SPLIT == 0 || BKT == 16, "the split form pairs the two 8-groups of a 16-k tile");
        const float* As = smem + buf * TILE;
        const float* Ws = As + BM * BKT;
        bf16x8 ap[TM][NPL], bp[TN][NPL];
        const int pc0 = ((0 + lh) ^ sw) * 4, pc1 = ((2 + lh) ^ sw) * 4;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float* r = &As[(wm * WM + i * 32 + l31) * BKT];
            split_bf16_planes<NPL>(*reinterpret_cast<const f32x4*>(r + pc0), *reinterpret_cast<const f32x4*>(r + pc1), ap[i]);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const float* r = &Ws[(wn * WN + j * 32 + l31) * BKT];
            split_bf16_planes<NPL>(*reinterpret_cast<const f32x4*>(r + pc0), *reinterpret_cast<const f32x4*>(r + pc1), bp[j]);
        }
        // products in order of the planes they need -- a1 b1 | a1 b2, a2 b1 | a2 b2, a1 b3, a3 b1 -- so that the VALU work of the
        // deeper planes can run under the MFMAs of the shallower ones (left to hipcc's scheduler: pinning 1 MFMA : 6 VALU groups with
        // sched_group_barrier was measured and changed nothing on the 128x128 tile, -4 % on the fat-wave macro-tile)
#pragma unroll
        for (int ord = 0; ord < NPL; ++ord)
#pragma unroll
            for (int la = 0; la <= ord; ++la)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[i][la], bp[j][ord - la], acc[i][j], 0, 0, 0);
    };
    auto compute_fp32 = [&](int buf) {
        const float* As = smem + buf * TILE;
        const float* Ws = As + BM * BKT;
#pragma unroll
        for (int kk = 0; kk < BKT / 8; ++kk) {
            const int pc = ((2 * kk + lh) ^ sw) * 4;            // physical position of logical chunk 2kk + half
            f32x4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4*>(&As[(wm * WM + i * 32 + l31) * BKT + pc]);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(&Ws[(wn * WN + j * 32 + l31) * BKT + pc]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
    };
    auto compute = [&](int buf) {
        if constexpr (SPLIT > 0) compute_split(buf);
        else compute_fp32(buf);
    };

    // LDS-DMA data is published by the issuing wave's vmcnt wait followed by a barrier.  The copy of tile kt+1 overlaps the
    // fragment reads and MFMAs of tile kt; hipcc is left free to sink the wait + barrier below the last fragment read, so a
    // wave still has ~16 register-only MFMAs to issue while it waits at the barrier and for the next tile's first reads
    // (A/B on MI355X: +3..6 % over draining the copy first, +6 % over pinning the barrier after all MFMAs).
    const int nk = klen / BKT;
#ifdef FERN_GEMM_TRACE
    long long* tr = p.trace ? p.trace + ((long)blockIdx.x * NW + wave) * FERN_GEMM_TRACE_SLOTS : nullptr;
    int tslot = 4;
#define FERN_TRACE_MARK()                                                                         \
    do {                                                                                          \
        if (tr && lane == 0 && tslot < FERN_GEMM_TRACE_SLOTS) tr[tslot] = (long long)__builtin_readcyclecounter(); \
        ++tslot;                                                                                  \
    } while (0)
    if (tr && lane == 0) {
        tr[0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);       // HW_ID
        tr[1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);      // XCC_ID
        tr[2] = (long long)__builtin_amdgcn_s_memrealtime();
    }
#else
#define FERN_TRACE_MARK() do {} while (0)
#endif
    FERN_TRACE_MARK();
    stage(0, 0);
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    FERN_TRACE_MARK();
    // Waves inside the main loop outrank co-resident waves that are in their prologue or epilogue: the epilogue is a few thousand
    // VALU issue slots (GELU: ~20 per element), and VALU and MFMA share the issue port -- at equal priority another workgroup's
    // epilogue delays this wave's next MFMA.  One switch per tile (round 2 toggled the priority around every 16-MFMA cluster and lost
    // 6 %: that disturbs the arbitration between waves that are all in their loops).  A/B on one box, 12608x3072x768 + GELU:
    // 112.4 -> 115.7 TFLOP/s (128x128 tiles), 115.2 -> 117.8 (macro-tiles); shapes with a plain epilogue are unchanged.
    __builtin_amdgcn_s_setprio(2);
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) stage((kt + 1) & 1, (kt + 1) * BKT);   // the other buffer is free: every wave passed the last barrier
        if (SYNC == 1) wait_vmcnt<0>();   // A/B variant: drain the copy before computing
        compute(kt & 1);
        if (SYNC == 2) __builtin_amdgcn_sched_barrier(0);
#ifdef FERN_GEMM_TRACE_PHASES      // three stamps per k tile: MFMAs issued | own DMA landed | barrier passed (pins the order: attribution only)
        __builtin_amdgcn_sched_barrier(0);
        FERN_TRACE_MARK();
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        FERN_TRACE_MARK();
#else
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // my DMA pieces landed, my fragment reads are done
#endif
        __builtin_amdgcn_s_barrier();
        FERN_TRACE_MARK();
    }
    __builtin_amdgcn_s_setprio(0);
    if (FILT == 2) rank_count_epilogue<BM, BN, WM, WN, TM, TN>(p, acc, bm, bn, wm, wn, l31, lh, smem);
    else if (FILT) filter_epilogue<BM, BN, WM, WN, TM, TN>(p, acc, bm, bn, wm, wn, l31, lh);
    else gemm_epilogue<BM, BN, WM, WN, TM, TN, WAVES_N>(p, acc, bm, bn, nbn, wm, wn, l31, lh, tid);
#ifdef FERN_GEMM_TRACE
    wait_vmcnt<0>();
    FERN_TRACE_MARK();
    if (tr && lane == 0) tr[3] = (long long)__builtin_amdgcn_s_memrealtime();
#endif
}

// ONE __shared__ object per kernel: with a second LDS object next to the DMA destination hipcc drains the DMA (s_waitcnt vmcnt(0))
// before the first ds_read of every k step, which serialises the copy and the MFMAs of a wave.
template <int BM, int BN, int WM, int WN, int BKT, int MINW, bool CONV = false, int SYNC = 0, int FILT = 0, int SPLIT = 0>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64, MINW) void gemm_f32_glds_kernel(GemmParams p) {
    __shared__ __attribute__((aligned(1024))) float smem[2 * (BM + BN) * BKT];
    if (p.gate && *p.gate == 0) return;
    glds_tile<BM, BN, WM, WN, BKT, CONV, SYNC, FILT, SPLIT>(p, blockIdx.x, smem);
}

// ---- f32x3 with the operands split ONCE per workgroup (round 4) ---------------------------------------------------------------
// In the SPLIT = 3 form above every wave splits the fragments it reads: on the 256x256 tile an A row block is split by four waves
// and a W row block by two, 216 split instructions per fat wave and 16-k tile, and the family is bound by the issue port, not by the
// MFMA pipe or the copy (profiles/r04_experiments.txt section 1).  Here the fp32 tile goes global -> registers (two 16-byte loads per
// (row, half) unit: chunks h and 2 + h, the 8 k values lane half h of that row feeds to one bf16 MFMA), is split by the thread that
// loaded it -- the same split(), so the same plane bits -- and the three bf16 planes are written to LDS, 16 bytes per unit and plane;
// every wave then reads ready fragments (ds_read_b128, conflict-free: a plane is [half][row][16 B]).  72 split instructions per wave
// and tile instead of 216, 18 fragment reads instead of 12.  Planes are double buffered: tile kt + 1 is split and published while
// the MFMAs of tile kt issue, tile kt + 2 is in flight in registers, one barrier per tile.  Same k -> slot map, same six products
// in the same order as the SPLIT = 3 form: bit-identical to every other configuration of the family.
// Wave tile 128x64 on (BM / 128) x (BN / 64) waves; two waves per SIMD of register budget.
template <int BM, int BN>
__global__ __launch_bounds__((BM / 128) * (BN / 64) * 64, 2) void gemm_f32x3_shared_kernel(GemmParams p) {
    constexpr int WM = 128, WN = 64, TM = 4, TN = 2;
    constexpr int WAVES_N = BN / WN, NW = (BM / WM) * WAVES_N, NT = NW * 64;
    constexpr int ROWS = BM + BN;                        // A rows then W rows
    constexpr int UNITS = ROWS * 2;                      // (row, half) units of a 16-k tile
    static_assert(UNITS % NT == 0, "units must divide over the threads");
    constexpr int UPT = UNITS / NT;
    constexpr int HALF = ROWS * 16 + 64;                 // bytes of one lane half of a plane (+ 64: the two halves of a row are written by neighbouring lanes -- different banks)
    constexpr int PLANE = 2 * HALF;
    constexpr int BUF = 3 * PLANE;
    __shared__ __attribute__((aligned(1024))) char smem[2 * BUF];
    if (p.gate && *p.gate == 0) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int l31 = lane & 31, lh = lane >> 5;
    const TileAt at = tile_at<BM, BN>(blockIdx.x, p.M, p.N);
    const int bm = at.bm, bn = at.bn, nbn = at.nbn;

    const float* src[UPT];
    int dst[UPT];
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
        const int unit = tid + NT * u;
        const int trow = unit >> 1, h = unit & 1;
        if (trow < BM) {
            src[u] = p.A + (long)clamp_row(bm * BM + trow, p.M) * p.lda + h * 4;
        } else {
            src[u] = p.W + (long)clamp_row(bn * BN + (trow - BM), p.N) * p.ldw + h * 4;
        }
        dst[u] = h * HALF + trow * 16;
    }
    // two register sets: the tile published in step kt was requested two steps earlier (a step is ~1.5 us: an HBM miss has landed)
    f32x4 g[2][UPT][2];
    const int klast = p.K - 16;
    auto load = [&](f32x4 (&gs)[UPT][2], int k0) {
        k0 = k0 < klast ? k0 : klast;                      // past the end: re-read the last tile (published, never multiplied): no branch in the loop
#pragma unroll
        for (int u = 0; u < UPT; ++u) {
            gs[u][0] = *reinterpret_cast<const f32x4*>(src[u] + k0);
            gs[u][1] = *reinterpret_cast<const f32x4*>(src[u] + k0 + 8);
        }
    };
    auto publish = [&](const f32x4 (&gs)[UPT][2], int buf) {
#pragma unroll
        for (int u = 0; u < UPT; ++u) {
            bf16x8 pl[3];
            split_bf16_planes<3>(gs[u][0], gs[u][1], pl);      // glds_tile's split: the same plane bits
#pragma unroll
            for (int lv = 0; lv < 3; ++lv) *reinterpret_cast<bf16x8*>(smem + buf * BUF + lv * PLANE + dst[u]) = pl[lv];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int arow = lh * HALF + (wm * WM + l31) * 16, wrow = lh * HALF + (BM + wn * WN + l31) * 16;
    auto compute = [&](int buf) {
        const char* P = smem + buf * BUF;
        bf16x8 ap[TM][3], bp[TN][3];
#pragma unroll
        for (int lv = 0; lv < 3; ++lv) {
#pragma unroll
            for (int i = 0; i < TM; ++i) ap[i][lv] = *reinterpret_cast<const bf16x8*>(P + lv * PLANE + arow + i * 512);
#pragma unroll
            for (int j = 0; j < TN; ++j) bp[j][lv] = *reinterpret_cast<const bf16x8*>(P + lv * PLANE + wrow + j * 512);
        }
#pragma unroll
        for (int ord = 0; ord < 3; ++ord)
#pragma unroll
            for (int la = 0; la <= ord; ++la)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[i][la], bp[j][ord - la], acc[i][j], 0, 0, 0);
    };

    const int nk = p.K / 16;
    load(g[0], 0);
    publish(g[0], 0);
    load(g[1], 16);
    load(g[0], 32);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_s_setprio(2);
    // step kt (parity P): MFMAs on plane buffer P; tile kt + 1 (register set P ^ 1) is split and published into buffer P ^ 1 -- free:
    // every wave passed the last barrier -- and that register set is refilled with tile kt + 3.  Straight-line code: the split
    // instructions interleave with the MFMAs.
    auto step = [&](int kt, auto parity) {
        constexpr int P = decltype(parity)::value;
        compute(P);
        publish(g[P ^ 1], P ^ 1);
        load(g[P ^ 1], (kt + 3) * 16);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // my fragment reads and my plane writes are done
        __builtin_amdgcn_s_barrier();
    };
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        step(kt, std::integral_constant<int, 0>{});
        step(kt + 1, std::integral_constant<int, 1>{});
    }
    if (kt < nk) step(kt, std::integral_constant<int, 0>{});
    __builtin_amdgcn_s_setprio(0);
    gemm_epilogue<BM, BN, WM, WN, TM, TN, WAVES_N>(p, acc, bm, bn, nbn, wm, wn, l31, lh, tid);
}

// ---- mixed-geometry launch ------------------------------------------------------------------------------------------------
// The 8-wave 256x128 (or 128x256) macro-tile has the best main loop of the family (0.75x the L2 -> LDS bytes per flop of the
// 128x128 tile: 126-128 TFLOP/s against 121 on a shape both tile evenly, tools/probe/gemm_timeline.hip), but the encoder's GEMMs are
// only 3.5-9 macro-tiles per CU deep, so whole-matrix macro-tiling loses more to the ragged last round than it gains.  Here ONE
// launch covers the rows in three bands, big tiles first:  rows [0, ra) in macro-tiles, [ra, rb) in 128x128 tiles, [rb, M) in
// 64x128 tiles -- all on 8 waves (wave tiles 64x64 / 64x32 / 32x32), every band with its own XCD-aware tile order.  The hardware
// dispatcher hands out workgroups in block order, so the small tiles back-fill the CUs as the macro-tiles drain instead of waiting
// behind a kernel boundary (the two-launch bulk + remainder plan serialises there).  Every geometry accumulates each output over k
// in the same order: results are bit-identical to every other configuration, and the bands can be cut at any row.
// SPLIT = 3 (f32x3 family): the same three bands on FOUR waves -- macro-tile on fat waves (wave tile 128x64 / 64x128: the bf16
// planes need the registers of two waves per SIMD), 128x128 and 64x128 on 64x64 / 32x64 wave tiles.
template <bool WIDE, int SPLIT = 0>
__global__ __launch_bounds__(SPLIT ? 256 : 512, SPLIT ? 2 : 4) void gemm_f32_mixed_kernel(GemmParams p, int ra, int rb, int n_a8, int n_b8) {
    __shared__ __attribute__((aligned(1024))) float smem[2 * 384 * 16];
    const int bid = blockIdx.x;
    auto band = [&](int row0, int rows) {      // the rows [row0, row0 + rows) as a GEMM of their own (plain, row-independent epilogues only)
        GemmParams q = p;
        q.A = p.A + (long)row0 * p.lda;
        q.C = p.C + (long)row0 * p.ldc;
        if (p.R) q.R = p.R + (long)row0 * p.ldc;
        q.M = rows;
        return q;
    };
    constexpr int BMA = WIDE ? 128 : 256, BNA = WIDE ? 256 : 128;
    constexpr int WMA = SPLIT ? BMA / 2 : 64, WNA = SPLIT ? BNA / 2 : 64;      // 2 x 2 fat waves, or 8 waves of 64x64
    if (bid < n_a8) {
        const int tiles = (ra / BMA) * ((p.N + BNA - 1) / BNA);
        if (bid < tiles) glds_tile<BMA, BNA, WMA, WNA, 16, false, 0, 0, SPLIT>(band(0, ra), bid, smem);
    } else if (bid < n_a8 + n_b8) {
        const int tiles = ((rb - ra + 127) / 128) * ((p.N + 127) / 128);
        if (bid - n_a8 < tiles) glds_tile<128, 128, 64, SPLIT ? 64 : 32, 16, false, 0, 0, SPLIT>(band(ra, rb - ra), bid - n_a8, smem);
    } else {
        glds_tile<64, 128, 32, SPLIT ? 64 : 32, 16, false, 0, 0, SPLIT>(band(rb, p.M - rb), bid - n_a8 - n_b8, smem);
    }
}

// ---- two GEMMs in one launch (round 6) ------------------------------------------------------------------------
// The text tower's GEMMs (M = 77 B = 4 928 rows, K = 512) are a few hundred small tiles each: on their own they run at 84-119 TFLOP/s
// (2.4 rounds of 64x64 tiles on 256 CUs) while the image tower's GEMM of the same layer runs at 117-128.  The two towers are
// independent until the fusion, so the text layer's GEMM rides in the SAME launch as the image layer's GEMM of the same kind: the first
// problem keeps the mixed plan the tuner chose for it (macro-tiles, 128x128, 64x128 bands), the second problem follows as two more bands
// (128x128 tiles, then 64x128 for the ragged rows) -- the dispatcher hands out its workgroups as the first problem's tail drains, so
// its tiles back-fill CUs that would otherwise idle behind a kernel boundary.  Same tiles, same k order: bit-identical to two launches.
template <bool WIDE, int SPLIT = 0>
__global__ __launch_bounds__(SPLIT ? 256 : 512, SPLIT ? 2 : 4) void gemm_f32_pair_kernel(GemmParams p, int ra, int rb, int n_a8, int n_b8, int n_c8, GemmParams p2,
                                                                                        int rb2, int n_d8) {
    __shared__ __attribute__((aligned(1024))) float smem[2 * 384 * 16];
    const int bid = blockIdx.x;
    auto band = [&](const GemmParams& g, int row0, int rows) {
        GemmParams q = g;
        q.A = g.A + (long)row0 * g.lda;
        q.C = g.C + (long)row0 * g.ldc;
        if (g.R) q.R = g.R + (long)row0 * g.ldc;
        q.M = rows;
        return q;
    };
    constexpr int BMA = WIDE ? 128 : 256, BNA = WIDE ? 256 : 128;
    constexpr int WMA = SPLIT ? BMA / 2 : 64, WNA = SPLIT ? BNA / 2 : 64;
    constexpr int WNS = SPLIT ? 64 : 32;                  // wave tile width of the 128x128 and 64x128 bands (8 waves, or 4 for the split family)
    // block order: the SECOND problem's bands first (its 128x128 tiles, then its ragged 64x128 rows), then the first problem's bands in the
    // order its plan was tuned for -- so that the launch still ends in the first problem's own small-tile band (appended BEHIND it, the second
    // problem's few hundred long-k tiles were the new tail: 12608 x 768 x 3072 + 4928 x 512 x 2048 ran at 112.6 TFLOP/s against 119.9 as two
    // launches)
    const int n_e8 = (((p2.M - rb2 + 63) / 64) * ((p2.N + 127) / 128) + 7) & ~7;
    const int n2 = n_d8 + n_e8;
    if (bid < n_d8) {
        const int tiles = (rb2 / 128) * ((p2.N + 127) / 128);
        if (bid < tiles) glds_tile<128, 128, 64, WNS, 16, false, 0, 0, SPLIT>(band(p2, 0, rb2), bid, smem);
    } else if (bid < n2) {
        const int tiles = ((p2.M - rb2 + 63) / 64) * ((p2.N + 127) / 128);
        if (bid - n_d8 < tiles) glds_tile<64, 128, 32, WNS, 16, false, 0, 0, SPLIT>(band(p2, rb2, p2.M - rb2), bid - n_d8, smem);
    } else if (bid - n2 < n_a8) {
        const int b1 = bid - n2;
        const int tiles = (ra / BMA) * ((p.N + BNA - 1) / BNA);
        if (b1 < tiles) glds_tile<BMA, BNA, WMA, WNA, 16, false, 0, 0, SPLIT>(band(p, 0, ra), b1, smem);
    } else if (bid - n2 < n_a8 + n_b8) {
        const int b1 = bid - n2 - n_a8;
        const int tiles = ((rb - ra + 127) / 128) * ((p.N + 127) / 128);
        if (b1 < tiles) glds_tile<128, 128, 64, WNS, 16, false, 0, 0, SPLIT>(band(p, ra, rb - ra), b1, smem);
    } else {
        glds_tile<64, 128, 32, WNS, 16, false, 0, 0, SPLIT>(band(p, rb, p.M - rb), bid - n2 - n_a8 - n_b8, smem);
    }
    (void)n_c8;
}

// ---- small-M variant on v_mfma_f32_16x16x4_f32 ----------------------------------------------------------------------
// The fusion stage is a chain of M = 64 GEMMs (combiner MLPs, class-row chain of the last ViT block): a 32x32 MFMA tile has
// to walk its whole k chain on one SIMD (K = 4096: 2048 dependent-pipe MFMAs of 64 cycles = 57 us) and there are only
// M/32 x N/32 tiles to spread.  A 16x16 tile has a 4x shorter chain per output and 4x as many tiles.  Both fp32 MFMAs are exact
// sequential fmaf chains over their k slots (tools/probe/mfma16_probe.hip), so with the slot -> k assignment below this kernel
// adds every output element's products in the SAME order as the 32x32 kernels (per 8-group g: 8g, 8g+4, 8g+1, 8g+5, 8g+2,
// 8g+6, 8g+3, 8g+7) and is bit-identical to them: lane (row/col l & 15, slot q = l >> 4) feeds k = 8g + 2m + 4(q & 1) + (q >> 1)
// to MFMA m = 0, 1 of group g.  Workgroup = 64 rows x 32 columns, wave = 16 rows x two 16-column tiles (the 32-column group of
// the reduce epilogues); tiles arrive by LDS-DMA through a 5-stage ring of 64-float (256-byte) rows.
typedef float f32x4v __attribute__((ext_vector_type(4)));

template <int STAGES, int BKT>
__global__ __launch_bounds__(256) void gemm_f32_skinny_kernel(GemmParams p) {
    constexpr int BM = 64, BN = 32, NW = 4;
    constexpr int ROWS = BM + BN;                        // A rows then W rows
    constexpr int C4 = BKT / 4;                          // 16-byte chunks per tile row (8 or 16)
    constexpr int RPP = 64 / C4;                         // tile rows per 1 KiB piece
    constexpr int PIECES = ROWS / RPP;
    constexpr int PPW = PIECES / NW;
    constexpr int TILE = ROWS * BKT;                     // floats per stage
    __shared__ __attribute__((aligned(1024))) float smem[STAGES * TILE];
    if (p.gate && *p.gate == 0) return;
    int kbeg = 0, klen = p.K;
    if (p.ksplit > 1) {      // split-K slice: raw accumulators to kpart[slice]
        klen = p.K / p.ksplit;
        kbeg = blockIdx.y * klen;
        p.C = p.kpart + (long)blockIdx.y * p.M * p.N; p.ldc = p.N; p.epi = EPI_BIAS; p.bias = nullptr;
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    const int nbn = (p.N + BN - 1) / BN;
    const int bm = blockIdx.x / nbn, bn = blockIdx.x % nbn;

    const float* src[PPW];
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int piece = wave + NW * j;
        const int trow = piece * RPP + lane / C4;
        // 16-byte chunk c of row r lives at position c ^ f(r); f makes every ds_read_b128 group hit 16 distinct bank quads
        const int chunk = (lane & (C4 - 1)) ^ (BKT == 32 ? ((trow >> 1) & 7) : (trow & 15));
        if (trow < BM) {
            src[j] = p.A + (long)clamp_row(bm * BM + trow, p.M) * p.lda + chunk * 4 + kbeg;
        } else {
            src[j] = p.W + sample_row(clamp_row(bn * BN + (trow - BM), p.N), p.w_sample) * p.ldw + chunk * 4 + kbeg;
        }
    }
    auto stage = [&](int buf, int k0) {
#pragma unroll
        for (int j = 0; j < PPW; ++j)
            lds_dma16(src[j] + k0, smem + buf * TILE + (wave + NW * j) * 256);
    };

    f32x4v acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    // per-lane row offsets (floats) and swizzles of the three fragment rows: A row, W rows of the two column tiles
    const int ra = wave * 16 + r16, rb0 = BM + r16, rb1 = BM + 16 + r16;
    const int sa = BKT == 32 ? (ra >> 1) & 7 : ra & 15, sb0 = BKT == 32 ? (rb0 >> 1) & 7 : rb0 & 15, sb1 = BKT == 32 ? (rb1 >> 1) & 7 : rb1 & 15;
    const int w0 = q >> 1;                                   // word inside the 16-byte chunk (MFMA 0); MFMA 1 uses w0 + 2
    auto compute = [&](int buf) {
        const float* T = smem + buf * TILE;
#pragma unroll
        for (int g = 0; g < BKT / 8; ++g) {
            const int c = 2 * g + (q & 1);                   // logical chunk holding k = 8g + 4(q&1) .. +3
            // whole 16-byte chunks (conflict-free ds_read_b128: the 16 lanes of a read group sit on 16 distinct
            // (row parity, chunk position) pairs); the lane then keeps words w0 and w0 + 2.  Single-word reads would be
            // 4-way bank conflicted (128-byte rows: a word's bank is its position in the row) and made the kernel LDS-bound.
            const f32x4v va = *reinterpret_cast<const f32x4v*>(T + ra * BKT + ((c ^ sa) << 2));
            const f32x4v vb0 = *reinterpret_cast<const f32x4v*>(T + rb0 * BKT + ((c ^ sb0) << 2));
            const f32x4v vb1 = *reinterpret_cast<const f32x4v*>(T + rb1 * BKT + ((c ^ sb1) << 2));
            const float a0 = w0 ? va[1] : va[0], a1 = w0 ? va[3] : va[2];
            const float b00 = w0 ? vb0[1] : vb0[0], b01 = w0 ? vb0[3] : vb0[2];
            const float b10 = w0 ? vb1[1] : vb1[0], b11 = w0 ? vb1[3] : vb1[2];
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b00, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b10, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b01, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b11, acc[1], 0, 0, 0);
        }
    };

    const int nk = klen / BKT;
#pragma unroll
    for (int t = 0; t < STAGES - 1; ++t)
        if (t < nk) stage(t, t * BKT);
    int slot = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + STAGES - 2 < nk) wait_vmcnt<PPW * (STAGES - 2)>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (kt + STAGES - 1 < nk) {
            int fill = slot + STAGES - 1;
            fill = fill >= STAGES ? fill - STAGES : fill;
            stage(fill, (kt + STAGES - 1) * BKT);
        }
        compute(slot);
        slot = slot + 1 == STAGES ? 0 : slot + 1;
    }

    // ---- epilogue: C/D map of the 16x16 MFMA: col = lane & 15, row = 4 * (lane >> 4) + r.  Same arithmetic, element by element,
    // as gemm_epilogue.h (bit-identical outputs); the reduce form adds the two column tiles first (the xor-16 step of the
    // 32-lane tree of the 32x32 kernels), then the xor 8, 4, 2, 1 steps inside the 16-lane group.
    const int row0 = bm * BM + wave * 16 + 4 * q;
    if (p.epi == EPI_RELU_DOT) {
        const int ng = (p.N + 31) / 32;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int col = bn * BN + t * 16 + r16;
                v[t] = col < p.N ? fmaxf(acc[t][r] + p.bias[col], 0.0f) * p.aux0[col] : 0.0f;
            }
            float sum = v[0] + v[1];
            sum += __shfl_xor(sum, 8);
            sum += __shfl_xor(sum, 4);
            sum += __shfl_xor(sum, 2);
            sum += __shfl_xor(sum, 1);
            const int row = row0 + r;
            if (r16 == 0 && row < p.M) p.partial[(long)row * ng + bn] = sum;
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int col = bn * BN + t * 16 + r16;
        if (col >= p.N) continue;
        const float bia = p.bias ? p.bias[col] : 0.0f;
        float sc = 1.0f, sh = 0.0f;
        if (p.epi == EPI_COLAFFINE_TANH) { sc = p.aux0[col]; sh = p.aux1[col]; }
        float add[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.epi == EPI_BIAS_RESIDUAL || p.epi == EPI_BIAS_RESIDUAL_RELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (row0 + r < p.M) add[r] = p.R[(long)(row0 + r) * p.ldc + col];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (row0 + r >= p.M) continue;
            float v = acc[t][r] + bia;
            switch (p.epi) {
                case EPI_BIAS_GELU: v = gelu_erf2(f32x2{v, v})[0]; break;      // the 32x32 kernels' arithmetic, bit for bit
                case EPI_BIAS_QUICKGELU: v = quick_gelu2(f32x2{v, v})[0]; break;
                case EPI_BIAS_RELU: v = fmaxf(v, 0.0f); break;
                case EPI_BIAS_RESIDUAL: v += add[r]; break;
                case EPI_BIAS_RESIDUAL_RELU: v = fmaxf(v + add[r], 0.0f); break;
                case EPI_COLAFFINE_TANH: v = tanhf(v * sc + sh); break;
                default: break;
            }
            p.C[(long)(row0 + r) * p.ldc + col] = v;
        }
    }
}

static bool epi_is_sweep(int e) { return e == EPI_TOPK_FILTER || e == EPI_RANK_COUNT; }      // nothing stored: the four LDS-DMA tiles with their own epilogues

static int best_of(int M, int N, int first, int last) {
    int best = first;
    double best_cost = 1e300;
    for (int c = first; c < last; ++c) {
        const long nb = (long)((M + kCfgs[c].bm - 1) / kCfgs[c].bm) * ((N + kCfgs[c].bn - 1) / kCfgs[c].bn);
        const double cost = (double)((nb + 255) / 256) * kCfgs[c].bm * kCfgs[c].bn / kCfgs[c].eff;
        if (cost < best_cost * 0.999) { best_cost = cost; best = c; }
    }
    return best;
}

// Heuristic (used as is for the reduce epilogues and as the fallback of the tuner): large problems stream their tiles
// with LDS-DMA (configs 8-11: more resident waves, no ds_write pass); small-M problems are latency-bound per block and
// do better with the register-prefetched 32-wide k tiles (configs 0-3).
static int choose_cfg(int M, int N, int K) {
    const int f = forced_cfg(FAM_F32);
    if (cfg_fits(FAM_F32, f, K)) return f;
    if (f >= 100) return best_of(M, N, 8, 12);
    return (M >= 1024 || (K & 31)) ? best_of(M, N, 8, 12) : best_of(M, N, 0, kNumAuto);   // K % 32 != 0: only the 16-wide k tiles fit
}

// Partial sums per row written by the reduce epilogues: one per 32-column group, whatever tile configuration runs.
int gemm_num_col_blocks(int M, int N, int K) {
    (void)M; (void)K;
    return (N + 31) / 32;
}

// configurations 8-11 (the four LDS-DMA tile geometries) of one variant of gemm_f32_glds_kernel; false: c is none of them
template <int MINW, bool CONV, int FILT>
static bool launch_glds_8_11(int c, dim3 grid, const GemmParams& p, hipStream_t s) {
    switch (c) {
        case 8: FERN_LAUNCH((gemm_f32_glds_kernel<128, 128, 64, 64, 16, MINW, CONV, 0, FILT>), grid, dim3(256), 0, s, p); return true;
        case 9: FERN_LAUNCH((gemm_f32_glds_kernel<64, 128, 32, 64, 16, MINW, CONV, 0, FILT>), grid, dim3(256), 0, s, p); return true;
        case 10: FERN_LAUNCH((gemm_f32_glds_kernel<128, 64, 64, 32, 16, MINW, CONV, 0, FILT>), grid, dim3(256), 0, s, p); return true;
        case 11: FERN_LAUNCH((gemm_f32_glds_kernel<64, 64, 32, 32, 16, MINW, CONV, 0, FILT>), grid, dim3(256), 0, s, p); return true;
        default: return false;
    }
}
static hipError_t launch_cfg(int c, const GemmParams& p, hipStream_t s) {
    const int nb = tile_blocks(kCfgs[c].bm, kCfgs[c].bn, p);
    const int ks = p.ksplit > 1 ? p.ksplit : 1;
    const dim3 grid(nb, ks);
    if (p.epi == EPI_TOPK_FILTER) {      // the filtered sweep: LDS-DMA family, own instantiations
        if (p.aload != ALOAD_PLAIN || !launch_glds_8_11<2, false, 1>(c, grid, p, s)) return hipErrorInvalidValue;
        return hipGetLastError();
    }
    if (p.epi == EPI_RANK_COUNT) {      // the counting sweep of the exact target ranks: the same four tiles, counting epilogue
        if (p.aload != ALOAD_PLAIN || ks != 1 || !launch_glds_8_11<2, false, 2>(c, grid, p, s)) return hipErrorInvalidValue;
        return hipGetLastError();
    }
    if (p.aload == ALOAD_CONV3) {      // 3x3 window loader exists for the LDS-DMA family only
        if (launch_glds_8_11<4, true, 0>(c, grid, p, s)) return hipGetLastError();
        switch (c) {
            case 14: FERN_LAUNCH((gemm_f32_glds_kernel<128, 96, 32, 96, 16, 4, true>), grid, dim3(256), 0, s, p); break;
            case 15: FERN_LAUNCH((gemm_f32_glds_kernel<128, 160, 32, 160, 16, 3, true>), grid, dim3(256), 0, s, p); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (c) {
        case 0: FERN_LAUNCH((gemm_f32_kernel<128, 128, 64, 64, 32, false>), grid, dim3(256), 0, s, p); break;
        case 1: FERN_LAUNCH((gemm_f32_kernel<64, 128, 32, 64, 32, false>), grid, dim3(256), 0, s, p); break;
        case 2: FERN_LAUNCH((gemm_f32_kernel<128, 64, 64, 32, 32, false>), grid, dim3(256), 0, s, p); break;
        case 3: FERN_LAUNCH((gemm_f32_kernel<64, 64, 32, 32, 32, false>), grid, dim3(256), 0, s, p); break;
        case 6: FERN_LAUNCH((gemm_f32_skinny_kernel<5, 64>), grid, dim3(256), 0, s, p); break;
        case 8: case 9: case 10: case 11: launch_glds_8_11<4, false, 0>(c, grid, p, s); break;
        case 12: FERN_LAUNCH((gemm_f32_glds_kernel<256, 128, 64, 64, 16, 4>), grid, dim3(512), 0, s, p); break;
        case 13: FERN_LAUNCH((gemm_f32_glds_kernel<128, 256, 64, 64, 16, 4>), grid, dim3(512), 0, s, p); break;
        case 14: FERN_LAUNCH((gemm_f32_glds_kernel<128, 96, 32, 96, 16, 4>), grid, dim3(256), 0, s, p); break;
        case 15: FERN_LAUNCH((gemm_f32_glds_kernel<128, 160, 32, 160, 16, 4>), grid, dim3(256), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

static bool skinny_form_ok(const GemmParams& p) {      // forms the 16x16 small-M kernel covers ...
    return (p.K % 64) == 0 && p.aload == ALOAD_PLAIN && p.epi != EPI_SR_LOCAL && p.epi != EPI_PATCH_EMBED && !epi_is_sweep(p.epi);
}
static bool skinny_ok(const GemmParams& p) { return p.M <= 128 && skinny_form_ok(p); }      // ... and the shapes it is a candidate for on its own

// ---- per-shape tile selection (gemm_tuner.h has the store and the plans) ---------------------------------------------------------------
// The reduce epilogues are tuned like the stored ones: their partial sums are laid out per 32-column group, independent of the tile
// configuration.
static bool split_ok(const GemmParams& p) {      // row-independent epilogue and loader: the rows can be cut anywhere
    return p.aload == ALOAD_PLAIN && p.w_sample <= 1 && p.ksplit <= 1 &&
           (p.epi == EPI_BIAS || p.epi == EPI_BIAS_GELU || p.epi == EPI_BIAS_QUICKGELU || p.epi == EPI_BIAS_RELU || p.epi == EPI_BIAS_RESIDUAL ||
            p.epi == EPI_BIAS_RESIDUAL_RELU || p.epi == EPI_COLAFFINE_TANH);
}
// the rows [rows_a, M) of a plain-epilogue GEMM as a GEMM of their own
static GemmParams tail_rows(const GemmParams& p, int rows_a) {
    GemmParams t = p;
    t.A = p.A + (long)rows_a * p.lda;
    t.C = p.C + (long)rows_a * p.ldc;
    if (p.R) t.R = p.R + (long)rows_a * p.ldc;
    t.M = p.M - rows_a;
    return t;
}

// The blocks of a mixed plan's three bands of rows over an M x N problem: macro-tiles on [0, rows_a), 128x128 tiles on [rows_a, cfg_b),
// 64x128 tiles on [cfg_b, M).  Every band starts on a multiple of 8 blocks (block % 8 stays the XCD inside the band), so the counts are
// rounded up to 8 -- but for the last band that has blocks at all in `blocks`, the grid of the plan on its own.
struct MixedBands {
    int n_a8, n_b8, n_c8, blocks;
    MixedBands(const Plan& pl, int M, int N) {
        const bool wide = pl.cfg == kCfgMixed + 1;
        const int bma = wide ? 128 : 256, bna = wide ? 256 : 128, nbn = (N + 127) / 128;
        const int n_a = (pl.rows_a / bma) * ((N + bna - 1) / bna), n_b = ((pl.cfg_b - pl.rows_a + 127) / 128) * nbn, n_c = ((M - pl.cfg_b + 63) / 64) * nbn;
        n_a8 = (n_a + 7) & ~7;
        n_b8 = (n_b + 7) & ~7;
        n_c8 = (n_c + 7) & ~7;
        blocks = n_c > 0 ? n_a8 + n_b8 + n_c : n_b > 0 ? n_a8 + n_b : n_a;
    }
};
static hipError_t launch_mixed(const Plan& pl, const GemmParams& p, hipStream_t s) {
    if (!mixed_plan_ok(pl, p.M)) return hipErrorInvalidValue;
    const bool wide = pl.cfg == kCfgMixed + 1;
    const int ra = pl.rows_a, rb = pl.cfg_b;
    const MixedBands b(pl, p.M, p.N);
    if (p.split == 3) {
        if (wide) FERN_LAUNCH((gemm_f32_mixed_kernel<true, 3>), dim3(b.blocks), dim3(256), 0, s, p, ra, rb, b.n_a8, b.n_b8);
        else FERN_LAUNCH((gemm_f32_mixed_kernel<false, 3>), dim3(b.blocks), dim3(256), 0, s, p, ra, rb, b.n_a8, b.n_b8);
    } else if (wide) FERN_LAUNCH(gemm_f32_mixed_kernel<true>, dim3(b.blocks), dim3(512), 0, s, p, ra, rb, b.n_a8, b.n_b8);
    else FERN_LAUNCH(gemm_f32_mixed_kernel<false>, dim3(b.blocks), dim3(512), 0, s, p, ra, rb, b.n_a8, b.n_b8);
    return hipGetLastError();
}

// the cuts the tuners time for a mixed plan: ra by whole rounds of 512 / 256 macro-tiles or every full macro row, rb = everything /
// nothing / whole 128-row tiles / 128x128 tiles in whole rounds of the chip
static int mixed_candidates(int M, int N, Plan (&out)[32]) {
    int n = 0;
    auto add = [&](int cfg, int ra, int rb) {
        const Plan pl{cfg, ra, rb};
        if (!mixed_plan_ok(pl, M) || n >= 32) return;
        for (int i = 0; i < n; ++i)
            if (out[i].cfg == cfg && out[i].rows_a == ra && out[i].cfg_b == rb) return;
        out[n++] = pl;
    };
    const int nbn = (N + 127) / 128;
    for (int w = 0; w < 2; ++w) {
        const int bma = w ? 128 : 256, bna = w ? 256 : 128;
        const long nbna = (N + bna - 1) / bna, row_tiles = M / bma;
        const int ras[3] = {(int)row_tiles * bma, (int)((row_tiles * nbna / 512) * 512 / nbna) * bma, (int)((row_tiles * nbna / 256) * 256 / nbna) * bma};
        for (int ra : ras) {
            if (ra < bma) continue;
            const int mr = M - ra;
            add(kCfgMixed + w, ra, M);
            add(kCfgMixed + w, ra, ra);
            add(kCfgMixed + w, ra, ra + (mr / 128) * 128);
            add(kCfgMixed + w, ra, ra + (int)(((long)(mr / 128) * nbn / 256) * 256 / nbn) * 128);
        }
    }
    return n;
}

static hipError_t launch_plan(const Plan& pl, const GemmParams& p, hipStream_t s) {
    if (pl.cfg >= kCfgMixed) return launch_mixed(pl, p, s);
    if (pl.rows_a <= 0 || pl.rows_a >= p.M) return launch_cfg(pl.cfg, p, s);
    if ((pl.cfg_b == 6 || pl.cfg == 6) && !skinny_form_ok(p)) return launch_cfg(pl.cfg == 6 ? 11 : pl.cfg, p, s);      // a pinned pair on a call the 16x16 kernel cannot serve
    g_last_dispatches = 2;
    GemmParams head = p;
    head.M = pl.rows_a;
    hipError_t e = launch_cfg(pl.cfg, head, s);
    if (e != hipSuccess) return e;
    return launch_cfg(pl.cfg_b, tail_rows(p, pl.rows_a), s);
}

// The trials of a shape of the fp32 family (lookup_or_tune: `tuned`).  Rounds outermost: every candidate is timed in two rounds and
// keeps its faster time -- the first launches after an idle spell run while the clocks are still ramping, which would otherwise favour
// whichever candidates happen to be tried last.
static Plan tune_shape(const GemmParams& p, hipStream_t s, bool& tuned) {
    const int fallback_cfg = choose_cfg(p.M, p.N, p.K);
    const Plan fallback{fallback_cfg, 0, fallback_cfg};
    tuned = false;
    long out_rows = p.M;
    if (p.epi == EPI_PATCH_EMBED) out_rows = p.M + p.M / (p.grid * p.grid) + 2;
    const bool reduce = epi_is_reduce(p.epi);
    const size_t scratch_floats = reduce ? (size_t)p.M * ((p.N + 31) / 32) : p.epi == EPI_TOPK_FILTER ? 4 :
                                  p.epi == EPI_RANK_COUNT ? (size_t)RANKC_P * p.M * RANKC_T : (size_t)out_rows * p.ldc;
    TrialTimer timer(s);
    float* scratch = static_cast<float*>(timer.scratch(scratch_floats * sizeof(float)));
    if (!timer.ok()) return fallback;
    GemmParams q = p;      // split-K launches write only to kpart, which is scratch already
    q.gate = nullptr;
    if (reduce) q.partial = scratch;
    else q.C = scratch;       // residual input (p.R) is only read: tuning has no side effects on the caller's buffers
    if (p.epi == EPI_TOPK_FILTER) q.filt.thr_key = nullptr;      // trial launches reject every score: nothing is appended
    if (p.epi == EPI_RANK_COUNT) q.rankc.partial = reinterpret_cast<int*>(scratch);      // trial launches count (atomics and all) into scratch sets
    auto timed = [&](auto&& launch) { return timer.best_ms(launch, 1, 2); };
    static const int cands[] = {0, 1, 2, 3, 6, 8, 9, 10, 11, 12, 13, 14, 15};
    // {bulk cfg, remainder cfg, tiles per round}: the bulk covers the rows whose tiles fill whole rounds of the chip -- 256 = one tile
    // per CU; the 8-wave macro-tiles keep two workgroups per CU, so a round of 512 gives every CU an even number of them
    static const int pairs[][3] = {{8, 11, 256}, {8, 9, 256}, {9, 11, 256}, {10, 11, 256}, {12, 8, 256}, {12, 8, 512}, {12, 11, 256}, {12, 11, 512},
                                   {13, 8, 256}, {13, 8, 512}, {13, 11, 256}, {13, 11, 512}};
    constexpr int NC = sizeof(cands) / sizeof(cands[0]), NP = sizeof(pairs) / sizeof(pairs[0]);
    float t_single[NC], t_pair[NP];
    Plan pair_plan[NP];
    for (float& t : t_single) t = 1e30f;
    for (float& t : t_pair) t = 1e30f;
    // bulk + remainder: only worth a look when the matrix is several rounds of tiles deep
    const bool try_pairs = split_ok(p) && p.M >= 2048 && p.K % 16 == 0;
    for (int round = 0; round < 2; ++round) {
        for (int i = 0; i < NC; ++i) {
            const int c = cands[i];
            if (c == 6 && !skinny_ok(p)) continue;
            if ((c == 12 || c == 13) && (epi_is_sweep(p.epi) || p.aload != ALOAD_PLAIN || p.M < 2048)) continue;      // macro-tiles: plain loader, stored outputs, deep matrices
            if (c >= 14) {      // odd-width tiles: only where they pad fewer columns than the 64-wide tiles do (N = 80: 96 < 128) or as many with a wider tile (N = 160, 320)
                const int pad64 = (p.N + 63) / 64 * 64, padc = (p.N + kCfgs[c].bn - 1) / kCfgs[c].bn * kCfgs[c].bn;
                if (epi_is_sweep(p.epi) || epi_is_reduce(p.epi) || p.M < 1024 || (c == 14 ? padc >= pad64 : padc > pad64)) continue;
            }
            if (c < 8 && epi_is_sweep(p.epi)) continue;
            if (c >= 8 && p.aload == ALOAD_IM2COL) continue;
            if (c < 8 && p.aload == ALOAD_CONV3) continue;
            if (p.K % kCfgs[c].bk) continue;
            t_single[i] = std::min(t_single[i], timed([&] { return launch_cfg(c, q, s); }));
        }
        for (int i = 0; try_pairs && i < NP; ++i) {
            const int bm = kCfgs[pairs[i][0]].bm, bn = kCfgs[pairs[i][0]].bn;
            const long nbn = (p.N + bn - 1) / bn, tiles = (long)((p.M + bm - 1) / bm) * nbn;
            const int rows_a = (int)((tiles / pairs[i][2]) * pairs[i][2] / nbn) * bm;
            if (rows_a < bm || rows_a >= p.M) continue;
            pair_plan[i] = Plan{pairs[i][0], rows_a, pairs[i][1]};
            t_pair[i] = std::min(t_pair[i], timed([&] { return launch_plan(pair_plan[i], q, s); }));
        }
    }
    // mixed plans (one launch, three bands of rows: macro-tiles, 128x128, 64x128): where to cut is a balance question the
    // dispatcher answers at run time, so a handful of cuts are simply timed
    Plan mixed[32];
    float t_mixed[32];
    int nmixed = 0;
    if (try_pairs && p.ksplit <= 1) {
        nmixed = mixed_candidates(p.M, p.N, mixed);
        for (int i = 0; i < nmixed; ++i) t_mixed[i] = 1e30f;
        for (int round = 0; round < 2; ++round)
            for (int i = 0; i < nmixed; ++i) t_mixed[i] = std::min(t_mixed[i], timed([&] { return launch_mixed(mixed[i], q, s); }));
    }
    Plan best = fallback;
    float best_ms = 1e30f;
    for (int i = 0; i < NC; ++i)
        if (t_single[i] < best_ms) { best_ms = t_single[i]; best = Plan{cands[i], 0, cands[i]}; }
    for (int i = 0; i < NP; ++i)
        if (t_pair[i] < best_ms * 0.99f) { best_ms = t_pair[i]; best = pair_plan[i]; }      // two launches must earn their keep
    for (int i = 0; i < nmixed; ++i)
        if (t_mixed[i] < best_ms) { best_ms = t_mixed[i]; best = mixed[i]; }
    tuned = best_ms < 1e29f;
    return best;
}

// ---- f32x3 family (GemmParams.split == 3; gemm_tuner.h: kCfgsS) -----------------------------------------------------------------------
static bool split_family_ok(const GemmParams& p) {
    return p.split == 3 && split_ok(p) && p.M >= 256 && p.K % 16 == 0;
}
static hipError_t launch_cfg_split(int c, const GemmParams& p, hipStream_t s) {
    const int nb = tile_blocks(kCfgsS[c].bm, kCfgsS[c].bn, p);
    switch (c) {
        case 0: FERN_LAUNCH((gemm_f32_glds_kernel<128, 128, 64, 64, 16, 3, false, 0, false, 3>), dim3(nb), dim3(256), 0, s, p); break;
        case 1: FERN_LAUNCH((gemm_f32_glds_kernel<256, 128, 128, 64, 16, 2, false, 0, false, 3>), dim3(nb), dim3(256), 0, s, p); break;
        case 2: FERN_LAUNCH((gemm_f32_glds_kernel<128, 256, 64, 128, 16, 2, false, 0, false, 3>), dim3(nb), dim3(256), 0, s, p); break;
        case 3: FERN_LAUNCH((gemm_f32_glds_kernel<64, 128, 32, 64, 16, 4, false, 0, false, 3>), dim3(nb), dim3(256), 0, s, p); break;
        case 4: FERN_LAUNCH((gemm_f32_glds_kernel<128, 64, 64, 32, 16, 4, false, 0, false, 3>), dim3(nb), dim3(256), 0, s, p); break;
        case 5: FERN_LAUNCH((gemm_f32_glds_kernel<64, 64, 32, 32, 16, 4, false, 0, false, 3>), dim3(nb), dim3(256), 0, s, p); break;
        case 6: FERN_LAUNCH((gemm_f32_glds_kernel<256, 256, 128, 64, 16, 2, false, 0, false, 3>), dim3(nb), dim3(512), 0, s, p); break;
        case 7: FERN_LAUNCH((gemm_f32x3_shared_kernel<256, 256>), dim3(nb), dim3(512), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
static int heuristic_split(const GemmParams& p) {
    const long t128 = (long)((p.M + 127) / 128) * ((p.N + 127) / 128);
    return t128 >= 1024 ? 1 : t128 >= 384 ? 0 : 5;
}
static hipError_t launch_plan_split(const Plan& pl, const GemmParams& p, hipStream_t s) {
    return pl.cfg >= kCfgMixed ? launch_mixed(pl, p, s) : launch_cfg_split(pl.cfg, p, s);
}
static Plan tune_shape_split(const GemmParams& p, hipStream_t s, bool& tuned) {      // rounds outermost, as tune_shape
    tuned = false;
    const int fb = heuristic_split(p);
    const Plan fallback{fb, 0, fb};
    TrialTimer timer(s);
    GemmParams q = p;
    q.C = static_cast<float*>(timer.scratch((size_t)p.M * p.ldc * sizeof(float)));      // the residual input is only read
    if (!timer.ok()) return fallback;
    Plan cand[kNumCfgsS + 32];
    int nc = 0;
    for (int c = 0; c < kNumCfgsS; ++c) cand[nc++] = Plan{c, 0, c};
    if (p.M >= 2048) {
        Plan mixed[32];
        const int nm = mixed_candidates(p.M, p.N, mixed);
        for (int i = 0; i < nm; ++i) cand[nc++] = mixed[i];
    }
    float t[kNumCfgsS + 32];
    for (float& v : t) v = 1e30f;
    for (int round = 0; round < 2; ++round)
        for (int c = 0; c < nc; ++c) t[c] = std::min(t[c], timer.best_ms([&] { return launch_plan_split(cand[c], q, s); }, 1, 2));
    Plan best = fallback;
    float best_ms = 1e30f;
    for (int c = 0; c < nc; ++c)
        if (t[c] < best_ms) { best_ms = t[c]; best = cand[c]; }
    tuned = best_ms < 1e29f;
    return best;
}
static hipError_t launch_gemm_split(const GemmParams& p, hipStream_t s) {
    const int f = forced_cfg(FAM_F32X3);
    if (f >= 0 && f < kNumCfgsS) return launch_cfg_split(f, p, s);
    const double flops = 2.0 * p.M * (double)p.N * p.K;
    const int hb = heuristic_split(p);
    Plan pl{hb, 0, hb};
    if (tuning_enabled() && flops >= 2.5e8 && flops <= 2e11)
        pl = lookup_or_tune(choice_store().f32x3, ShapeKey{p.M, p.N, p.K, p.epi, 0}, [&](bool& tuned) { return tune_shape_split(p, s, tuned); });
    return launch_plan_split(pl, p, s);
}

hipError_t launch_gemm(const GemmParams& p, hipStream_t s) {
    g_last_dispatches = 1;
    if (p.M <= 0 || p.N <= 0) return hipSuccess;
    if (p.K <= 0 || (p.K % 16) != 0 || (p.ldw & 3) || (p.aload == ALOAD_PLAIN && (p.lda & 3))) return hipErrorInvalidValue;
    if (p.aload == ALOAD_CONV3 && (p.conv_h <= 0 || p.conv_w <= 0 || p.conv_c <= 0 || p.conv_c % 16 || p.K != 9 * p.conv_c || !p.zeros ||
                                   ((uintptr_t)p.zeros & 15) || p.M % (p.conv_h * p.conv_w)))
        return hipErrorInvalidValue;
    if (((uintptr_t)p.A & 15) || ((uintptr_t)p.W & 15)) return hipErrorInvalidValue;
    if (p.aload == ALOAD_IM2COL && ((p.patch & 3) || (p.img & 3))) return hipErrorInvalidValue;
    if (p.ksplit > 1 && (p.aload != ALOAD_PLAIN || !p.kpart || p.K % (p.ksplit * 64) || (p.N & 3))) return hipErrorInvalidValue;
    if (split_family_ok(p)) return launch_gemm_split(p, s);
    int c = choose_cfg(p.M, p.N, p.K);
    // tuned: problems big enough to matter and small enough that ~30 trial launches are cheap (beyond ~0.2 TFLOP per launch
    // -- the gallery-side GEMMs over tens of thousands of rows -- every candidate fills the chip and the heuristic is used)
    const double flops = 2.0 * p.M * (double)p.N * p.K;
    const bool tunable = forced_cfg(FAM_F32) < 0 && tuning_enabled() && flops >= 2.5e8 && flops <= 2e11;
    if (tunable) {
        const ShapeKey key{p.M, p.N, p.K, p.epi, p.aload + 1000 * (p.ksplit > 1 ? p.ksplit : 0)};
        const Plan pl = lookup_or_tune(choice_store().f32, key, [&](bool& tuned) { return tune_shape(p, s, tuned); });
        if (pl.rows_a > 0 && split_ok(p)) return launch_plan(pl, p, s);
        c = pl.cfg < kCfgMixed ? pl.cfg : choose_cfg(p.M, p.N, p.K);      // a pinned mixed plan on a call it cannot serve: heuristic tile
    }
    if (c == 6 && !skinny_ok(p)) c = (p.K & 31) ? best_of(p.M, p.N, 8, 12) : best_of(p.M, p.N, 0, kNumAuto);   // forced but not applicable
    if (c != 6 && forced_cfg(FAM_F32) < 0 && !tunable && p.M <= 64 && p.N >= 256 && skinny_ok(p)) c = 6;     // untuned small-M GEMMs
    if (epi_is_sweep(p.epi) && (c < 8 || c > 11)) c = 8 + (c & 3);     // filtered / counting sweep: the four LDS-DMA tiles only
    if (p.aload == ALOAD_CONV3 && (c < 8 || c == 12 || c == 13)) c = 8 + (c & 3);     // 3x3 window: LDS-DMA family without the macro-tiles
    if (c >= 8 && p.aload == ALOAD_IM2COL) c &= 3;                        // patch loader: register-staged family only
    return launch_cfg(c, p, s);
}

// fern's GEMM pairs (api_ctx.hip: run_gemm_pair): p1 = the image tower's GEMM, p2 = the text tower's GEMM of the same layer.  One launch when
// p1's tuned plan is a mixed plan and both calls are plain (row-independent epilogue, plain loader, same arithmetic family); two launches
// otherwise -- also the first time a shape is seen (launch_gemm tunes it; the next call finds the plan) and for the pairs that the one-launch
// form does not speed up (pair_wins, timed once per pair of shapes).  FERN_GEMM_PAIR=0 turns it off.
static hipError_t launch_pair_kernel(const Plan& pl, const GemmParams& p1, const GemmParams& p2, hipStream_t s) {
    const bool wide = pl.cfg == kCfgMixed + 1;
    const int ra = pl.rows_a, rb = pl.cfg_b, nbn2 = (p2.N + 127) / 128;
    const MixedBands b(pl, p1.M, p1.N);
    const int rb2 = (p2.M / 128) * 128;
    const int n_d = (rb2 / 128) * nbn2, n_e = ((p2.M - rb2 + 63) / 64) * nbn2;
    const int n_d8 = (n_d + 7) & ~7, n_e8 = (n_e + 7) & ~7;      // the second problem's bands start on a multiple of 8 blocks too
    const int grid = n_d8 + n_e8 + b.blocks;
    if (p1.split == 3) {
        if (wide) FERN_LAUNCH((gemm_f32_pair_kernel<true, 3>), dim3(grid), dim3(256), 0, s, p1, ra, rb, b.n_a8, b.n_b8, b.n_c8, p2, rb2, n_d8);
        else FERN_LAUNCH((gemm_f32_pair_kernel<false, 3>), dim3(grid), dim3(256), 0, s, p1, ra, rb, b.n_a8, b.n_b8, b.n_c8, p2, rb2, n_d8);
    } else if (wide) FERN_LAUNCH(gemm_f32_pair_kernel<true>, dim3(grid), dim3(512), 0, s, p1, ra, rb, b.n_a8, b.n_b8, b.n_c8, p2, rb2, n_d8);
    else FERN_LAUNCH(gemm_f32_pair_kernel<false>, dim3(grid), dim3(512), 0, s, p1, ra, rb, b.n_a8, b.n_b8, b.n_c8, p2, rb2, n_d8);
    return hipGetLastError();
}
// per (first shape, second shape): does the ONE-launch form beat two launches?  Timed once on scratch outputs, like the tile tuners: the
// second problem rides as 128x128 / 64x128 tiles, which is not every shape's best geometry (4928 x 512 x 2048 behind 12608 x 768 x 3072:
// 117 TFLOP/s paired against 120 as two launches; the other three pairs of a ViT-B/16 + text layer gain 1-2 %).  Candidates outermost:
// the two-launch form first, both of its rounds (its warm launches also tune the second shape), then the one-launch form.
static int pair_wins(const Plan& pl, const GemmParams& p1, const GemmParams& p2, hipStream_t s, bool& timed) {
    timed = false;
    TrialTimer timer(s);
    GemmParams q1 = p1, q2 = p2;      // the residual inputs are only read: no side effects on the caller's buffers
    q1.C = static_cast<float*>(timer.scratch((size_t)p1.M * p1.ldc * sizeof(float)));
    q2.C = static_cast<float*>(timer.scratch((size_t)p2.M * p2.ldc * sizeof(float)));
    if (!timer.ok()) return 0;
    const float t_two = timer.best_ms([&] { const hipError_t e = launch_gemm(q1, s); return e != hipSuccess ? e : launch_gemm(q2, s); }, 2, 2);
    const float t_one = timer.best_ms([&] { return launch_pair_kernel(pl, q1, q2, s); }, 2, 2);
    timed = t_two < 1e29f && t_one < 1e29f;
    return timed && t_one < t_two;
}
hipError_t launch_gemm_pair(const GemmParams& p1, const GemmParams& p2, hipStream_t s) {
    bool paired = false;
    Plan pl{-1, 0, 0};
    const bool sp = p1.split == 3, same_family = sp == (p2.split == 3);
    if (pair_enabled() && same_family && split_ok(p1) && split_ok(p2) && !p1.gate && !p2.gate && p1.K % 16 == 0 && p2.K % 16 == 0 && p1.M >= 256 && p2.M >= 64 &&
        p2.N >= 128 && !(p1.lda & 3) && !(p2.lda & 3) && !(p1.ldw & 3) && !(p2.ldw & 3) && !((uintptr_t)p1.A & 15) && !((uintptr_t)p2.A & 15) &&
        !((uintptr_t)p1.W & 15) && !((uintptr_t)p2.W & 15) && forced_cfg(FAM_F32) < 0 && forced_cfg(FAM_F32X3) < 0 && tuning_enabled() &&
        (!sp || (split_family_ok(p1) && split_family_ok(p2)))) {
        load_pinned_tiles();
        ChoiceStore& st = choice_store();
        {
            std::lock_guard<std::mutex> lock(st.mu);
            const std::map<ShapeKey, Plan>& plans = sp ? st.f32x3 : st.f32;
            const auto it = plans.find(ShapeKey{p1.M, p1.N, p1.K, p1.epi, sp ? 0 : p1.aload});
            if (it != plans.end()) pl = it->second;
        }
        // no mixed plan (yet): two launches -- launch_gemm tunes the shape on first sight
        if (pl.cfg >= kCfgMixed && mixed_plan_ok(pl, p1.M)) {
            const PairKey key{ShapeKey{p1.M, p1.N, p1.K, p1.epi, sp ? 3000 : p1.aload}, ShapeKey{p2.M, p2.N, p2.K, p2.epi, sp ? 3000 : p2.aload}};
            paired = lookup_or_tune_pair(st.pair, key, [&](bool& timed) { return pair_wins(pl, p1, p2, s, timed); }) != 0;
        }
    }
    if (!paired) {
        const hipError_t e = launch_gemm(p1, s);
        if (e != hipSuccess) return e;
        const int d1 = g_last_dispatches;
        const hipError_t e2 = launch_gemm(p2, s);
        g_last_dispatches += d1;
        return e2;
    }
    g_last_dispatches = 1;
    return launch_pair_kernel(pl, p1, p2, s);
}

}  // namespace fern

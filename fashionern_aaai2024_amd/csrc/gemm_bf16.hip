// bf16 MFMA GEMM for gfx950 (CDNA4): C[M,N] = A[M,K] * W[N,K]^T, bf16 operands, fp32 accumulation, fused epilogues.
//
// This is the "perf mode" of the encoder GEMMs (BASELINE config 5's reduced-precision encoder):
// the CLIP towers' QKV / out-proj / MLP contractions with activations and weights rounded to bf16 (RNE) and summed in
// fp32 on v_mfma_f32_32x32x16_bf16 (16 x the fp32 matrix rate).  The residual stream, LayerNorm statistics, softmax
// and every epilogue stay fp32.
//
// Structure = the LDS-DMA fp32 kernel of gemm.hip in byte terms: A and W tiles go L2 -> LDS with
// global_load_lds_dwordx4 (lane-linear 1 KiB pieces, bank swizzle applied on the per-lane SOURCE address), double
// buffered, one barrier per k tile.  A tile row is BKE bf16 = 64 or 128 bytes; one ds_read_b128 fetches the 8
// consecutive k values a lane feeds to one 32x32x16 MFMA (lane half h supplies k = 16*kk + 8*h .. +7 of both
// operands).  Every configuration adds the 16-wide k groups in ascending order, so all of them produce bit-identical
// results and a row's result does not depend on the batch it is part of.
#include "gemm_tile.h"
#include "gemm_tuner.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace fern {

// FP8: the operands are OCP e4m3fn bytes and the MFMA is v_mfma_f32_32x32x16_fp8_fp8 (same rate as bf16, half the bytes):
// a BKE-element tile row is then BKE bytes, one ds_read_b128 holds the fragments of TWO consecutive MFMA k-steps (low /
// high 8 bytes), and the tile loop runs half as many iterations for the same K.
// bytes of LDS a configuration stages through (the wrappers and the pair kernel size their one __shared__ object with it)
template <int BM, int BN, int BKE, int STAGES, bool FP8>
constexpr int bf16_tile_lds() { return STAGES * (BM + BN) * BKE * (FP8 ? 1 : 2); }
// The kernel body as a device function of (problem, block index, LDS base): gemm_bf16_glds_kernel is its one-problem wrapper, and
// gemm_mxbf_pair_kernel below runs it on the SECOND problem of an image + text pair (round 6).
template <int BM, int BN, int WM, int WN, int BKE, int STAGES, bool FP8 = false>
__device__ __forceinline__ void bf16_tile_body(const GemmParams& p, const int bid, char* smem) {
    constexpr int WAVES_N = BN / WN;
    constexpr int WAVES_M = BM / WM;
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int ROWS = BM + BN;                        // A rows then W rows
    constexpr int ES = FP8 ? 1 : 2;                      // operand element size (bytes)
    constexpr int RB = BKE * ES;                         // bytes per tile row (64 or 128)
    using TR = TileRows<RB>;
    constexpr int PIECES = ROWS / TR::RPP;
    static_assert(PIECES % NW == 0, "pieces must divide over the waves");
    constexpr int PPW = PIECES / NW;
    constexpr int TILE = ROWS * RB;                      // bytes per stage

    // (the caller's ONE __shared__ object -- see gemm.hip: a second one makes hipcc drain the DMA before every first fragment read)
    static_assert(STAGES * TILE == bf16_tile_lds<BM, BN, BKE, STAGES, FP8>(), "LDS size");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int l31 = lane & 31, lh = lane >> 5;

    const TileAt at = tile_at<BM, BN>(bid, p.M, p.N);
    const int bm = at.bm, bn = at.bn, nbn = at.nbn;

    const char* src[PPW];
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int piece = wave + NW * j;                       // wave-uniform
        const int trow = piece * TR::RPP + lane / TR::C4;      // row in the [A; W] tile-row space
        const int chunk = TR::store_chunk(lane, trow);
        if (trow < BM) {
            int row = bm * BM + trow;
            row = row < p.M ? row : p.M - 1;
            src[j] = reinterpret_cast<const char*>(p.Ab) + (long)row * p.lda * ES + chunk * 16;
        } else {
            int row = bn * BN + (trow - BM);
            row = row < p.N ? row : p.N - 1;
            src[j] = reinterpret_cast<const char*>(p.Wb) + (long)row * p.ldw * ES + chunk * 16;
        }
    }
    auto stage = [&](int buf, int k0) {
#pragma unroll
        for (int j = 0; j < PPW; ++j) {
            const int piece = wave + NW * j;
            lds_dma16(src[j] + (long)k0 * ES, smem + buf * TILE + piece * 1024);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int sw = TR::read_swizzle(l31);
    auto compute = [&](int buf) {
        const char* As = smem + buf * TILE;
        const char* Ws = As + BM * RB;
#pragma unroll
        for (int kk = 0; kk < RB / 32; ++kk) {                  // one 16-byte chunk per lane half and step
            const int pc = ((2 * kk + lh) ^ sw) * 16;
            bf16x8 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const bf16x8*>(As + (wm * WM + i * 32 + l31) * RB + pc);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const bf16x8*>(Ws + (wn * WN + j * 32 + l31) * RB + pc);
            if (FP8) {
                // the 16 bytes are k = 32kk + 16h .. +15 of this lane's row: bytes 0-7 feed one 32x32x16 step, 8-15 the next
                // (both operands use the same k grouping, so the sum is the plain dot product)
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            const i64x2 a2 = __builtin_bit_cast(i64x2, af[i]), b2 = __builtin_bit_cast(i64x2, bf[j]);
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a2[e], b2[e], acc[i][j], 0, 0, 0);
                        }
            } else {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }
    };

    // STAGES-deep ring: tiles kt+1 .. kt+STAGES-2 stay in flight while tile kt is consumed (a bf16 tile is only ~256 MFMA
    // cycles of work per wave, far less than one L2/HBM round trip, so a single tile in flight leaves the loop latency-bound).
    // Top of iteration kt: wait until this wave's pieces of tile kt have landed (counted vmcnt: younger tiles may still be
    // in flight), barrier (=> every wave's pieces landed, and every wave is done reading tile kt-1), then refill the slot
    // of tile kt-1 with tile kt+STAGES-1.
    const int nk = p.K / BKE;
#pragma unroll
    for (int t = 0; t < STAGES - 1; ++t)
        if (t < nk) stage(t, t * BKE);
    int slot = 0;                                   // ring slot of tile kt
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + STAGES - 2 < nk) {                 // steady state: STAGES-2 younger tiles issued after tile kt
            if (STAGES == 2) wait_vmcnt<0>();
            else if (STAGES == 3) wait_vmcnt<PPW>();
            else wait_vmcnt<2 * PPW>();
        } else {
            wait_vmcnt<0>();
        }
        __builtin_amdgcn_s_barrier();
        if (kt + STAGES - 1 < nk) {
            int fill = slot + STAGES - 1;
            fill = fill >= STAGES ? fill - STAGES : fill;
            stage(fill, (kt + STAGES - 1) * BKE);
        }
        compute(slot);
        slot = slot + 1 == STAGES ? 0 : slot + 1;
    }
    gemm_epilogue<BM, BN, WM, WN, TM, TN, WAVES_N, true>(p, acc, bm, bn, nbn, wm, wn, l31, lh, tid);
}
template <int BM, int BN, int WM, int WN, int BKE, int STAGES, int MINW, bool FP8 = false>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64, MINW) void gemm_bf16_glds_kernel(GemmParams p) {
    __shared__ __attribute__((aligned(1024))) char smem[bf16_tile_lds<BM, BN, BKE, STAGES, FP8>()];
    bf16_tile_body<BM, BN, WM, WN, BKE, STAGES, FP8>(p, blockIdx.x, smem);
}

// ---- MX (block-scaled) fp8: v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands --------------------------------------------
// One instruction is a 32x32 tile over 64 k: lane (r = lane & 31, h = lane >> 5) supplies 32 bytes of its row of A (8 VGPRs) and of
// W -- bytes 0-15 are k = 16h .. 16h+15, bytes 16-31 are k = 32 + 16h .. +15 -- plus ONE E8M0 scale byte per operand: the byte of
// the h = 0 lane scales k = 0..31 of that row (bytes 0-15 of BOTH halves), the h = 1 lane's byte k = 32..63
// (tools/probe/mfma_scale_probe2.hip maps byte -> k and byte -> scale on hardware; mfma_scale_probe.hip the opsel byte select).
// It issues in twice the cycles of the 32x32x16 bf16 form at 4x the k: twice the bf16 / plain-fp8 rate.
//
// Tiles: 128-byte rows (128 k = two MFMA k steps), the LDS-DMA staging and chunk swizzle of the kernel above; a lane's 32 bytes are
// two swizzled 16-byte chunks.  Scales travel with the tile: the mx_scale_offset layout holds one dword per (128-k tile, row) =
// bytes (step 0, h 0), (step 0, h 1), (step 1, h 0), (step 1, h 1), so a tile's scales are (BM + BN) consecutive dwords per operand
// block, staged by 4-byte LDS-DMA pieces of 64 rows behind the tile's data.  A lane reads its row's dword, shifts it right by 8h
// and opsel (0 / 2) picks the step's byte; its data are the two swizzled 16-byte chunks h and 2 + h of the step.  Every configuration adds the 64-wide k steps in ascending order.
template <int BM, int BN, int STAGES, int RB>
constexpr int mx8_tile_lds() { return STAGES * (((BM + BN) * RB + (BM + BN) * 4 + 1023) / 1024 * 1024); }
// body / wrapper split as for the bf16 kernel above
template <int BM, int BN, int WM, int WN, int STAGES, int RB = 128>
__device__ __forceinline__ void mx8_tile_body(const GemmParams& p, const int bid, char* smem) {
    constexpr int WAVES_N = BN / WN;
    constexpr int WAVES_M = BM / WM;
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int ROWS = BM + BN;
    static_assert(RB == 128 || RB == 64, "tile rows are one or two 64-k MFMA steps");   // RB: bytes (= k) per tile row
    using TR = TileRows<RB>;
    constexpr int PIECES = ROWS / TR::RPP;
    static_assert(PIECES % NW == 0, "pieces must divide over the waves");
    constexpr int PPW = PIECES / NW;
    constexpr int SP = ROWS / 64;                        // 256-byte scale pieces (64 rows x 1 dword)
    constexpr int SPW = (SP + NW - 1) / NW;              // per wave (the surplus re-stages a piece: same bytes, same place)
    constexpr int DATA = ROWS * RB;
    constexpr int TILE = (DATA + ROWS * 4 + 1023) / 1024 * 1024;   // bytes per stage: rows, then one scale dword per row
    static_assert(STAGES >= 2 && STAGES <= 4, "ring depth");
    static_assert(STAGES * TILE == mx8_tile_lds<BM, BN, STAGES, RB>(), "LDS size");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int l31 = lane & 31, lh = lane >> 5;

    const TileAt at = tile_at<BM, BN>(bid, p.M, p.N);
    const int bm = at.bm, bn = at.bn, nbn = at.nbn;

    const char* src[PPW];
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int piece = wave + NW * j;
        const int trow = piece * TR::RPP + lane / TR::C4;
        const int chunk = TR::store_chunk(lane, trow);
        if (trow < BM) {
            int row = bm * BM + trow;
            row = row < p.M ? row : p.M - 1;
            src[j] = reinterpret_cast<const char*>(p.Ab) + (long)row * p.lda + chunk * 16;
        } else {
            int row = bn * BN + (trow - BM);
            row = row < p.N ? row : p.N - 1;
            src[j] = reinterpret_cast<const char*>(p.Wb) + (long)row * p.ldw + chunk * 16;
        }
    }
    const char* ssrc[SPW];
    long sstep[SPW];                                      // bytes between consecutive k tiles of that operand's scales
#pragma unroll
    for (int j = 0; j < SPW; ++j) {
        const int sp = (wave + NW * j) % SP;
        const int trow = sp * 64 + lane;
        if (trow < BM) {
            int row = bm * BM + trow;
            row = row < p.M ? row : p.M - 1;
            ssrc[j] = reinterpret_cast<const char*>(p.mxa) + (long)row * 4;
            sstep[j] = p.mxa_rows * 4;
        } else {
            int row = bn * BN + (trow - BM);
            row = row < p.N ? row : p.N - 1;
            ssrc[j] = reinterpret_cast<const char*>(p.mxw) + (long)row * 4;
            sstep[j] = p.mxw_rows * 4;
        }
    }
    auto stage = [&](int buf, int kt) {
#pragma unroll
        for (int j = 0; j < PPW; ++j) {
            const int piece = wave + NW * j;
            lds_dma16(src[j] + (long)kt * RB, smem + buf * TILE + piece * 1024);
        }
#pragma unroll
        for (int j = 0; j < SPW; ++j) {
            const int sp = (wave + NW * j) % SP;
            lds_dma4(ssrc[j] + (RB == 64 ? kt >> 1 : kt) * sstep[j], smem + buf * TILE + DATA + sp * 256);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int sw = TR::read_swizzle(l31);
    auto compute = [&](int buf, int kt) {
        const char* As = smem + buf * TILE;
        const char* Ws = As + BM * RB;
        const unsigned* Ss = reinterpret_cast<const unsigned*>(As + DATA);
        int sa[TM], sb[TN];
        const int sh = RB == 64 ? 16 * (kt & 1) + 8 * lh : 8 * lh;       // 64-byte rows: a tile is ONE step, the dword covers two tiles
#pragma unroll
        for (int i = 0; i < TM; ++i) sa[i] = (int)(Ss[wm * WM + i * 32 + l31] >> sh);
#pragma unroll
        for (int j = 0; j < TN; ++j) sb[j] = (int)(Ss[BM + wn * WN + j * 32 + l31] >> sh);
#pragma unroll
        for (int e = 0; e < RB / 64; ++e) {                     // the 64-k MFMA steps of a tile
            const int pc0 = ((4 * e + lh) ^ sw) * 16, pc1 = ((4 * e + 2 + lh) ^ sw) * 16;     // k = 16h .. +15 and 32 + 16h .. +15
            i32x8 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const char* r = As + (wm * WM + i * 32 + l31) * RB;
                af[i] = __builtin_shufflevector(*reinterpret_cast<const i32x4*>(r + pc0), *reinterpret_cast<const i32x4*>(r + pc1), 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const char* r = Ws + (wn * WN + j * 32 + l31) * RB;
                bf[j] = __builtin_shufflevector(*reinterpret_cast<const i32x4*>(r + pc0), *reinterpret_cast<const i32x4*>(r + pc1), 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (e == 0) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[i], bf[j], acc[i][j], 0, 0, 0, sa[i], 0, sb[j]);
                    else acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[i], bf[j], acc[i][j], 0, 0, 2, sa[i], 2, sb[j]);
                }
        }
    };

    const int nk = p.K / RB;
#pragma unroll
    for (int t = 0; t < STAGES - 1; ++t)
        if (t < nk) stage(t, t);
    int slot = 0;
    for (int kt = 0; kt < nk; ++kt) {
        // tiles kt+1 .. kt+STAGES-2 may stay in flight; near the end fewer have been issued
        const int younger = nk - 1 - kt < STAGES - 2 ? nk - 1 - kt : STAGES - 2;
        if (STAGES >= 4 && younger == 2) wait_vmcnt<2 * (PPW + SPW)>();
        else if (STAGES >= 3 && younger == 1) wait_vmcnt<PPW + SPW>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (kt + STAGES - 1 < nk) {
            int fill = slot + STAGES - 1;
            fill = fill >= STAGES ? fill - STAGES : fill;
            stage(fill, kt + STAGES - 1);
        }
        compute(slot, kt);
        slot = slot + 1 == STAGES ? 0 : slot + 1;
    }
    if (!p.out_mx8) {
        gemm_epilogue<BM, BN, WM, WN, TM, TN, WAVES_N, true, 2, false>(p, acc, bm, bn, nbn, wm, wn, l31, lh, tid);
        return;
    }
    // Quantising epilogue: bias (+ GELU) in the accumulator layout (lane = column), then each 32x32 tile is turned through a
    // private LDS patch so that a lane holds 16 consecutive columns of ONE row (2 lanes per row = one 32-column MX block):
    // block maximum -> E8M0 byte -> 16 e4m3fn bytes, one 16-byte store per lane.
    __syncthreads();                                         // every wave is done with the operand tiles
    constexpr int PS = 36;                                   // patch row stride in floats (16-byte aligned rows)
    float* patch = reinterpret_cast<float*>(smem) + wave * (32 * PS);
    static_assert(NW * 32 * PS * 4 <= STAGES * TILE, "patches must fit the operand ring");
    const int row_w = bm * BM + wm * WM, col_w = bn * BN + wn * WN;
    const int rr = lane >> 1, hh = lane & 1;
    unsigned char* C8 = reinterpret_cast<unsigned char*>(p.C);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int row0 = row_w + i * 32, col0 = col_w + j * 32;            // wave-uniform
            if (row0 >= p.M || col0 >= p.N) continue;
            const float bia = p.bias ? p.bias[col0 + l31] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                f32x2 v2 = {acc[i][j][r] + bia, acc[i][j][r + 1] + bia};
                if (p.epi == EPI_BIAS_GELU) v2 = gelu_tanh2(v2);      // the family's GELU (gemm_epilogue.h): same values as the stored epilogues
                else if (p.epi == EPI_BIAS_QUICKGELU) v2 = quick_gelu2(v2);
                patch[((r & 3) + 8 * (r >> 2) + 4 * lh) * PS + l31] = v2[0];
                patch[(((r + 1) & 3) + 8 * ((r + 1) >> 2) + 4 * lh) * PS + l31] = v2[1];
                __builtin_amdgcn_sched_barrier(0);      // one pair at a time (register budget of the 128-VGPR configurations)
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // the wave's own LDS writes, then its reads
            f32x4 v4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v4[q] = *reinterpret_cast<const f32x4*>(patch + rr * PS + hh * 16 + q * 4);
            float am = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) am = fmaxf(am, fabsf(v4[q][e]));
            am = fmaxf(am, __shfl_xor(am, 1));
            const unsigned e8 = mx_scale_byte(am);
            const float inv = mx_inv_scale(e8);
            uint4 o;
            o.x = pack4_fp8(v4[0][0] * inv, v4[0][1] * inv, v4[0][2] * inv, v4[0][3] * inv);
            o.y = pack4_fp8(v4[1][0] * inv, v4[1][1] * inv, v4[1][2] * inv, v4[1][3] * inv);
            o.z = pack4_fp8(v4[2][0] * inv, v4[2][1] * inv, v4[2][2] * inv, v4[2][3] * inv);
            o.w = pack4_fp8(v4[3][0] * inv, v4[3][1] * inv, v4[3][2] * inv, v4[3][3] * inv);
            const int row = row0 + rr;
            if (row < p.M) {
                *reinterpret_cast<uint4*>(C8 + (long)row * p.ldc + col0 + hh * 16) = o;
                if (hh == 0) p.mxc[mx_scale_offset(row, col0 >> 5, p.mxc_rows)] = (unsigned char)e8;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // reads done before the next tile overwrites the patch
        }
}
template <int BM, int BN, int WM, int WN, int STAGES, int MINW, int RB = 128>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64, MINW) void gemm_mx8_kernel(GemmParams p) {
    __shared__ __attribute__((aligned(1024))) char smem[mx8_tile_lds<BM, BN, STAGES, RB>()];
    mx8_tile_body<BM, BN, WM, WN, STAGES, RB>(p, blockIdx.x, smem);
}

// ---- tile configurations of the three families (gemm_tuner.h: kCfgsB, kCfgsF8, kCfgsMx) -----------------------------------------------
static hipError_t launch_cfg_b(int c, const GemmParams& p, hipStream_t s) {
    const int nb = tile_blocks(kCfgsB[c].bm, kCfgsB[c].bn, p);
    switch (c) {
        case 0: FERN_LAUNCH((gemm_bf16_glds_kernel<128, 128, 64, 64, 32, 2, 4>), dim3(nb), dim3(256), 0, s, p); break;
        case 1: FERN_LAUNCH((gemm_bf16_glds_kernel<256, 128, 64, 64, 32, 3, 2>), dim3(nb), dim3(512), 0, s, p); break;
        case 2: FERN_LAUNCH((gemm_bf16_glds_kernel<256, 256, 64, 64, 32, 3, 1>), dim3(nb), dim3(1024), 0, s, p); break;
        case 3: FERN_LAUNCH((gemm_bf16_glds_kernel<64, 128, 32, 64, 32, 2, 4>), dim3(nb), dim3(256), 0, s, p); break;
        case 4: FERN_LAUNCH((gemm_bf16_glds_kernel<128, 64, 64, 32, 32, 2, 4>), dim3(nb), dim3(256), 0, s, p); break;
        case 5: FERN_LAUNCH((gemm_bf16_glds_kernel<64, 64, 32, 32, 32, 2, 4>), dim3(nb), dim3(256), 0, s, p); break;
        case 6: FERN_LAUNCH((gemm_bf16_glds_kernel<128, 128, 64, 64, 64, 2, 2>), dim3(nb), dim3(256), 0, s, p); break;
        case 7: return launch_gemm_pp(false, p, s);
        case 8: FERN_LAUNCH((gemm_bf16_glds_kernel<64, 64, 32, 32, 64, 3, 3>), dim3(nb), dim3(256), 0, s, p); break;
        case 9: FERN_LAUNCH((gemm_bf16_glds_kernel<64, 128, 32, 64, 64, 3, 2>), dim3(nb), dim3(256), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
static hipError_t launch_cfg_f8(int c, const GemmParams& p, hipStream_t s) {
    const int nb = tile_blocks(kCfgsF8[c].bm, kCfgsF8[c].bn, p);
    switch (c) {
        case 0: FERN_LAUNCH((gemm_bf16_glds_kernel<128, 128, 64, 64, 64, 2, 4, true>), dim3(nb), dim3(256), 0, s, p); break;
        case 1: FERN_LAUNCH((gemm_bf16_glds_kernel<256, 128, 64, 64, 64, 3, 2, true>), dim3(nb), dim3(512), 0, s, p); break;
        case 2: FERN_LAUNCH((gemm_bf16_glds_kernel<256, 256, 64, 64, 64, 3, 1, true>), dim3(nb), dim3(1024), 0, s, p); break;
        case 3: FERN_LAUNCH((gemm_bf16_glds_kernel<64, 128, 32, 64, 64, 2, 4, true>), dim3(nb), dim3(256), 0, s, p); break;
        case 4: FERN_LAUNCH((gemm_bf16_glds_kernel<128, 64, 64, 32, 64, 2, 4, true>), dim3(nb), dim3(256), 0, s, p); break;
        case 5: FERN_LAUNCH((gemm_bf16_glds_kernel<64, 64, 32, 32, 64, 2, 4, true>), dim3(nb), dim3(256), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
static hipError_t launch_cfg_mx(int c, const GemmParams& p, hipStream_t s) {
    const int nb = tile_blocks(kCfgsMx[c].bm, kCfgsMx[c].bn, p);
    switch (c) {
        case 0: FERN_LAUNCH((gemm_mx8_kernel<128, 128, 64, 64, 2, 2>), dim3(nb), dim3(256), 0, s, p); break;
        case 1: FERN_LAUNCH((gemm_mx8_kernel<256, 128, 64, 64, 2, 2>), dim3(nb), dim3(512), 0, s, p); break;
        case 2: FERN_LAUNCH((gemm_mx8_kernel<256, 128, 128, 64, 2, 1>), dim3(nb), dim3(256), 0, s, p); break;
        case 3: FERN_LAUNCH((gemm_mx8_kernel<128, 128, 64, 64, 3, 1>), dim3(nb), dim3(256), 0, s, p); break;
        case 4: FERN_LAUNCH((gemm_mx8_kernel<64, 128, 32, 64, 2, 3>), dim3(nb), dim3(256), 0, s, p); break;
        case 5: FERN_LAUNCH((gemm_mx8_kernel<128, 64, 64, 32, 2, 3>), dim3(nb), dim3(256), 0, s, p); break;
        case 6: FERN_LAUNCH((gemm_mx8_kernel<64, 64, 32, 32, 2, 4>), dim3(nb), dim3(256), 0, s, p); break;
        case 7: FERN_LAUNCH((gemm_mx8_kernel<256, 256, 64, 64, 2, 1>), dim3(nb), dim3(1024), 0, s, p); break;
        case 8: FERN_LAUNCH((gemm_mx8_kernel<128, 128, 64, 64, 3, 3, 64>), dim3(nb), dim3(256), 0, s, p); break;
        case 9: FERN_LAUNCH((gemm_mx8_kernel<256, 128, 64, 64, 3, 4, 64>), dim3(nb), dim3(512), 0, s, p); break;
        case 10: FERN_LAUNCH((gemm_mx8_kernel<256, 256, 128, 64, 4, 2, 64>), dim3(nb), dim3(512), 0, s, p); break;
        case 11: return launch_gemm_pp(true, p, s);
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

static int heuristic_b(int M, int N) {
    static const int order[] = {2, 1, 0, 3, 5};       // largest tile that still gives every CU >= 2 workgroups' worth of work
    for (int c : order) {
        const long nb = (long)((M + kCfgsB[c].bm - 1) / kCfgsB[c].bm) * ((N + kCfgsB[c].bn - 1) / kCfgsB[c].bn);
        const long per_cu = (long)kCfgsB[c].bm * kCfgsB[c].bn / (128 * 128);   // 128x128-equivalents per workgroup
        if (nb * per_cu >= 1024) return c;
    }
    return 5;
}
static int heuristic_mx(int M, int N) { return (long)((M + 127) / 128) * ((N + 127) / 128) >= 256 ? 0 : 6; }
static int first_cfg(int, int) { return 0; }

// What tells the three families apart on the host.  Per-shape tile selection is as in gemm.hip: every configuration of a family
// produces bit-identical results, so the choice is purely a speed choice; each new (M, N, K, epilogue, output form) inside the family's
// flop window is timed once on scratch outputs.
struct FamilyB {
    int family;                                                        // FAM_*: the forced configuration and the k rule (gemm_tuner.h)
    const TileCfgB* cfgs;
    hipError_t (*launch)(int c, const GemmParams& p, hipStream_t s);
    int key_bits;                                                      // the family's bits of its keys' tag
    double max_flops;                                                  // the tuning window is [2.5e8, max_flops]
    int (*untuned)(int M, int N);                                      // the configuration of a shape outside the window
    int (*fallback)(int M, int N);                                     // ... and of a shape inside it whose trials cannot run
};
static const FamilyB kFamiliesB[3] = {{FAM_BF16, kCfgsB, launch_cfg_b, 0, 1.6e12, heuristic_b, heuristic_b},
                                      {FAM_FP8, kCfgsF8, launch_cfg_f8, 2, HUGE_VAL, first_cfg, first_cfg},
                                      {FAM_MX8, kCfgsMx, launch_cfg_mx, 4, HUGE_VAL, heuristic_mx, first_cfg}};
static const FamilyB& family_of(const GemmParams& p) { return kFamiliesB[p.fp8 == 2 ? 2 : p.fp8 ? 1 : 0]; }
static ShapeKey shape_key_b(const GemmParams& p) {
    return ShapeKey{p.M, p.N, p.K, p.epi, p.out_bf16 | family_of(p).key_bits | (p.fp8 == 2 && p.out_mx8 ? 8 : 0)};
}

// With several batches in flight (fern_tuner_set_concurrency) a launch that leaves workgroup slots free is cheaper than its isolated time:
// the other lanes' kernels run in them.  The tuner scores a candidate as time x share^e, share = the fraction of the chip's slots it fills.
static double share_exponent() {
    static const double expo = [] { const char* e = getenv("FERN_TUNE_SHARE_EXP"); return e ? atof(e) : 0.75; }();      // A/B knob (tools/c5_exp_ab.sh: 0 = latency score 17.9-18.3 k queries/s on c5, 0.5 ... 1.5 all 19.2-19.5 k)
    return expo;
}

// The trials of a shape (lookup_or_tune: `tuned`, and the caller holds the store's lock).  Rounds outermost: two rounds, each candidate
// keeps its faster time (the first launches after an idle spell run on ramping clocks).
static int tune_shape_b(const FamilyB& fam, const GemmParams& p, hipStream_t s, bool& tuned) {
    tuned = false;
    const int fallback = fam.fallback(p.M, p.N);
    if (!tuning_enabled()) return fallback;
    TrialTimer timer(s);
    GemmParams q = p;
    q.C = static_cast<float*>(timer.scratch((size_t)p.M * p.ldc * sizeof(float)));      // the residual input is only read: tuning has no side effects on the caller's buffers
    if (!timer.ok()) return fallback;
    if (p.out_mx8) { q.mxc = reinterpret_cast<unsigned char*>(q.C) + (size_t)p.M * p.ldc; q.mxc_rows = p.M; }   // bytes [M*ldc, M*ldc + M*N/32)
    const int ncand = kFamilies[fam.family].ncfg;
    float t[16];
    for (float& v : t) v = 1e30f;
    for (int round = 0; round < 2; ++round)
        for (int c = 0; c < ncand; ++c)
            if (cfg_fits(fam.family, c, p.K)) t[c] = std::min(t[c], timer.best_ms([&] { return fam.launch(c, q, s); }, 1, 2));
    const int conc = choice_store().concurrency;
    int best = fallback;
    float best_ms = 1e30f;
    for (int c = 0; c < ncand; ++c) {
        if (t[c] > 1e29f) continue;
        float score = t[c];
        if (conc > 1) {
            const double nwg = tile_blocks(fam.cfgs[c].bm, fam.cfgs[c].bn, p);
            const double share = std::min(1.0, nwg / (256.0 * fam.cfgs[c].per_cu));
            score *= (float)std::pow(share, share_exponent());
        }
        if (score < best_ms) { best_ms = score; best = c; }
    }
    tuned = best_ms < 1e29f;
    return best;
}

// the argument checks of the family (launch_gemm_bf16 and the pair launcher below)
static bool rp_args_ok(const GemmParams& p) {
    const int kq = p.fp8 == 2 ? 128 : p.fp8 ? 64 : 32, aq = p.fp8 ? 15 : 7;
    if (p.K <= 0 || (p.K % kq) != 0 || (p.lda & aq) || (p.ldw & aq) || p.aload != ALOAD_PLAIN || epi_is_reduce(p.epi)) return false;
    if (!p.Ab || !p.Wb || ((uintptr_t)p.Ab & 15) || ((uintptr_t)p.Wb & 15)) return false;
    if ((p.scale_a == nullptr) != (p.scale_w == nullptr)) return false;
    if (p.fp8 == 2) {
        if (!p.mxa || !p.mxw || p.scale_a || ((uintptr_t)p.mxa & 3) || ((uintptr_t)p.mxw & 3) || p.mxa_rows < p.M || p.mxw_rows < p.N) return false;
        if (p.epi == EPI_BIAS_RESIDUAL && (p.out_bf16 ? !p.Rb : !p.R)) return false;
        if (p.out_mx8 && (!p.mxc || p.mxc_rows < p.M || (p.N & 31) || (p.ldc & 15) || ((uintptr_t)p.C & 15) || (p.epi != EPI_BIAS && p.epi != EPI_BIAS_GELU && p.epi != EPI_BIAS_QUICKGELU)))
            return false;
    }
    return true;
}

hipError_t launch_gemm_bf16(const GemmParams& p, hipStream_t s) {
    if (p.M <= 0 || p.N <= 0) return hipSuccess;
    if (!rp_args_ok(p)) return hipErrorInvalidValue;
    const FamilyB& fam = family_of(p);
    // the configuration: forced, else (inside the flop window) stored or tuned per shape, else the family's heuristic
    int c = forced_cfg(fam.family);
    if (!cfg_fits(fam.family, c, p.K)) {
        const double flops = 2.0 * p.M * (double)p.N * p.K;
        if (flops >= 2.5e8 && flops <= fam.max_flops)
            c = lookup_or_tune(choice_store().rp, shape_key_b(p), [&](bool& tuned) { return tune_shape_b(fam, p, s, tuned); });
        else
            c = fam.untuned(p.M, p.N);
    }
    return fam.launch(c, p, s);
}

// ---- image + text GEMM pair of the mixed mode, ONE launch (round 6) -------------------------------------------------------------------
// FERN_PREC_MX8_IMG runs the image tower's GEMMs block-scaled and the text tower's in bf16.  The text GEMMs (M = 77 B rows, K = 512) are a
// few dozen big tiles each: on their own every one of them is an 18-23 us launch that fills a fraction of the chip, while the image GEMM
// of the same layer leaves CUs idle in its last round (12608 x 768: 150 tiles of 256 x 256 on 256 CUs).  The two towers are independent until
// the fusion, so the text layer's GEMM rides in the image layer's launch: the SECOND problem's tiles come first in block order (a tail of
// long-k tiles behind the first problem's cost more than it saved in the fp32 family: gemm.hip, gemm_f32_pair_kernel), then the first
// problem's.  Both halves run the bodies of the family's own kernels on the tiles those kernels would compute, in the same k order:
// bit-identical to two launches.  V = 0: 16 waves (256 x 256 block-scaled tiles with 128-byte rows + 256 x 256 bf16 tiles); V = 1: 8 waves,
// two workgroups per CU (256 x 128 with 64-byte rows + 256 x 128 bf16).
template <int V>
__global__ __launch_bounds__(V == 0 ? 1024 : 512, V == 0 ? 1 : 4) void gemm_mxbf_pair_kernel(GemmParams p1, GemmParams p2, int n2_8) {
    constexpr int L1 = V == 0 ? mx8_tile_lds<256, 256, 2, 128>() : mx8_tile_lds<256, 128, 3, 64>();
    constexpr int L2 = V == 0 ? bf16_tile_lds<256, 256, 32, 3, false>() : bf16_tile_lds<256, 128, 32, 3, false>();
    __shared__ __attribute__((aligned(1024))) char smem[L1 > L2 ? L1 : L2];
    const int bid = blockIdx.x;
    if (bid < n2_8) {
        constexpr int BN2 = V == 0 ? 256 : 128;
        const int tiles = ((p2.M + 255) / 256) * ((p2.N + BN2 - 1) / BN2);
        if (bid >= tiles) return;
        if (V == 0) bf16_tile_body<256, 256, 64, 64, 32, 3, false>(p2, bid, smem);
        else bf16_tile_body<256, 128, 64, 64, 32, 3, false>(p2, bid, smem);
    } else {
        if (V == 0) mx8_tile_body<256, 256, 64, 64, 2, 128>(p1, bid - n2_8, smem);
        else mx8_tile_body<256, 128, 64, 64, 3, 64>(p1, bid - n2_8, smem);
    }
}
static hipError_t launch_mxbf_pair(int v, const GemmParams& p1, const GemmParams& p2, hipStream_t s) {
    const int bn = v == 0 ? 256 : 128;
    const int n1 = ((p1.M + 255) / 256) * ((p1.N + bn - 1) / bn), n2 = ((p2.M + 255) / 256) * ((p2.N + bn - 1) / bn);
    const int n2_8 = (n2 + 7) & ~7;                       // the first problem starts on a multiple of 8 blocks: block % 8 stays its XCD
    if (v == 0) FERN_LAUNCH((gemm_mxbf_pair_kernel<0>), dim3(n2_8 + n1), dim3(1024), 0, s, p1, p2, n2_8);
    else FERN_LAUNCH((gemm_mxbf_pair_kernel<1>), dim3(n2_8 + n1), dim3(512), 0, s, p1, p2, n2_8);
    return hipGetLastError();
}
// per (block-scaled shape, bf16 shape): 0 = two launches (each with its own tuned tile), 1 / 2 = the pair kernel V = 0 / 1.  Timed once on
// scratch outputs; exported / pinned / imported with the tile choices ("pairb ..." lines).  Candidates outermost: the two-launch form
// first, all of its rounds (its warm launches also tune the two shapes), then each pair form.
static int tune_pair_b(const GemmParams& p1, const GemmParams& p2, hipStream_t s, bool& timed) {
    timed = false;
    TrialTimer timer(s);
    // scratch outputs: the residual inputs are only read, so the trials have no side effects (a quantising first problem also writes scales)
    const size_t c1_bytes = (size_t)p1.M * p1.ldc * sizeof(float);
    GemmParams q1 = p1, q2 = p2;
    q1.C = static_cast<float*>(timer.scratch(c1_bytes + (p1.out_mx8 ? (size_t)p1.M * p1.N / 32 + 256 : 0)));
    q2.C = static_cast<float*>(timer.scratch((size_t)p2.M * p2.ldc * sizeof(float)));
    if (!timer.ok()) return 0;
    if (p1.out_mx8) { q1.mxc = reinterpret_cast<unsigned char*>(q1.C) + c1_bytes; q1.mxc_rows = p1.M; }
    float t[3];
    t[0] = timer.best_ms([&] { const hipError_t e = launch_gemm_bf16(q1, s); return e != hipSuccess ? e : launch_gemm_bf16(q2, s); }, 3, 3);
    t[1] = timer.best_ms([&] { return launch_mxbf_pair(0, q1, q2, s); }, 3, 3);
    t[2] = timer.best_ms([&] { return launch_mxbf_pair(1, q1, q2, s); }, 3, 3);
    if (t[0] > 1e29f) return 0;
    timed = true;
    // Which pair form: alone the two are within a few per cent of each other on the ViT shapes (the choice flipped from run to run); with four
    // batches in flight the 8-wave form costs 1 % (out-proj) to 3 % (c_proj) of the c5 step (tools/pairb_forms_ab.sh: all pairs 16-wave
    // 19.58-19.74 k queries/s, out-proj + c_proj 8-wave 18.86-19.17 k) -- its two workgroups hold 156 of a CU's 160 KiB of LDS, the 16-wave
    // form leaves 28 KiB and 16 wave slots to the other lanes' kernels.  The tile tuner's share score does not see that (both forms fill the
    // same fraction of their slots), so under concurrency the 8-wave form must win alone by 10 %.  Pair or two launches: plain times -- the
    // share score overrates what the other lanes make of a short text launch's free slots (it chose two launches for three of the four
    // pairs; measured 2-4 % below the pairs).
    const float sc[2] = {t[1], tuner_concurrency() > 1 ? t[2] * 1.10f : t[2]};
    const int form = sc[1] < sc[0] ? 2 : 1;
    return t[form] < t[0] ? form : 0;
}
// p1: a block-scaled GEMM (fp8 == 2), p2: a bf16 GEMM (fp8 == 0); one launch where a one-off timing says it wins, two otherwise
hipError_t launch_gemm_mxbf_pair(const GemmParams& p1, const GemmParams& p2, hipStream_t s) {
    g_last_dispatches = 1;
    int choice = 0;
    if (pair_enabled() && p1.fp8 == 2 && p2.fp8 == 0 && p1.M >= 256 && p2.M >= 256 && p1.N >= 256 && p2.N >= 256 && rp_args_ok(p1) && rp_args_ok(p2) &&
        forced_cfg(FAM_MX8) < 0 && forced_cfg(FAM_BF16) < 0 && tuning_enabled())
        choice = lookup_or_tune_pair(choice_store().pairb, PairKey{shape_key_b(p1), shape_key_b(p2)}, [&](bool& timed) { return tune_pair_b(p1, p2, s, timed); });
    if (choice == 1 || choice == 2) return launch_mxbf_pair(choice - 1, p1, p2, s);
    g_last_dispatches = 2;
    const hipError_t e1 = launch_gemm_bf16(p1, s);
    return e1 != hipSuccess ? e1 : launch_gemm_bf16(p2, s);
}

}  // namespace fern

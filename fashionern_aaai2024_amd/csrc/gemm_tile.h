// Tile vocabulary of the GEMM kernels, each piece defined once: the workgroup -> tile map, the geometry and bank swizzle of 64- and
// 128-byte tile rows, the clamped source row, the LDS-DMA and vmcnt wrappers, the operand vector types and the f32x3 plane split.
// Leaves only -- integer arithmetic and one-line wrappers.  No k-loop schedule lives here: which tile is staged, awaited or read when
// is each kernel's own (gemm.hip, gemm_bf16.hip, gemm_pp.h, sweep_bf16.hip), and the epilogues are gemm_epilogue.h.  Which kernels
// compile to the parent's instructions with these, and which pieces were NOT adopted where because they did not:
// profiles/gemm_tile_toolkit_ab.txt.
#pragma once
#include "gemm_epilogue.h"

namespace fern {

// ---- operand vectors (f32x16, f32x4 and f32x2 are gemm_epilogue.h's) -------------------------------------------------------------------
typedef short bf16x8 __attribute__((ext_vector_type(8)));       // 8 bf16 bit patterns: one operand of v_mfma_f32_32x32x16_bf16
typedef int i32x4 __attribute__((ext_vector_type(4)));          // one ds_read_b128 of fp8 bytes
typedef int i32x8 __attribute__((ext_vector_type(8)));          // one operand of v_mfma_scale_f32_32x32x64_f8f6f4
typedef long i64x2 __attribute__((ext_vector_type(2)));         // two operands of v_mfma_f32_32x32x16_fp8_fp8
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// ---- workgroup -> tile ---------------------------------------------------------------------------------------------------------------
// XCD-aware bijective map: workgroup `bid` runs on XCD bid % 8 (private L2), and each XCD gets a contiguous run of the n-fastest tile
// order -- the first nwg % 8 XCDs one tile more than the others -- so that the tiles an XCD works on share operand rows in its L2.
// bid in [0, ceil(M / BM) * ceil(N / BN)); wave-uniform.  nbn is the number of tile columns (the reduce epilogues index by it).
struct TileAt { int bm, bn, nbn; };
template <int BM, int BN>
__device__ __forceinline__ TileAt tile_at(int bid, int M, int N) {
    const int nbm = (M + BM - 1) / BM, nbn = (N + BN - 1) / BN;
    const int nwg = nbm * nbn;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const int swz = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    return {swz / nbn, swz % nbn, nbn};
}
// workgroups of a launch over bm x bn tiles (host)
inline int tile_blocks(int bm, int bn, const GemmParams& p) { return ((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn); }

// source row of tile row `row`: rows past the operand's end re-read its last row (their products are never stored).  The fp32 bodies
// (gemm.hip) use it.  The bodies of gemm_bf16.hip and gemm_pp.h keep the two statements spelled out: through a function the compiler
// attaches a value range to the minimum, and their register allocation changed from the prologue on (profile file, section 0).
__device__ __forceinline__ int clamp_row(int row, int limit) { return row < limit ? row : limit - 1; }

// ---- tile rows of RB = 64 or 128 bytes behind LDS-DMA ----------------------------------------------------------------------------------
// One LDS-DMA wave instruction writes 64 lanes x 16 B = 1 KiB lane-linear: a piece of RPP consecutive tile rows of C4 chunks.  The bank
// swizzle is therefore applied on the SOURCE: position c of tile row r holds the row's logical chunk c ^ ((r >> FSH) & FMASK), and a
// fragment read of logical chunk c goes to position c ^ read_swizzle (conflict-free for the 16-lane groups of ds_read_b128).
template <int RB>
struct TileRows {
    static_assert(RB == 64 || RB == 128, "tile rows are 64 or 128 bytes");
    static constexpr int C4 = RB / 16;                   // 16-byte chunks per tile row
    static constexpr int RPP = 64 / C4;                  // tile rows per 1 KiB piece
    static constexpr int FSH = RB == 64 ? 2 : 1;
    static constexpr int FMASK = C4 - 1;
    // the logical chunk lane `lane` of a piece fetches; trow = piece * RPP + lane / C4 is the lane's tile row
    static __device__ __forceinline__ int store_chunk(int lane, int trow) { return (lane & FMASK) ^ ((trow >> FSH) & FMASK); }
    // XOR of the rows l31, l31 + 32, ... a lane reads fragments of (tile-row offsets are multiples of 32: the same value for all)
    static __device__ __forceinline__ int read_swizzle(int l31) { return (l31 >> FSH) & FMASK; }
};

// ---- LDS-DMA and its wait --------------------------------------------------------------------------------------------------------------
// global_load_lds: each lane names its own source, the wave's destination is `lds` (wave-uniform) + 16 (or 4) x lane.  Size and aux must
// be literals, hence one function per form.  The data is visible to a ds_read only after the ISSUING wave's wait_vmcnt and, for other
// waves, a barrier behind it.
__device__ __forceinline__ void lds_dma16(const void* global, void* lds) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)global, (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}
__device__ __forceinline__ void lds_dma16_nt(const void* global, void* lds) {      // aux 2 = nt: bytes that are read once
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)global, (__attribute__((address_space(3))) void*)lds, 16, 0, 2);
}
__device__ __forceinline__ void lds_dma4(const void* global, void* lds) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)global, (__attribute__((address_space(3))) void*)lds, 4, 0, 0);
}
// wait until all but the N most recent vector-memory operations of this wave are done (they retire in issue order)
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ---- f32x3: eight fp32 values -> NPL bf16 planes by truncation --------------------------------------------------------------------------
// g0 / g1 are the two 16-byte chunks a lane feeds to one bf16 MFMA.  Plane 0 = the top 16 bits of x (one v_perm_b32 packs two), the
// residual x - plane 0 is exact in fp32 (one packed subtract per pair), plane 1 = its top 16 bits, ...: 8 + 8 + 8 mantissa bits.  The
// plane bits are part of the f32x3 family's results: every configuration must split through this one function.
template <int NPL>
__device__ __forceinline__ void split_bf16_planes(const f32x4& g0, const f32x4& g1, bf16x8 (&planes)[NPL]) {
    f32x2 x[4] = {{g0[0], g0[1]}, {g0[2], g0[3]}, {g1[0], g1[1]}, {g1[2], g1[3]}};
#pragma unroll
    for (int lv = 0; lv < NPL; ++lv) {
        u32x4 packed;
#pragma unroll
        for (int q2 = 0; q2 < 4; ++q2)      // bytes 2-3 of two floats -> one dword of two bf16
            packed[q2] = __builtin_amdgcn_perm(__float_as_uint(x[q2][1]), __float_as_uint(x[q2][0]), 0x07060302u);
        planes[lv] = __builtin_bit_cast(bf16x8, packed);
        if (lv + 1 < NPL) {
#pragma unroll
            for (int q2 = 0; q2 < 4; ++q2) {
                const u32x2 top = __builtin_bit_cast(u32x2, x[q2]) & 0xFFFF0000u;
                x[q2] = x[q2] - __builtin_bit_cast(f32x2, top);
            }
        }
    }
}

}  // namespace fern

// Wave (64 lanes) and workgroup primitives of the ranking kernels, each defined once: lane moves of 64-bit values, the bitonic network
// over one value per lane, integer reductions, the prefix sum of a workgroup, the two ballot appends and the leader-vote histogram add.
// No ranking policy lives here (keys, margins and the row-key rule are kernels.h and select.h).  Every piece is called by ALL lanes of
// a wave (they vote, shuffle or read lanes); the contract of each -- wave-uniform arguments, barriers inside and behind, LDS words -- is
// stated where it applies.  The float reductions (select.h's margin, row_ops.h's wave_sum) are NOT here: their order is part of a
// result's bits and stays with the result.
#pragma once
#include <hip/hip_runtime.h>

namespace fern {

typedef unsigned long long u64;
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- 64-bit lane moves ---------------------------------------------------------------------------------------------------------------
// A wave-uniform source lane is a v_readlane_b32 (SGPR lane select), the shift by one lane a DPP wave_shr:1 move: plain VALU / SALU
// latencies.  The per-lane forms go through ds_bpermute (~120 cycles each): fine once per network stage, too slow for a chain of
// dependent insertions.
__device__ __forceinline__ u64 shfl64(u64 v, int src) {       // src must be wave-uniform
    const int l = __builtin_amdgcn_readfirstlane(src);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl64v(u64 v, int src) {      // per-lane source
    const unsigned lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_xor64(u64 v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {      // lane i <- lane i - d (lanes below d keep their value)
    const unsigned lo = __shfl_up((unsigned)v, d), hi = __shfl_up((unsigned)(v >> 32), d);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 dpp_shr1_64(u64 v) {           // lane i <- lane i - 1 (lane 0 keeps its value), DPP
    const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)v, (int)(unsigned)v, 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(v >> 32), (int)(unsigned)(v >> 32), 0x138, 0xf, 0xf, false);
    return ((u64)(unsigned)hi << 32) | (unsigned)lo;
}
// the two key widths of the network below
__device__ __forceinline__ u64 lane_xor(u64 v, int m) { return shfl_xor64(v, m); }
__device__ __forceinline__ unsigned lane_xor(unsigned v, int m) { return __shfl_xor(v, m); }
__device__ __forceinline__ u64 lane_from(u64 v, int src) { return shfl64v(v, src); }
__device__ __forceinline__ unsigned lane_from(unsigned v, int src) { return __shfl(v, src); }

// ---- bitonic network, one key per lane, descending (lane 0 = largest); T = u64 or unsigned -------------------------------------------
// v holds a BITONIC sequence across the lanes: sort it with log2(64) compare-exchange stages.
template <class T>
__device__ __forceinline__ T bitonic_finish_desc(T v, int lane) {
#pragma unroll
    for (int st = 32; st >= 1; st >>= 1) {
        const T o = lane_xor(v, st);
        const bool low = (lane & st) == 0;                         // the lower lane of a pair keeps the larger key
        v = low ? (v > o ? v : o) : (v > o ? o : v);
    }
    return v;
}
// Top-64 of the union of two descending-sorted 64-entry lists: max(a[i], b[63-i]) is bitonic and holds exactly those.
template <class T>
__device__ __forceinline__ T merge_sorted_desc(T a, T b_sorted, int lane) {
    const T r = lane_from(b_sorted, 63 - lane);
    return bitonic_finish_desc(a > r ? a : r, lane);
}
// Full bitonic sort of one key per lane.
template <class T>
__device__ __forceinline__ T sort_desc(T v, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j >= 1; j >>= 1) {
            const T o = lane_xor(v, j);
            const bool desc = (lane & k) == 0 || k == 64;          // final pass: whole wave descending
            const bool low = (lane & j) == 0;
            const bool keep_max = desc ? low : !low;
            v = keep_max ? (v > o ? v : o) : (v > o ? o : v);
        }
    }
    return v;
}

// ---- integer reductions: every lane gets the wave's result ---------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_i32(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);      // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);      // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);     // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);     // row_mirror: every lane holds its 16-lane row's sum
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const unsigned o = __shfl_xor(v, m); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const unsigned o = __shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}

// ---- prefix sums ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        v += lane >= d ? t : 0;
    }
    return v;
}
// Exclusive scan of one count per thread over a workgroup of NW waves; returns the thread's offset, `total` the workgroup's sum.
// wtot: NW words of LDS.  Lane 63 of every wave publishes the wave's total, ONE barrier, then every thread adds the totals of the
// waves below its own.  No barrier behind: a caller that writes wtot again (the next scan of a loop, another use of the words)
// synchronises first.  block_scan_base is the half behind the barrier, for a caller whose own barrier stands between the two halves.
template <int NW>
__device__ __forceinline__ int block_scan_base(int incl, int v, const int* wtot, int& total) {
    const int wave = threadIdx.x >> 6;
    int base = incl - v;
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int t = wtot[w];
        base += w < wave ? t : 0;
        total += t;
    }
    return base;
}
template <int NW>
__device__ __forceinline__ int block_exclusive_scan(int v, int* wtot, int& total) {
    const int lane = threadIdx.x & 63;
    const int incl = wave_inclusive_sum(v, lane);
    if (lane == 63) wtot[threadIdx.x >> 6] = incl;
    __syncthreads();
    return block_scan_base<NW>(incl, v, wtot, total);
}

// ---- a wave appends its lanes' hits --------------------------------------------------------------------------------------------------
// To the wave's OWN segment: one compare + ballot per element, no atomics (one returning LDS atomic per hit was ~200 cycles each).
// wn (wave-uniform) counts every hit, stored or not: wn > cap afterwards means the segment overflowed.  store(pos) writes the lane's entry.
template <class Store>
__device__ __forceinline__ void wave_append(bool hit, int& wn, int cap, Store store) {
    const u64 m = __ballot(hit);
    if (m) {
        const int pos = wn + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
        if (hit && pos < cap) store(pos);
        wn += __popcll(m);
    }
}
// To a list the workgroup shares: `counter` (one LDS word, zero before the first append) counts every hit; one returning atomic per
// wave and ballot, issued by lane 0 -- the whole wave calls, from wave-uniform control flow.  *counter > cap behind the caller's
// barrier means the list overflowed.  The order of the entries depends on the order the waves arrive in.
template <class Store>
__device__ __forceinline__ void wave_append_shared(bool hit, int* counter, int cap, Store store) {
    const u64 m = __ballot(hit);
    if (m) {
        int p0 = 0;
        if ((threadIdx.x & 63) == 0) p0 = atomicAdd(counter, __popcll(m));
        p0 = __builtin_amdgcn_readlane(p0, 0);
        const int pos = p0 + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
        if (hit && pos < cap) store(pos);
    }
}

// ---- digit vote: hist[digit] += 1 for every lane with `match` ------------------------------------------------------------------------
// Keys that match a radix prefix mostly share the next digit too: the first matching lane's digit is counted by ONE atomic for all the
// lanes that hold it, the rest add singly.  (Three such rounds per wave measured slower than one.)  hist: LDS, int or unsigned.
template <class H>
__device__ __forceinline__ void wave_hist_add(bool match, int digit, H* hist) {
    const u64 m = __ballot(match);
    if (m == 0) return;
    const int leader = __ffsll((long long)m) - 1;
    const int dl = __builtin_amdgcn_readlane(digit, leader);
    const u64 same = __ballot(match && digit == dl);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[dl], (H)__popcll(same));
    if (match && digit != dl) atomicAdd(&hist[digit], (H)1);
}

}  // namespace fern

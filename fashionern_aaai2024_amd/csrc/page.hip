// Ranking pages (include/fern.h: fern_rank_select, fern_sim_topk_page): which key holds a given place of a query's ranking, at any depth.
// A radix select over the STORED score row of each query (the deep stage's S [m, ld]), spread over many workgroups per query.  The key is
// the 64-bit ranking key orderable(score) << 32 | ~global_index, searched in eight digits of eight bits, most significant first.  A place's
// STATE after digit d ("level d"; level 8 = before any digit) is {prefix = the digits fixed so far, need = the place counted among the keys
// that match the prefix, flag}.
//   select_init_kernel   level 8: {0, place + 1, searching}; need 0 = the place holds no row;
//   select_pass_kernel   digit d.  Prologue: every workgroup derives level d + 1 from level d + 2 and the summed histogram of digit d + 1
//                        (select_pick; redundantly, no kernel in between: the pick is a pure function of integer sums, so every workgroup
//                        gets the same state and the result does not depend on the order workgroups arrive in); workgroup x = 0 stores it.
//                        Walk: blockIdx.y = query, the workgroups of a query stride over its row with 16-byte loads; per place the keys that
//                        match the prefix are counted by digit value in an LDS histogram (wave.h: wave_hist_add, one atomic per wave and leading digit value), the
//                        workgroup's histograms are added into hist [m, SEL_T, 8, 256] with vector atomics.  One walk serves SEL_T places;
//                        digit 7 is counted once for all of them (no prefix is fixed yet).
//                        A place whose picked bucket held ONE key is `single`: the next walk reads that key off the row instead of
//                        counting (one writer, so still deterministic), after which the place is `found`.  A query whose places are all
//                        found (or hold no row) returns after the prologue: random scores end a walk or two early, tie floods need all 8;
//   select_emit_kernel   level 0 -> out_keys (0 for a place without a row); zeroes the query's histograms for the next call.
// Rows scoring -inf (ineligible pairs are stored so), positions past N and the query's excluded row have no key (kernels.h:
// stored_row_key).  No capacity anywhere and nothing read back.
#include "kernels.h"
#include "wave.h"

#include <algorithm>

namespace fern {

constexpr int SEL_NT = 256;               // threads per workgroup = digit values
constexpr int SEL_ROWS = SEL_NT * 4;      // row positions of one workgroup step
constexpr unsigned SEL_SEARCH = 0, SEL_SINGLE = 1, SEL_FOUND = 2;

__global__ __launch_bounds__(SEL_NT) void select_init_kernel(const int* places, int pstride, int nt, int clamp, SelectState* st, int B) {
    const int i = blockIdx.x * SEL_NT + threadIdx.x;
    if (i >= B * SEL_T) return;
    const int b = i / SEL_T, t = i % SEL_T;
    unsigned need = 0;
    if (t < nt) {
        const int p = places[(long)b * pstride + t];
        need = p >= 0 ? (unsigned)p + 1u : (clamp ? 1u : 0u);
    }
    st[i] = SelectState{0ull, need, SEL_SEARCH};
}

// Level d of one query from level d + 1 (`in`, [SEL_T]) and the summed histograms of digit d (`hq`: the query's [SEL_T, 8, 256]), into
// cur [SEL_T] (LDS).  Every thread of a 256-thread workgroup calls it; thread i = digit value i.  `found`: the query's [SEL_T] keys that
// the walk of digit d read off the row for its single places.
__device__ __forceinline__ void select_pick(const SelectState* in, const unsigned* hq, const u64* found, int nt, int d, SelectState* cur,
                                            unsigned (*wtot)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool first = d == 7;
    SelectState sv[SEL_T];
    unsigned cnt[SEL_T], incl[SEL_T];
#pragma unroll
    for (int t = 0; t < SEL_T; ++t) {
        sv[t] = in[t < nt ? t : 0];
        const bool searching = t < nt && sv[t].need != 0 && sv[t].flag == SEL_SEARCH;
        cnt[t] = searching ? hq[((first ? 0 : t) * 8 + d) * 256 + tid] : 0u;
        unsigned v = cnt[t];                   // keys of this wave with a digit value >= tid
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned o = __shfl_down(v, s);
            if (lane + s < 64) v += o;
        }
        incl[t] = v;
        if (lane == 0) wtot[t][wave] = v;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < SEL_T; ++t) {
        if (t >= nt) continue;
        const SelectState s = sv[t];
        if (s.need == 0 || s.flag != SEL_SEARCH) {      // no row / found: kept; single: the walk of digit d read the key off the row
            if (tid == 0) cur[t] = s.need != 0 && s.flag == SEL_SINGLE ? SelectState{found[t], 1u, SEL_FOUND} : s;
            continue;
        }
        unsigned above = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            above += w > wave ? wtot[t][w] : 0u;
            total += wtot[t][w];
        }
        const unsigned hi = incl[t] + above, lo = hi - cnt[t];      // keys with a digit value >= tid / > tid
        if (lo < s.need && s.need <= hi)
            cur[t] = SelectState{s.prefix | ((u64)tid << (8 * d)), s.need - lo, d == 0 ? SEL_FOUND : cnt[t] == 1 ? SEL_SINGLE : SEL_SEARCH};
        if (tid == 0 && s.need > total) cur[t] = SelectState{0ull, 0u, SEL_SEARCH};      // (only at digit 7) fewer keys in the row than the place asks for
    }
    __syncthreads();
}

// states: [9][B][SEL_T] by level; hist: [B][SEL_T][8][256]; found: [B][SEL_T]
__global__ __launch_bounds__(SEL_NT) void select_pass_kernel(const float* S, long ld, long N, const int* exclude, long idx_offset, SelectState* states,
                                                             unsigned* hist, u64* found, int nt, int d, int B) {
    __shared__ unsigned h[SEL_T][256];
    __shared__ SelectState cur[SEL_T];
    __shared__ unsigned wtot[SEL_T][4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const bool first = d == 7;                 // no digit fixed yet: every place matches the same keys, one histogram serves them all
    unsigned* hq = hist + (long)b * SEL_T * 8 * 256;
    u64* fq = found + (long)b * SEL_T;
    SelectState* level = states + ((long)(d + 1) * B + b) * SEL_T;
    if (first) {
        if (tid < SEL_T) cur[tid] = level[tid];
        __syncthreads();
    } else {
        select_pick(states + ((long)(d + 2) * B + b) * SEL_T, hq, fq, nt, d + 1, cur, wtot);
        if (blockIdx.x == 0 && tid < nt) level[tid] = cur[tid];
    }
    u64 prefix[SEL_T];
    bool count[SEL_T], single[SEL_T];
    bool any_count = false, any_single = false;
#pragma unroll
    for (int t = 0; t < SEL_T; ++t) {
        const SelectState s = cur[t < nt ? t : 0];
        prefix[t] = s.prefix;
        count[t] = t < nt && s.need != 0 && s.flag == SEL_SEARCH;
        single[t] = t < nt && s.need != 0 && s.flag == SEL_SINGLE;
        any_count |= count[t];
        any_single |= single[t];
    }
    if (!any_count && !any_single) return;     // (uniform) every place of the query is found or holds no row
    if (first) {
#pragma unroll
        for (int t = 1; t < SEL_T; ++t) count[t] = false;
        count[0] = true;
    }
    const u64 mask = first ? 0ull : ~0ull << (8 * (d + 1));
#pragma unroll
    for (int t = 0; t < SEL_T; ++t) h[t][tid] = 0;
    __syncthreads();
    const long drop = excluded_local_row(exclude, b, idx_offset, N);
    const float* row = S + (long)b * ld;
    for (long base = (long)blockIdx.x * SEL_ROWS; base < N; base += (long)gridDim.x * SEL_ROWS) {
        const long i = base + (long)tid * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + (i < N ? i : 0));      // ld % 4 == 0: the whole vector is inside the row
        u64 key[4];
        bool valid[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            valid[e] = row_takes_place(v[e], i + e, N, drop);      // stored_row_key in two halves: the key is formed unconditionally,
            key[e] = make_key(v[e], (unsigned)(i + e + idx_offset));      // `valid` gates every use of it (a select per key measured +3 %)
        }
#pragma unroll
        for (int t = 0; t < SEL_T; ++t) {
            if (single[t]) {                   // (uniform) exactly one key of the row matches: its owner stores it
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (valid[e] && (key[e] & mask) == prefix[t]) fq[t] = key[e];
                continue;
            }
            if (!count[t]) continue;           // (uniform)
            bool match[4];
            bool any = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                match[e] = valid[e] && (key[e] & mask) == prefix[t];
                any |= match[e];
            }
            if (__ballot(any) == 0) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) wave_hist_add(match[e], (int)((key[e] >> (8 * d)) & 255), h[t]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < SEL_T; ++t)
        if (count[t] && h[t][tid] != 0) atomicAdd(&hq[(t * 8 + d) * 256 + tid], h[t][tid]);
}

// One workgroup per query: level 0, out[b * ostride + t] = the place's key (0 for a place without a row), histograms zeroed.
__global__ __launch_bounds__(SEL_NT) void select_emit_kernel(const SelectState* states, unsigned* hist, const u64* found, int nt, int B, u64* out,
                                                             long ostride) {
    __shared__ SelectState cur[SEL_T];
    __shared__ unsigned wtot[SEL_T][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    unsigned* hq = hist + (long)b * SEL_T * 8 * 256;
    select_pick(states + ((long)B + b) * SEL_T, hq, found + (long)b * SEL_T, nt, 0, cur, wtot);
    if (tid < nt) out[(long)b * ostride + tid] = cur[tid].need != 0 ? cur[tid].prefix : 0ull;
    for (int i = tid; i < SEL_T * 8 * 256; i += SEL_NT) hq[i] = 0;      // every read of the query's histograms is behind the barrier in select_pick
}

hipError_t launch_rank_select(const float* S, long ld, int B, long N, const int* places, int pstride, int nt, int clamp, const int* exclude,
                              long idx_offset, SelectState* states, unsigned* hist, unsigned long long* found, unsigned long long* out_keys,
                              long ostride, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (nt < 1 || nt > SEL_T || N <= 0 || (ld & 3) || ld < N || !states || !hist || !found) return hipErrorInvalidValue;
    // ~4096 rows per workgroup and step; a lone query still spreads over the device
    const unsigned gx = (unsigned)std::min<long>(std::max<long>(1, (N + 4095) / 4096), std::max<long>(64, 2048 / B));
    FERN_LAUNCH(select_init_kernel, dim3((unsigned)((B * SEL_T + SEL_NT - 1) / SEL_NT)), dim3(SEL_NT), 0, s, places, pstride, nt, clamp,
                states + (long)8 * B * SEL_T, B);
    for (int d = 7; d >= 0; --d)
        FERN_LAUNCH(select_pass_kernel, dim3(gx, (unsigned)B), dim3(SEL_NT), 0, s, S, ld, N, exclude, idx_offset, states, hist, found, nt, d, B);
    FERN_LAUNCH(select_emit_kernel, dim3((unsigned)B), dim3(SEL_NT), 0, s, states, hist, found, nt, B, out_keys, ostride);
    return hipGetLastError();
}

}  // namespace fern

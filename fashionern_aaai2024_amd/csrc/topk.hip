// Wavefront-reduced exact top-K (K <= 64); replaces the reference's full torch.argsort of the [Q, N] distance matrix
// (run/test/test_fiq.py:50), of which only ranks < 50 (51 for CIRR) are ever consumed.
//
// Ordering = score descending, gallery index ascending.  Both are packed into one 64-bit key
//     key = orderable(score) << 32 | (0xFFFFFFFF - index)
// so a plain unsigned compare implements the whole rule and ties are deterministic.
//
// A wave keeps its current best-64 list SORTED, ONE ENTRY PER LANE.  Candidates are streamed 64 at a time (coalesced); a
// candidate enters only if it beats the list's K-th entry, so after warm-up almost every 64-wide step is a single compare +
// ballot.  An insertion is O(1) wave operations: position = popcount(ballot(list > cand)), shift the tail down one lane, drop
// the candidate in; dense batches and whole lists are merged with a bitonic network instead.
// The score matrix is never materialised: the sweep (gemm.hip EPI_TOPK_FILTER / sweep_bf16.hip) appends only the scores that
// reach a per-query bound to candidate lists; the two kernels here compute that bound from a row sample of the gallery
// (topk_sample_bound_kernel) and select the exact top-K from the lists (topk_candidates_kernel).  kernels.h: TopkFilter.
// The lane moves, the bitonic network, the wave reductions and the workgroup scan are wave.h; the excluded row and the query's
// filter words come from kernels.h's row-key rule; margins and key writers are select.h, the exact chains rescore.h.
#include "kernels.h"
#include "rescore.h"
#include "select.h"

#include <algorithm>

namespace fern {

// Offer one candidate per lane (key 0 = no candidate) to the wave's sorted list `best` (lane i = i-th best).  Few
// survivors of the threshold test are inserted one by one (O(1) wave ops each); many (list still filling) are sorted and
// merged as a batch, which costs the same whatever their number.
__device__ __forceinline__ void wave_offer(u64& best, u64 cand, int K, int lane) {
    u64 thr = shfl64(best, K - 1);
    u64 mask = __ballot(cand > thr);
    if (mask == 0) return;                                        // the common case after warm-up: nothing beats the K-th entry
    if (__popcll(mask) > 6) {
        best = merge_sorted_desc(best, sort_desc(cand, lane), lane);
        return;
    }
    while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        const u64 c = shfl64(cand, src);
        mask &= mask - 1;
        if (c > thr) {                                            // wave-uniform
            const int pos = __popcll(__ballot(best > c));        // entries that stay ahead of c
            const u64 up = dpp_shr1_64(best);
            best = lane < pos ? best : (lane == pos ? c : up);
            thr = shfl64(best, K - 1);
        }
    }
}

// merge R per-shard lists given as (score, global idx) pairs [R,B,K]
__global__ __launch_bounds__(64) void topk_merge_kernel(const float* scores, const int* idx, float* out_scores, int* out_idx, int R,
                                                        int B, int K) {
    const int b = blockIdx.x, lane = threadIdx.x;
    u64 best = 0;
#pragma unroll 1
    for (int r = 0; r < R; ++r) {
        u64 cand = 0;
        if (lane < K) {
            const long o = ((long)r * B + b) * K + lane;
            const int gi = idx[o];
            if (gi >= 0) cand = make_key(scores[o], (unsigned)gi);
        }
        wave_offer(best, cand, K, lane);
    }
    if (lane < K) write_key(best, 0, out_scores + (long)b * K + lane, out_idx + (long)b * K + lane);
}

// ---- fused sweep + selection (kernels.h: TopkFilter) -----------------------------------------------------------------
// Both kernels here need "the k-th largest of n keys" for n in the thousands, once per query.  Streaming the keys through the
// sorted wave lists cost 25-55 us (every early candidate is an insertion), a radix select with LDS histograms was no better
// (cosine scores share their top bytes: thousands of LDS atomics on a handful of bins serialise).  What is used instead is
// BISECTION BY COUNTING on keys held in registers: each of the 256 threads keeps <= PER keys, a step counts the keys >= a probe
// (PER compares per thread, a DPP wave sum, four partial sums through LDS, one barrier) and halves the range, which starts at
// [min, max] of the keys -- so the step count is log2 of the keys' spread, not of the key width.  Keys are 64-bit = hi
// (orderable score) << 32 | lo (~index): first the hi word, then lo among the keys that share the k-th hi (usually one key).
// (The wave reductions, the scan and the bitonic network used from here on are wave.h.)
// Workgroup helper (NW waves): `red` is 4 * NW words of LDS; `step` alternates the half used so that one barrier per
// reduction is enough (a wave can only reach step + 2 after every wave has read step's sums).
template <int NW>
struct WgReduce {
    int* red;
    int step;
    __device__ __forceinline__ int sum(int local) {
        const int s = wave_sum_i32(local);
        int* slot = red + (step & 1) * NW;
        if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = s;
        __syncthreads();
        ++step;
        int t = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += slot[w];
        return t;
    }
    __device__ __forceinline__ unsigned min(unsigned local) {
        const unsigned s = wave_min_u32(local);
        unsigned* slot = reinterpret_cast<unsigned*>(red) + 2 * NW + (step & 1) * NW;
        if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = s;
        __syncthreads();
        ++step;
        unsigned t = 0xFFFFFFFFu;
#pragma unroll
        for (int w = 0; w < NW; ++w) t = slot[w] < t ? slot[w] : t;
        return t;
    }
    __device__ __forceinline__ unsigned max(unsigned local) { return ~min(~local); }
};
// Fast path of the selection below.  A bisection step is mostly its barrier (LDS write, barrier, LDS read: ~350 ns with 4 waves,
// more with 16), and 30-odd steps made the bound and select kernels 14-23 us each.  Instead: every wave sorts its 64 lane maxima
// (registers only) and publishes the ceil(k / NW)-th largest; the minimum L0 of those NW values has at least k keys at or above it
// (ceil(k / NW) lanes of every wave hold one), so the k-th largest key lies among the keys with hi >= L0 -- typically a few more
// than k of the thousands.  Those are compacted into LDS (one prefix sum) and ranked by counting (every candidate reads the
// compact list once, broadcast reads): the candidate with k - 1 keys above it is the answer.  Four barriers in all.  More than
// CAPF candidates (tie-heavy galleries: thousands of keys share the k-th score) fall back to the bisection.
constexpr int SELECT_CAPF = 512;
// returns true and the k-th largest key in `out` when the fast path applies; every thread must call it (barriers inside);
// ck: SELECT_CAPF keys of LDS, red: 4 * NW + 8 ints of LDS.  The caller has checked that at least k keys exist.
template <int PER, int NW, class LoOf>
__device__ __forceinline__ bool select_kth_fast(const unsigned (&h)[PER], LoOf lo_of, int k, u64* ck, int* red, u64& out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned tmax = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) tmax = h[j] > tmax ? h[j] : tmax;
    const unsigned sorted = sort_desc(tmax, lane);
    const int tw = (k + NW - 1) / NW;                                   // <= 64: k <= 64
    const unsigned vw = (unsigned)__builtin_amdgcn_readlane((int)sorted, tw - 1);
    unsigned* ured = reinterpret_cast<unsigned*>(red);
    if (lane == 0) ured[wave] = vw;
    __syncthreads();
    unsigned l0 = 0xFFFFFFFFu;
#pragma unroll
    for (int w = 0; w < NW; ++w) l0 = ured[w] < l0 ? ured[w] : l0;
    l0 = l0 == 0 ? 1u : l0;                                             // 0 marks an empty slot, never a candidate
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) cnt += h[j] >= l0;
    int total;
    int base = block_exclusive_scan<NW>(cnt, red + NW, total);
    if (total > SELECT_CAPF) return false;                               // uniform
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (h[j] >= l0) ck[base++] = ((u64)h[j] << 32) | lo_of(j);
    if (tid == 0) { red[2 * NW] = 0; red[2 * NW + 1] = 0; }
    __syncthreads();
    for (int i = tid; i < total; i += NW * 64) {
        const u64 key = ck[i];
        int rank = 0;
        for (int j = 0; j < total; ++j) rank += ck[j] > key;
        if (rank == k - 1) { red[2 * NW] = (int)(unsigned)key; red[2 * NW + 1] = (int)(unsigned)(key >> 32); }
    }
    __syncthreads();
    out = ((u64)(unsigned)red[2 * NW + 1] << 32) | (unsigned)red[2 * NW];
    __syncthreads();                                                     // red / ck may be reused by the caller
    return true;
}

// k-th largest (k >= 1) of the workgroup's keys: thread-local hi words h[0..PER) (0 = empty slot) and lo words from lo_of(j).
// Returns 0 when fewer than k keys exist.  Every thread of the workgroup (NW waves) must call it (barriers inside).  `ck`:
// SELECT_CAPF keys of LDS for the fast path (null: bisection only); red: 4 * NW + 8 ints.
// HAVE_K: the caller knows that at least k keys exist (skips the count and its barrier).
template <int PER, int NW, bool HAVE_K = false, class LoOf>
__device__ __forceinline__ u64 select_kth_largest(const unsigned (&h)[PER], LoOf lo_of, int k, int* red, u64* ck = nullptr) {
    WgReduce<NW> wg{red, 0};
    if (!HAVE_K) {
        int nv = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) nv += h[j] != 0;
        if (wg.sum(nv) < k) return 0;
    }
    if (ck) {
        if (!HAVE_K) __syncthreads();                                    // the reduction above is done with `red`
        u64 fast;
        if (select_kth_fast<PER, NW>(h, lo_of, k, ck, red, fast)) return fast;
        wg.step = 0;
    }
    unsigned mn = 0xFFFFFFFFu, mx = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        mn = (h[j] != 0 && h[j] < mn) ? h[j] : mn;
        mx = h[j] > mx ? h[j] : mx;
    }
    unsigned lo = wg.min(mn), hi = wg.max(mx);
    while (lo < hi) {                                     // largest v with count(h >= v) >= k
        const unsigned mid = lo + (unsigned)(((u64)hi - lo + 1) >> 1);
        int c = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) c += h[j] >= mid;
        if (wg.sum(c) >= k) lo = mid;
        else hi = mid - 1;
    }
    const unsigned kh = lo;
    // among the keys with hi == kh, the r-th largest lo (r = k - #keys with a larger hi)
    int gt = 0;
    unsigned lmn = 0xFFFFFFFFu, lmx = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        gt += h[j] > kh;
        if (h[j] == kh) {
            const unsigned l = lo_of(j);
            lmn = l < lmn ? l : lmn;
            lmx = l > lmx ? l : lmx;
        }
    }
    const int r = k - wg.sum(gt);
    unsigned llo = wg.min(lmn), lhi = wg.max(lmx);
    while (llo < lhi) {
        const unsigned mid = llo + (unsigned)(((u64)lhi - llo + 1) >> 1);
        int c = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) c += (h[j] == kh) && lo_of(j) >= mid;
        if (wg.sum(c) >= r) llo = mid;
        else lhi = mid - 1;
    }
    return ((u64)kh << 32) | llo;
}

// Step 2: one workgroup per query keeps that query's SAMPLE scores (S columns; column c is gallery row sample_row(c, R)) in
// registers -- 1024 threads, thread t holds columns t, t + 1024, ... (four waves per SIMD keep the compare stream dense) -- and publishes the K-th best key as the query's bound.  Sample columns
// are in gallery order, so a key built from the column index ranks ties like one built from the row; the published key carries
// the real row.  Fewer than K sample rows -> bound 0 (accept all).  Also resets the query's list counters.
// NT threads: 256 (four waves: a barrier among them is a fraction of the 16-wave one, and a bisection step is mostly barrier) for
// samples of <= 4096 rows, 1024 for the larger ones (registers: PER keys per thread).
// Pre-filter form (margin.q != null; api.hip: fern_sim_topk_prefiltered): the sample scores are the bf16 sweep's approximations, and the
// sample's K-th best is <= T~ (select.h has the argument), so the bound published for the sweep is (sample K-th best) - margin as a key
// with the lowest index part; margin_out[b] keeps the margin for the rescoring kernel.
struct BoundMargin {
    const float* q;          // [B, D] fp32 queries (null: no margin -- the sample scores ARE the ranking scores)
    int D;
    const float* meta;       // fern_gallery_prepare: {E, G~, G}
    float* margin_out;       // [B]
};

template <int PER, int NT>
__global__ __launch_bounds__(NT) void topk_sample_bound_kernel(const float* scores, long ld, long S, int R, int K, const int* exclude,
                                                                long exclude_off, u64* thr_key, int* count, int* flags, int* state, BoundMargin mg) {
    __shared__ int red[80];
    __shared__ u64 ck[SELECT_CAPF];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = scores + (long)b * ld;
    float margin = 0.f;
    if (mg.q) {
        margin = margin_finish<NT / 64>(margin_accumulate<NT>(mg.q + (long)b * mg.D, mg.D), mg.D, mg.meta, reinterpret_cast<float*>(red));
        if (tid == 0) mg.margin_out[b] = margin;
        __syncthreads();                                 // the selection below reuses red
    }
    // sample column of the excluded gallery row (if it was sampled at all): it must not count towards the K rows of the bound
    long drop = -1;
    if (exclude) {
        const long er = (long)exclude[b] - exclude_off;
        if (er >= 0 && er / R < S && sample_row(er / R, R) == er) drop = er / R;
    }
    unsigned h[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const long c = tid + (long)NT * j;
        float v = -INFINITY;
        if (c < S && c != drop) v = row[c];
        h[j] = v == -INFINITY ? 0u : orderable(v);                          // -inf marks padding
    }
    for (int i = tid; i < RANK_SLOTS; i += NT) count[(long)b * RANK_SLOTS + i] = 0;
    const u64 kth = select_kth_largest<PER, NT / 64>(h, [&](int j) { return 0xFFFFFFFFu - (unsigned)(tid + NT * j); }, K, red, ck);
    if (tid == 0) {
        u64 out = 0;
        if (kth != 0) {
            const long c = (long)(0xFFFFFFFFu - (unsigned)kth);
            out = (kth & 0xFFFFFFFF00000000ull) | (u64)(0xFFFFFFFFu - (unsigned)sample_row(c, R));
            if (mg.q) {      // certified pre-filter: lowered by the margin, index part = lowest (every row with that score passes)
                const float lowered = unorderable((unsigned)(kth >> 32)) - margin;
                out = lowered == lowered ? (u64)orderable(lowered) << 32 : 0ull;      // NaN margin: accept all
            }
        }
        thr_key[b] = out;
        state[b] = 0;                      // 0: ranked by the select kernel; 1: lists overflowed -> exact pass; also its done-counter
        state[gridDim.x + b] = 0;
        if (b == 0) { flags[0] = 0; flags[1] = 0; }
    }
}

// Final step: one workgroup per query.  Thread t owns list t; a wave's 64 lists are read with one wave-wide load each and their
// keys dealt round-robin over the 256 threads' registers (LDS as the exchange), the K-th best key comes from the counting
// bisection, the K keys that reach it are collected and one bitonic sort of <= 64 keys writes the ranking.  More than CAND_MAX
// candidates (lists near full) take the streaming path.
constexpr int CAND_PER = 24;                    // keys per thread
constexpr int CAND_MAX = CAND_PER * 256;        // 6144 keys x 8 bytes of LDS
// A query's candidate lists -> the 256 threads' registers, for both select kernels.  Thread t owns list t.
//   begin   the list's count (clamped to the capacity), the wave's overflow vote and prefix sum -> wtotal / over (LDS; the caller's barrier
//           follows).  SPEC > 0: the list's first SPEC entries are requested together with its count (entries past the count are stale
//           and dropped later): one round trip instead of two for the ~K R / 256 entries a list typically holds;
//   overflow / total   after that barrier.  overflow: more rows reached the sampled bound than a list holds (a sample that missed a
//           cluster of good rows, a gallery of near-ties) -- the query goes to the exact pass (rank_exact_kernel: no capacity anywhere);
//   finish  (total <= CAND_MAX) every thread walks ITS list, eight independent loads in flight per round -- lists hold ~K * R / 256 <= 16
//           keys, so this is one or two round trips -- and drops the keys at its prefix-sum offset in c_key; then the keys are dealt
//           round-robin: mine[j] = key tid + 256 j (0 past the total), h[j] its score word.  One barrier inside, none behind.
template <int SPEC>
struct CandGather {
    const u64* mylist;
    const int *wtotal, *over;
    u64 first[SPEC > 0 ? SPEC : 1];
    int cnt, incl;
    __device__ __forceinline__ void begin(const TopkFilter& f, int b, int* wtotal_s, int* over_s) {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        mylist = f.cand + ((long)b * RANK_SLOTS + tid) * f.cap;
        wtotal = wtotal_s;
        over = over_s;
#pragma unroll
        for (int u = 0; u < SPEC; ++u) first[u] = u < f.cap ? mylist[u] : 0;
        const int cnt_raw = f.count[(long)b * RANK_SLOTS + tid];
        cnt = cnt_raw < f.cap ? cnt_raw : f.cap;
        const bool overflow_w = __any(cnt_raw > f.cap);
        incl = wave_inclusive_sum(cnt, lane);
        if (lane == 63) { wtotal_s[wave] = incl; over_s[wave] = overflow_w ? 1 : 0; }
    }
    __device__ __forceinline__ bool overflow() const { return (over[0] | over[1] | over[2] | over[3]) != 0; }
    __device__ __forceinline__ int total() const { return wtotal[0] + wtotal[1] + wtotal[2] + wtotal[3]; }
    __device__ __forceinline__ void finish(u64* c_key, int total, u64 (&mine)[CAND_PER], unsigned (&h)[CAND_PER]) const {
        const int tid = threadIdx.x;
        int sum;
        const int base = block_scan_base<4>(incl, cnt, wtotal, sum);      // (begin published the wave totals; the caller's barrier is between)
#pragma unroll
        for (int u = 0; u < SPEC; ++u)
            if (u < cnt) c_key[base + u] = first[u];
        const int maxc = (int)wave_max_u32((unsigned)cnt);                // cnt >= 0
#pragma unroll 1
        for (int e0 = SPEC; e0 < maxc; e0 += 8) {
            u64 key[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) key[u] = e0 + u < cnt ? mylist[e0 + u] : 0;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (e0 + u < cnt) c_key[base + e0 + u] = key[u];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CAND_PER; ++j) {
            const int i = tid + 256 * j;
            mine[j] = i < total ? c_key[i] : 0;
            h[j] = (unsigned)(mine[j] >> 32);
        }
    }
};

__global__ __launch_bounds__(256) void topk_candidates_kernel(TopkFilter f, int K, long idx_offset, float* out_scores, int* out_idx,
                                                              int* flags, int* state) {
    __shared__ u64 c_key[CAND_MAX];
    __shared__ int red[32];
    __shared__ u64 lists[4][64];
    __shared__ int wtotal[4], over[4], nsel;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    CandGather<0> gather;                                // (no speculative loads here)
    gather.begin(f, b, wtotal, over);
    if (tid == 0) nsel = 0;
    __syncthreads();
    if (gather.overflow()) {
        if (tid == 0) { state[b] = 1; flags[0] = 1; }
        return;
    }
    const int total = gather.total();
    u64 best = 0;                                        // wave 0 ends up with the sorted top-64 (lane i = i-th best)
    if (total <= CAND_MAX) {
        u64 mine[CAND_PER];
        unsigned h[CAND_PER];
        gather.finish(c_key, total, mine, h);
        const int want = total < K ? total : K;          // fewer candidates than K: all of them rank
        u64 kth = 0;
        __syncthreads();                                 // every thread holds its keys in registers: c_key's head becomes the fast path's compact list
        if (total > 64) kth = select_kth_largest<CAND_PER, 4>(h, [&](int j) { return (unsigned)mine[j]; }, want, red, c_key);
#pragma unroll
        for (int j = 0; j < CAND_PER; ++j) {
            if (mine[j] != 0 && mine[j] >= kth) {
                const int p = atomicAdd(&nsel, 1);
                if (p < 64) lists[0][p] = mine[j];
            }
        }
        __syncthreads();
        if (wave != 0) return;
        const int ns = nsel < 64 ? nsel : 64;
        best = sort_desc(lane < ns ? lists[0][lane] : 0, lane);
    } else {
        // streaming path (lists near full: > CAND_MAX candidates): the sorted wave lists of wave_offer
        const u64* cand = f.cand + (long)b * RANK_SLOTS * f.cap;
#pragma unroll 1
        for (int j = 0; j < 64; ++j) {
            const int n = __builtin_amdgcn_readlane(gather.cnt, j);
            wave_offer(best, lane < n ? cand[(long)(wave * 64 + j) * f.cap + lane] : 0, K, lane);
        }
        lists[wave][lane] = best;
        __syncthreads();
        if (wave != 0) return;
#pragma unroll 1
        for (int w = 1; w < 4; ++w) best = merge_sorted_desc(best, lists[w][lane], lane);
    }
    if (lane < K) write_key(best, idx_offset, out_scores + (long)b * K + lane, out_idx + (long)b * K + lane);
}

// ---- certified pre-filter: select on the approximate keys, then rescore the survivors exactly ---------------------------------------
// Final step of fern_sim_topk_prefiltered.  The candidate lists hold APPROXIMATE keys (bf16 sweep scores s~) of every row with
// s~ >= (sample bound) - margin.  Per query (one workgroup): gather the lists as topk_candidates_kernel does, T~ = the K-th best
// approximate score (exact, of the whole gallery: every row at or above the sample bound is in the lists), keep the rows with
// s~ >= T~ - margin -- a superset of the exact top-K (topk_sample_bound_kernel's comment has the argument) -- and give each survivor
// its EXACT fp32 score: one sequential v_fma_f32 chain per (query, row) in the k order of the fp32 MFMA kernels (8g, 8g+4, 8g+1, 8g+5,
// ...: oracle/chain.c), i.e. bit for bit the score fern_sim_topk's sweep produces.  The exact keys are then ranked.  Output = the
// exact top-K with the exact scores; the approximate scores decide nothing but which ~K + (rows within the margin) rows get rescored.
// Rescoring loads are COALESCED: a wave takes 64 survivors at a time and walks D in 64-float chunks; 16 lanes fetch one row's 256-byte
// chunk (4 rows per load instruction), the chunk tile [64 rows][64 k] is transposed through the wave's LDS tile and lane l then runs
// survivor l's chain over its 64 k.  (One lane loading its own row touches 64 cache lines per instruction: 8x the address work.)
// Anything without room -- a list overflow, more than CAND_MAX candidates, more than RESC_MAX survivors (galleries of near-ties) --
// goes to the exact pass (rank_exact_kernel on the fp32 gallery), whose bound (sample bound - margin) is a valid lower bound of the
// exact K-th best too.
constexpr int RESC_MAX = 1024;                  // survivors per query that are rescored here
constexpr int RESC_PER = RESC_MAX / 256;
constexpr int RESC_TILE_FLOATS = 4 * 2 * RESC_ROWS * RESC_TLD;      // the four waves' tiles, double buffered


// Exact scores of the survivors surv[0..ns) of query row `qrow` (LDS) and their ranking: the tail shared by the two rescoring
// kernels.  Every thread of the 256-thread workgroup calls it.  A wave takes 32 survivors per round (rescore_rows).
// Ranking: every thread counts the keys above its survivor's key (LDS broadcast reads) and writes rank < K straight to its slot -- no
// second selection, no sort.  D % 64 == 0.
__device__ __forceinline__ void rescore_and_rank(const unsigned* surv, int ns, const float* qrow, const float* gallery, int D, float* tiles,
                                                 u64* x_key, int K, long idx_offset, float* out_scores, int* out_idx) {
    const int tid = threadIdx.x, wave = tid >> 6;
    float* tl = tiles + wave * (2 * RESC_ROWS * RESC_TLD);
    for (int s0 = wave * RESC_ROWS; s0 < ns; s0 += 4 * RESC_ROWS) rescore_keys(surv, s0, ns, qrow, gallery, D, tl, x_key);
    if (tid < 4) x_key[ns + tid] = 0;                // the counting loop reads four keys at a time: zeros never count (x_key holds RESC_MAX + 4)
    __syncthreads();
    // rank by counting: keys are distinct (the index is part of the key); four keys per pair of LDS reads
    for (int i = tid; i < ns; i += 256) {
        const u64 key = x_key[i];
        int rank = 0;
        for (int j0 = 0; j0 < ns; j0 += 4) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(x_key + j0), c = *reinterpret_cast<const ulonglong2*>(x_key + j0 + 2);
            rank += (a.x > key) + (a.y > key) + (c.x > key) + (c.y > key);
        }
        if (rank < K) write_row(key, idx_offset, out_scores + rank, out_idx + rank);
    }
    for (int r = ns + tid; r < K; r += 256) write_key(0, idx_offset, out_scores + r, out_idx + r);      // fewer survivors than K: the gallery ran out
}

static_assert(RESC_TILE_FLOATS * 4 <= CAND_MAX * 8, "the four waves' (double-buffered) tiles overlay the candidate keys");
__global__ __launch_bounds__(256) void topk_rescore_kernel(TopkFilter f, const float* q, const float* gallery, int D, const float* margin_in, int K,
                                                           long idx_offset, float* out_scores, int* out_idx, int* flags, int* state) {
    __shared__ __attribute__((aligned(16))) u64 c_key[CAND_MAX];      // candidates (approximate keys); then select_kth_fast's compact list; then the waves' tiles
    __shared__ __attribute__((aligned(16))) u64 x_key[RESC_MAX + 4];      // exact keys of the survivors
    __shared__ unsigned surv[RESC_MAX];         // gallery rows of the survivors
    __shared__ __attribute__((aligned(16))) float qrow[1024];
    __shared__ int red[32];
    __shared__ int wtotal[4], over[4], nsurv;
    const int b = blockIdx.x, tid = threadIdx.x;
    CandGather<8> gather;
    gather.begin(f, b, wtotal, over);
    if (tid == 0) nsurv = 0;
    for (int i = tid; i < D; i += 256) qrow[i] = q[(long)b * D + i];
    __syncthreads();
    const int total = gather.total();
    if (gather.overflow() || total > CAND_MAX) {
        if (tid == 0) { state[b] = 1; flags[0] = 1; }
        return;
    }
    u64 mine[CAND_PER];
    unsigned h[CAND_PER];
    gather.finish(c_key, total, mine, h);
    const int want = total < K ? total : K;
    u64 kth = 0;
    __syncthreads();                                 // keys are in registers: c_key's head becomes the fast path's compact list
    if (total > K) kth = select_kth_largest<CAND_PER, 4, true>(h, [&](int j) { return (unsigned)mine[j]; }, want, red, c_key);
    // survivors: approximate score >= T~ - margin (total <= K: every candidate); a NaN on either side keeps the row
    const float cut = kth != 0 ? unorderable((unsigned)(kth >> 32)) - margin_in[b] : -INFINITY;
#pragma unroll
    for (int j = 0; j < CAND_PER; ++j) {
        if (mine[j] != 0 && !(unorderable(h[j]) < cut)) {
            const int p = atomicAdd(&nsurv, 1);
            if (p < RESC_MAX) surv[p] = 0xFFFFFFFFu - (unsigned)mine[j];
        }
    }
    __syncthreads();                                 // also: nobody reads c_key as keys any more -- it becomes the tiles
    const int ns = nsurv;
    if (ns > RESC_MAX) {
        if (tid == 0) { state[b] = 1; flags[0] = 1; }
        return;
    }
    rescore_and_rank(surv, ns, qrow, gallery, D, reinterpret_cast<float*>(c_key), x_key, K, idx_offset, out_scores + (long)b * K, out_idx + (long)b * K);
}

// ---- dense form of the certified pre-filter (galleries up to DENSE_MAX_N rows) -------------------------------------------------------
// For a small gallery the stage is launch boundaries, not bytes (C2: five kernels, 76 us, of which the sweep's 47 MB are ~10).  Here
// the bf16 sweep simply STORES its approximate scores ([B, ld] fp32: a quarter of the bf16 gallery's bytes at B = 64, D = 512) -- no
// sample pass, no bound kernel, no candidate lists, no atomics -- and this kernel does everything else, one workgroup per query:
//   pass 1  every thread's maximum over its strided share of the row -> per wave the ceil(K / 4)-th largest lane maximum -> l0 = the
//           smallest of the four: at least K scores are >= l0, so T~ (the K-th best approximate score) >= l0;
//   pass 2  (the row again, from L2) collect the rows with s~ >= l0 - margin: a superset of {s~ >= T~ - margin};
//   T~ among the collected, survivors = collected rows with s~ >= T~ - margin, exact rescoring + ranking (rescore_and_rank).
// Without room (more than DENSE_CAP collected, more than RESC_MAX survivors) the query is flagged for the exact pass with the bound
// it had reached (l0 - margin or T~ - margin: lower bounds of the exact K-th best).  Resets done[b] for that pass; flags[0] is
// zeroed by the host launcher before the sweep.
// Exact top-K of ONE query by its own workgroup (256 threads), for the dense form on SMALL galleries: a query the pre-filter has no room
// for (near-tie floods, galleries smaller than ~K, NaN scores) is ranked right here -- every row's exact chain, streamed through the
// waves' sorted lists (wave_offer: no capacity) -- instead of by the gated exact-pass launch, whose ~4.5 us of launch boundary every call
// paid for a case that almost never happens.  One CU streams the whole fp32 gallery (~60 GB/s): the launcher allows it up to 128 MB.
// tags != null: rows that are ineligible for this query ((tags[n] & mask) != value) are skipped like the excluded row.
__device__ __forceinline__ void exact_topk_inline(const float* qrow, const float* gallery, long N, int D, long drop, int K, long idx_offset,
                                                  float* os, int* oi, u64 (*wl)[64], const unsigned* tags = nullptr, QueryTags qt = {0u, 0u}) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64 best = 0;
#pragma unroll 1
    for (long n0 = (long)wave * 64; n0 < N; n0 += 256) {
        const long n = n0 + lane;
        u64 key = 0;
        if (n < N && n != drop && (!tags || row_eligible(tags[n], qt.mask, qt.value)))
            key = make_key(chain_run(gallery + n * D, qrow, D, 0.0f), (unsigned)n);
        wave_offer(best, key, K, lane);
    }
    wl[wave][lane] = best;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll 1
    for (int w = 1; w < 4; ++w) best = merge_sorted_desc(best, wl[w][lane], lane);
    if (lane < K) write_key(best, idx_offset, os + lane, oi + lane);
}

constexpr int DENSE_SEG = 1024;                 // collected keys per wave (4 segments)
constexpr int DENSE_UB = 16;                    // 16-byte loads a thread keeps in flight while it walks the score row
constexpr int DENSE_BATCH = 1024 * DENSE_UB;    // floats the workgroup covers per batch

// a cut as the bound the exact pass starts from (a cut that is no number: no bound)
__device__ __forceinline__ u64 bound_key(float cut) { return cut == cut ? (u64)orderable(cut) << 32 : 0ull; }

// NB > 0: the row fits NB batches, which stay in registers between the two passes (N <= NB * 16384); NB = 0: any N, the row is read
// twice (the second time from this XCD's L2).
template <int NB>
__global__ __launch_bounds__(256) void topk_dense_rescore_kernel(const float* approx, long ld, long N, const float* q, const float* gallery, int D,
                                                                 BoundMargin mg, int K, const int* exclude, long exclude_off, long idx_offset,
                                                                 float* out_scores, int* out_idx, u64* thr_key, int* flags, int* state, int* done, int inline_exact,
                                                                 RowTags rt) {
    // rt.tags != null: `approx` holds the MASKED sweep's scores (ineligible rows are -inf, so no walk collects them while the cut is a
    // number); the only places that look at the gallery itself again are the exact fallbacks, which apply the predicate.
    __shared__ u64 wlists[4][64];                                            // inline exact ranking: the waves' sorted lists
    __shared__ __attribute__((aligned(16))) u64 ckey[4][DENSE_SEG + 2];      // per wave: collected approximate keys (+ zero padding)
    __shared__ __attribute__((aligned(16))) float tiles[RESC_TILE_FLOATS];
    __shared__ __attribute__((aligned(16))) u64 x_key[RESC_MAX + 4];
    __shared__ unsigned surv[RESC_MAX];
    __shared__ __attribute__((aligned(16))) float qrow[1024];
    __shared__ float fred[8];                                                // margin_finish<4>
    __shared__ unsigned wmax[4];
    __shared__ int wcnt[4];
    __shared__ int nsurv;
    __shared__ unsigned kth_hi;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = approx + (long)b * ld;
    if (tid == 0) { nsurv = 0; kth_hi = 0; state[b] = 0; done[b] = 0; }
    for (int i = tid; i < D; i += 256) qrow[i] = q[(long)b * D + i];
    const long drop = excluded_local_row(exclude, b, exclude_off, N);
    const long n4 = N & ~3L;
    constexpr int NBR = NB > 0 ? NB : 1;
    f32x4 v[NBR][DENSE_UB];
    // This kernel runs ONE wave per SIMD (64 workgroups on 64 CUs): every VALU instruction of a phase is 4 cycles of its latency, so
    // the walks over the row are written for instruction count -- float maxima (v_max3_f32) instead of orderable keys, the excluded
    // row handled by a separate (rare) path, keys built only for the ~100 collected rows.
    // One batch: DENSE_UB loads per thread, UNCONDITIONAL on a clamped address and masked afterwards (behind `if (i < n4)` the
    // compiler put every load in its own branch with an s_waitcnt vmcnt(0) in front: sixteen serial round trips per batch).  The
    // row was written by the sweep from other XCDs: it comes from HBM / the Infinity Cache at 1-2 us a round trip.
    // Loaded values are SANITISED once (positions past the row and the excluded row become -inf), so that the two walks are one
    // v_max3 / one v_cmp per element.
    auto load_batch = [&](long base, f32x4 (&dst)[DENSE_UB]) {
#pragma unroll
        for (int u = 0; u < DENSE_UB; ++u) {
            const long i = base + u * 1024L + tid * 4;
            dst[u] = *reinterpret_cast<const f32x4*>(row + (i < n4 ? i : 0));
        }
#pragma unroll
        for (int u = 0; u < DENSE_UB; ++u) {
            const long i = base + u * 1024L + tid * 4;
            const bool in = i < n4;
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[u][e] = in ? dst[u][e] : -INFINITY;
            if (drop >= i && drop < i + 4) dst[u][drop - i] = -INFINITY;     // (rare: the excluded row)
        }
    };
    // the query's two norms (select.h): loads issued now, reduced after pass 1
    const QueryNorms qn = margin_accumulate<256>(q + (long)b * D, D);
    // pass 1: every thread's maximum score.  fmax drops NaNs; the running SUM of the scores is NaN whenever one of them is (or when
    // +inf meets -inf: a false alarm that only costs speed) -- a NaN anywhere makes the wave collect everything.
    float fmax_t = -INFINITY, nsum = 0.f;
    auto max_batch = [&](const f32x4 (&src)[DENSE_UB]) {
#pragma unroll
        for (int u = 0; u < DENSE_UB; ++u) {
            fmax_t = fmaxf(fmaxf(fmax_t, src[u][0]), fmaxf(src[u][1], fmaxf(src[u][2], src[u][3])));
            nsum += (src[u][0] + src[u][1]) + (src[u][2] + src[u][3]);      // (sanitised -inf positions keep the sum at -inf, not NaN)
        }
    };
    if (NB > 0) {
#pragma unroll
        for (int nb = 0; nb < NBR; ++nb) load_batch((long)nb * DENSE_BATCH, v[nb]);
#pragma unroll
        for (int nb = 0; nb < NBR; ++nb) max_batch(v[nb]);
    } else {
        for (long base = 0; base < n4; base += DENSE_BATCH) {
            load_batch(base, v[0]);
            max_batch(v[0]);
        }
    }
    float tail = -INFINITY;                          // the row's last N % 4 scores, one per thread (-inf: none / excluded)
    if (tid < (int)(N - n4) && n4 + tid != drop) { tail = row[n4 + tid]; fmax_t = fmaxf(fmax_t, tail); nsum += tail; }
    const bool nan_t = nsum != nsum;
    unsigned tmax = fmax_t == -INFINITY ? 0u : orderable(fmax_t);      // 0 = "no row": a thread without rows, or only -inf scores
    const float margin = margin_finish<4>(qn, D, mg.meta, fred);
    const unsigned sorted = sort_desc(tmax, lane);
    const int tw = (K + 3) / 4;
    const unsigned vw = (unsigned)__builtin_amdgcn_readlane((int)sorted, tw - 1);
    if (lane == 0) wmax[wave] = __any(nan_t) ? 0u : vw;                 // a NaN score anywhere in the wave's share: collect everything
    __syncthreads();
    unsigned l0 = wmax[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) l0 = wmax[w] < l0 ? wmax[w] : l0;
    // l0 == 0: some wave holds fewer than ceil(K / 4) rows (a gallery of < ~K rows), or met a NaN score
    // A query the pre-filter has no room for leaves the do-block with `fallback_thr` = the bound it had reached (a lower bound of the
    // exact K-th best) and is ranked exactly behind it: ONE copy of that code, at the end.
    u64 fallback_thr = 0;
    do {
    if (l0 == 0) break;      // (uniform) no bound -- tiny galleries, or NaN scores
    if (rt.tags && !(margin < INFINITY)) break;      // (uniform) filtered: a cut that is no number would collect the masked rows too
    const float cut0 = unorderable(l0) - margin;
    // (This kernel runs ONCE per CU on a cold instruction cache: its time follows the bytes of code it executes.  A second, never-taken
    // copy of the collection code (an "accept everything" form for tiny galleries) cost 4 us; those queries go to the exact pass instead.)
    // pass 2: collect the rows at or above cut0 into THIS WAVE's segment (wave_append), stored as raw (score bits, row), keyed after
    // the pass
    u64* seg = ckey[wave];
    int wn = 0;                                      // wave-uniform: entries in the segment so far
    auto collect_one = [&](float val, long n, bool hit) {
        wave_append(hit, wn, DENSE_SEG, [&](int pos) { seg[pos] = ((u64)__float_as_uint(val) << 32) | (unsigned)n; });
    };
    auto collect_batch = [&](long base, const f32x4 (&src)[DENSE_UB]) {
#pragma unroll
        for (int u = 0; u < DENSE_UB; ++u) {
            const long i = base + u * 1024L + tid * 4;
            {
                // two v_max3 + one compare reject a position (64 lanes x 4 scores) that holds nothing at or above the cut -- about half of them
                const float m4 = fmaxf(fmaxf(src[u][0], src[u][1]), fmaxf(src[u][2], src[u][3]));
                const bool nan4 = (src[u][0] + src[u][1]) + (src[u][2] + src[u][3]) != (src[u][0] + src[u][1]) + (src[u][2] + src[u][3]);
                if (__ballot(!(m4 < cut0) || nan4) == 0) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) collect_one(src[u][e], i + e, !(src[u][e] < cut0));      // sanitised positions are -inf < cut0
            }
        }
    };
    if (NB > 0) {
#pragma unroll
        for (int nb = 0; nb < NBR; ++nb) collect_batch((long)nb * DENSE_BATCH, v[nb]);
    } else {
        for (long base = 0; base < n4; base += DENSE_BATCH) {
            load_batch(base, v[0]);
            collect_batch(base, v[0]);
        }
    }
    collect_one(tail, n4 + tid, tid < (int)(N - n4) && n4 + tid != drop && !(tail < cut0));
    // raw entries -> ranking keys (orderable score, ~row), in place: the wave's own entries, no barrier needed before
    for (int i = lane; i < (wn < DENSE_SEG ? wn : DENSE_SEG); i += 64) {
        const u64 r = seg[i];
        seg[i] = make_key(__uint_as_float((unsigned)(r >> 32)), (unsigned)r);
    }
    const int wkeep = wn < DENSE_SEG ? wn : DENSE_SEG;
    if (lane < 2) seg[wkeep + lane] = 0;             // zero padding: the counting loop reads two keys at a time
    if (lane == 0) wcnt[wave] = wn;
    __syncthreads();
    const int c0 = wcnt[0], c1 = wcnt[1], c2 = wcnt[2], c3 = wcnt[3];
    const int nc = c0 + c1 + c2 + c3;
    if (c0 > DENSE_SEG || c1 > DENSE_SEG || c2 > DENSE_SEG || c3 > DENSE_SEG) {
        fallback_thr = bound_key(cut0);
        break;
    }
    // the i-th collected key (segments in wave order)
    auto key_at = [&](int i) -> u64 {
        if (i < c0) return ckey[0][i];
        i -= c0;
        if (i < c1) return ckey[1][i];
        i -= c1;
        if (i < c2) return ckey[2][i];
        return ckey[3][i - c2];
    };
    // T~ = K-th best approximate key of the collected rows (= of the gallery), by counting: keys are distinct, one 64-bit compare per
    // pair (the scores and rows as separate words cost ~15 VALU instructions per pair: 10 us at 127 collected rows)
    unsigned khi = 0;
    if (nc > K) {
        for (int i = tid; i < nc; i += 256) {
            const u64 key = key_at(i);
            int rank = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int cw = w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
                for (int j0 = 0; j0 < cw; j0 += 2) {
                    const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(&ckey[w][j0]);
                    rank += (a.x > key) + (a.y > key);
                }
            }
            if (rank == K - 1) kth_hi = (unsigned)(key >> 32);
        }
        __syncthreads();
        khi = kth_hi;
    }
    const float cut = khi != 0 ? unorderable(khi) - margin : -INFINITY;
    for (int i = tid; i < nc; i += 256) {
        const u64 key = key_at(i);
        if (!(unorderable((unsigned)(key >> 32)) < cut)) {
            const int p = atomicAdd(&nsurv, 1);
            if (p < RESC_MAX) surv[p] = 0xFFFFFFFFu - (unsigned)key;
        }
    }
    __syncthreads();
    const int ns = nsurv;
    if (ns > RESC_MAX) {
        fallback_thr = khi != 0 ? bound_key(cut) : 0ull;
        break;
    }
    rescore_and_rank(surv, ns, qrow, gallery, D, tiles, x_key, K, idx_offset, out_scores + (long)b * K, out_idx + (long)b * K);
    return;
    } while (0);
    if (inline_exact) {      // small galleries: ranked exactly right here
        exact_topk_inline(qrow, gallery, N, D, drop, K, idx_offset, out_scores + (long)b * K, out_idx + (long)b * K, wlists, rt.tags,
                          query_tags(rt, b));
    } else if (tid == 0) {   // flagged for the gated exact pass
        state[b] = 1;
        flags[0] = 1;
        thr_key[b] = fallback_thr;
    }
}

// ---- dense form on tile maxima (galleries past TILES_MIN_N rows) -------------------------------------------------------------------
// topk_dense_rescore_kernel walks a query's whole score row twice with ONE workgroup: 2 x 184 KB at C2 (13 us of its 24), 2 x 800 KB
// at C3 (~60 of ~75).  Here the sweep also leaves tmax[b][t] = the largest score of gallery tile t (32 consecutive rows: one wave tile
// of sweep_bf16_kernel, reduced across its lanes), and the kernel reads N / 32 numbers instead of N:
//   bound   every thread's maximum over its strided share of the TILE maxima -> per wave the ceil(K' / 4)-th largest -> l0 = the
//           smallest of the four: K' distinct tiles hold a score >= l0 (K' = K + 1 when a row is excluded: it may be one of them),
//           so T~ (the K-th best approximate score) >= l0;
//   tiles   the tiles with tmax >= l0 - margin (~one per collected row: ~130 of 1 438 at C2) are listed, per wave, by ballot;
//   gather  only those tiles' scores are read (128 bytes each, all loads of the workgroup in flight at once) and the rows at or above
//           l0 - margin collected -- the same set the row walk collected;
//   then T~, survivors, exact rescoring and ranking exactly as topk_dense_rescore_kernel.
// A margin that is not finite (NaN / inf anywhere in the query or the gallery: launch_gallery_prepare poisons meta) sends the query to
// the exact ranking at once; with a finite margin every score is finite (|s~| <= ||q|| G~ (1 + D 2^-24)), so fmax loses nothing.
constexpr int TILES_TB = 32;                    // tile maxima a thread holds per batch (8 192 tiles = 262 144 rows per batch)
constexpr int TILES_SEG = 512;                  // listed tiles per wave
constexpr long TILES_MIN_N = 16384;             // below: the row walk (a wave needs ceil(K' / 4) tiles of its own for the bound)
template <bool HOLD>
__global__ __launch_bounds__(256) void topk_tiles_rescore_kernel(const float* approx, long ld, const float* tmax, long ldt, long N, const float* q,
                                                                 const float* gallery, int D, BoundMargin mg, int K, const int* exclude, long exclude_off,
                                                                 long idx_offset, float* out_scores, int* out_idx, u64* thr_key, int* flags, int* state,
                                                                 int* done, int inline_exact, RowTags rt) {
    // (rt: as in topk_dense_rescore_kernel -- tile maxima and scores come from the masked sweep; a tile whose rows are all ineligible
    //  has maximum -inf = "no tile")
    __shared__ u64 wlists[4][64];
    __shared__ __attribute__((aligned(16))) u64 ckey[4][DENSE_SEG + 2];
    __shared__ __attribute__((aligned(16))) float tiles[RESC_TILE_FLOATS];
    __shared__ __attribute__((aligned(16))) u64 x_key[RESC_MAX + 4];
    __shared__ unsigned surv[RESC_MAX];
    __shared__ __attribute__((aligned(16))) float qrow[1024];
    __shared__ int tlist[4][TILES_SEG];
    __shared__ float fred[8];                        // margin_finish<4>
    __shared__ unsigned wmax[4];
    __shared__ int wcnt[4], tcnt[4];
    __shared__ int nsurv;
    __shared__ unsigned kth_hi;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = approx + (long)b * ld;
    const float* trow = tmax + (long)b * ldt;
    const long ntiles = (N + 31) >> 5;
    if (tid == 0) { nsurv = 0; kth_hi = 0; state[b] = 0; done[b] = 0; }
    for (int i = tid; i < D; i += 256) qrow[i] = q[(long)b * D + i];
    const long drop = excluded_local_row(exclude, b, exclude_off, N);
    // tile maxima: TILES_TB unconditional loads on clamped addresses (topk_dense_rescore_kernel's note), masked afterwards
    float tv[TILES_TB];
    auto load_tiles = [&](long base) {
#pragma unroll
        for (int u = 0; u < TILES_TB; ++u) {
            const long t = base + u * 256 + tid;
            tv[u] = trow[t < ntiles ? t : 0];
        }
#pragma unroll
        for (int u = 0; u < TILES_TB; ++u) tv[u] = base + u * 256 + tid < ntiles ? tv[u] : -INFINITY;
    };
    const QueryNorms qn = margin_accumulate<256>(q + (long)b * D, D);      // reduced after the walk, as in topk_dense_rescore_kernel
    float fmax_t = -INFINITY;
    for (long base = 0; base < (HOLD ? 1 : ntiles); base += 256 * TILES_TB) {
        load_tiles(base);
#pragma unroll
        for (int u = 0; u < TILES_TB; u += 2) fmax_t = fmaxf(fmax_t, fmaxf(tv[u], tv[u + 1]));
    }
    const unsigned tmx = fmax_t == -INFINITY ? 0u : orderable(fmax_t);      // 0 = "no tile"
    const float margin = margin_finish<4>(qn, D, mg.meta, fred);
    const unsigned sorted = sort_desc(tmx, lane);
    const int tw = (K + (drop >= 0 ? 1 : 0) + 3) / 4;
    const unsigned vw = (unsigned)__builtin_amdgcn_readlane((int)sorted, tw - 1);
    if (lane == 0) wmax[wave] = vw;
    __syncthreads();
    unsigned l0 = wmax[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) l0 = wmax[w] < l0 ? wmax[w] : l0;
    u64 fallback_thr = 0;
    do {
    if (l0 == 0 || !(margin < INFINITY)) break;      // (uniform) no bound: a wave without ceil(K' / 4) tiles; or no certificate
    const float cut0 = unorderable(l0) - margin;
    // the tiles that can hold a row at or above cut0, per wave by ballot
    int* tl = tlist[wave];
    int tn = 0;                                      // wave-uniform
    for (long base = 0; base < (HOLD ? 1 : ntiles); base += 256 * TILES_TB) {
        if (!HOLD) load_tiles(base);
#pragma unroll
        for (int u = 0; u < TILES_TB; ++u)           // masked positions are -inf < cut0 (cut0 is finite)
            wave_append(!(tv[u] < cut0), tn, TILES_SEG, [&](int pos) { tl[pos] = (int)(base + u * 256 + tid); });
    }
    if (lane == 0) tcnt[wave] = tn;
    __syncthreads();
    const int t0 = tcnt[0], t1 = tcnt[1], t2 = tcnt[2], t3 = tcnt[3];
    if (t0 > TILES_SEG || t1 > TILES_SEG || t2 > TILES_SEG || t3 > TILES_SEG) {      // near-tie floods: the exact ranking, behind the bound
        fallback_thr = (u64)orderable(cut0) << 32;
        break;
    }
    const int p1 = t0, p2 = t0 + t1, p3 = p2 + t2, nt = p3 + t3;
    // gather: 8 lanes x 16 bytes per listed tile, four rounds of loads in flight; hits go to the wave's segment as ranking keys
    u64* seg = ckey[wave];
    int wn = 0;
    const int items = nt * 8;
    for (int e0 = 0; e0 < items; e0 += 1024) {
        f32x4 val[4];
        long nn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * 256 + tid, ec = e < items ? e : 0, slot = ec >> 3;
            const int w = (slot >= p1) + (slot >= p2) + (slot >= p3);
            const int tile = tlist[w][slot - (w == 0 ? 0 : w == 1 ? p1 : w == 2 ? p2 : p3)];
            nn[u] = (long)tile * 32 + (ec & 7) * 4;
            val[u] = *reinterpret_cast<const f32x4*>(row + nn[u]);      // ld covers whole tiles (launcher)
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = e0 + u * 256 + tid < items;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long n = nn[u] + j;
                wave_append(in && n < N && n != drop && !(val[u][j] < cut0), wn, DENSE_SEG,
                            [&](int pos) { seg[pos] = make_key(val[u][j], (unsigned)n); });
            }
        }
    }
    const int wkeep = wn < DENSE_SEG ? wn : DENSE_SEG;
    if (lane < 2) seg[wkeep + lane] = 0;
    if (lane == 0) wcnt[wave] = wn;
    __syncthreads();
    const int c0 = wcnt[0], c1 = wcnt[1], c2 = wcnt[2], c3 = wcnt[3];
    const int nc = c0 + c1 + c2 + c3;
    if (c0 > DENSE_SEG || c1 > DENSE_SEG || c2 > DENSE_SEG || c3 > DENSE_SEG) {
        fallback_thr = (u64)orderable(cut0) << 32;
        break;
    }
    auto key_at = [&](int i) -> u64 {
        if (i < c0) return ckey[0][i];
        i -= c0;
        if (i < c1) return ckey[1][i];
        i -= c1;
        if (i < c2) return ckey[2][i];
        return ckey[3][i - c2];
    };
    unsigned khi = 0;
    if (nc > K) {
        for (int i = tid; i < nc; i += 256) {
            const u64 key = key_at(i);
            int rank = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int cw = w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
                for (int j0 = 0; j0 < cw; j0 += 2) {
                    const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(&ckey[w][j0]);
                    rank += (a.x > key) + (a.y > key);
                }
            }
            if (rank == K - 1) kth_hi = (unsigned)(key >> 32);
        }
        __syncthreads();
        khi = kth_hi;
    }
    const float cut = khi != 0 ? unorderable(khi) - margin : -INFINITY;
    for (int i = tid; i < nc; i += 256) {
        const u64 key = key_at(i);
        if (!(unorderable((unsigned)(key >> 32)) < cut)) {
            const int p = atomicAdd(&nsurv, 1);
            if (p < RESC_MAX) surv[p] = 0xFFFFFFFFu - (unsigned)key;
        }
    }
    __syncthreads();
    const int ns = nsurv;
    if (ns > RESC_MAX) {
        fallback_thr = khi != 0 ? (u64)orderable(cut) << 32 : 0ull;
        break;
    }
    rescore_and_rank(surv, ns, qrow, gallery, D, tiles, x_key, K, idx_offset, out_scores + (long)b * K, out_idx + (long)b * K);
    return;
    } while (0);
    if (inline_exact) {
        exact_topk_inline(qrow, gallery, N, D, drop, K, idx_offset, out_scores + (long)b * K, out_idx + (long)b * K, wlists, rt.tags,
                          query_tags(rt, b));
    } else if (tid == 0) {
        state[b] = 1;
        flags[0] = 1;
        thr_key[b] = fallback_thr;
    }
}

// ---- exact pass ---------------------------------------------------------------------------------------------------------------
// Runs (gated on flags[0]) for the queries the select kernel sent here.  One launch of `groups` workgroups; workgroup g, wave w
// owns the 32-row gallery tiles (4g + w) + j * 4 * groups.  The flagged queries are compacted (in query order) and taken 32 AT A
// TIME as the 32 A rows of the tile MFMAs -- ONE gallery pass per 32 flagged queries (round 3 broadcast one query to all 32 rows:
// a pass per query, 1/32 of the MFMA).  A tile's scores come from the SAME MFMA sequence as the sweep kernels -- fp32:
// v_mfma_f32_32x32x2_f32 per 8-group g8 and e = 0..3 with lane half h feeding k = 8 g8 + 4 h + e (gemm.hip); bf16:
// v_mfma_f32_32x32x16_bf16 per 16-k step with lane half h feeding k = 16 ks + 8 h .. + 7, the query rounded to bf16 like
// sweep_bf16.hip does -- so register r of lane (n & 31) + 32 h holds the bit-identical score of gallery row n for query
// (r & 3) + 8 (r >> 2) + 4 h of the chunk.  Keys that reach a query's (still valid) sampled bound are offered to that query's sorted
// list of the wave (64 entries, one per lane, kept in LDS: lists[wave][query]); after the pass the four wave lists of a query are
// merged into partial[b][g], and the last workgroup to finish a query (a ticket in done[b]) merges the partial lists and writes the
// ranking.  Nothing here has a capacity: whatever the gallery looks like, the result is the exact top-K.
typedef short bf16x8e __attribute__((ext_vector_type(8)));
constexpr int EXACT_QB = 32;                    // flagged queries per gallery pass (the A rows of one MFMA tile)
template <bool BF16>
__global__ __launch_bounds__(256) void rank_exact_kernel(const float* q, const void* gallery, int B, long N, int D, int K, const int* state,
                                                         const u64* thr_key, const int* exclude, long exclude_off, long idx_offset,
                                                         u64* partial, int* done, float* out_scores, int* out_idx, const int* gate, RowTags rt) {
    if (*gate == 0) return;
    __shared__ unsigned mk_s[EXACT_QB], vl_s[EXACT_QB];      // rt.tags != null: the chunk's row filters (ineligible rows are never offered)
    __shared__ u64 lists[4][EXACT_QB][64];      // 64 KiB: every wave's sorted list of every query of the chunk
    __shared__ int flagged[1024];               // the flagged queries in query order (a plan holds <= 1024 queries: api.hip kRankQueryChunk)
    __shared__ u64 thr_s[EXACT_QB];
    __shared__ long ex_s[EXACT_QB];
    __shared__ int wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int G = gridDim.x, g = blockIdx.x;
    const long ntiles = (N + 31) / 32;
    // compaction: thread t looks at queries 4t .. 4t + 3
    int fl[4], cnt = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int b = tid * 4 + u;
        fl[u] = b < B && state[b] != 0;
        cnt += fl[u];
    }
    int nflag;
    int base = block_exclusive_scan<4>(cnt, wtot, nflag);
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (fl[u]) flagged[base++] = tid * 4 + u;
    __syncthreads();
    for (int c0 = 0; c0 < nflag; c0 += EXACT_QB) {
        const int nq = nflag - c0 < EXACT_QB ? nflag - c0 : EXACT_QB;       // queries of this chunk (uniform)
        if (tid < EXACT_QB) {
            const int b = flagged[c0 + (tid < nq ? tid : 0)];
            thr_s[tid] = tid < nq ? thr_key[b] : ~0ull;
            ex_s[tid] = (tid < nq && exclude) ? (long)exclude[b] - exclude_off : -1;
            const QueryTags qt = tid < nq ? query_tags(rt, b) : QueryTags{0u, 0u};
            mk_s[tid] = qt.mask;
            vl_s[tid] = qt.value;
        }
        for (int i = tid; i < 4 * EXACT_QB * 64; i += 256) (&lists[0][0][0])[i] = 0;
        __syncthreads();
        const float* qrow = q + (long)flagged[c0 + (l31 < nq ? l31 : 0)] * D;      // this lane's A row
        float bound[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) bound[r] = filter_bound(thr_s[(r & 3) + 8 * (r >> 2) + 4 * lh]);      // +inf for the unused rows
        for (long t = (long)g * 4 + wave; t < ntiles; t += (long)G * 4) {
            const long n = t * 32 + l31;
            const long nc = n < N ? n : N - 1;
            const unsigned tag = rt.tags ? rt.tags[nc] : 0u;
            f32x16 acc;
            if (BF16) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
                const unsigned short* grow = reinterpret_cast<const unsigned short*>(gallery) + nc * D;
                for (int ks = 0; ks < D / 16; ++ks) {
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(qrow + ks * 16 + lh * 8);
                    const f32x4 a1 = *reinterpret_cast<const f32x4*>(qrow + ks * 16 + lh * 8 + 4);
                    bf16x8e af;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { af[e] = (short)f32_to_bf16_bits(a0[e]); af[4 + e] = (short)f32_to_bf16_bits(a1[e]); }
                    const bf16x8e bf = *reinterpret_cast<const bf16x8e*>(grow + ks * 16 + lh * 8);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
                }
            } else {
                acc = score_tile_f32(qrow, reinterpret_cast<const float*>(gallery) + nc * D, D, lh);
            }
            // which queries of the chunk have a score at or above their bound in this tile (wave-uniform bit mask)
            unsigned qmask = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const u64 m = __ballot(n < N && !(acc[r] < bound[r]));
                const int qa = (r & 3) + 8 * (r >> 2);
                qmask |= ((unsigned)m != 0u ? 1u : 0u) << qa;
                qmask |= ((unsigned)(m >> 32) != 0u ? 1u : 0u) << (qa + 4);
            }
            qmask &= nq >= 32 ? 0xFFFFFFFFu : ((1u << nq) - 1u);
            while (qmask) {                                        // wave-uniform loop over the queries with survivors
                const int qi = __builtin_ctz(qmask);
                qmask &= qmask - 1;
                const int rsel = (qi & 3) + 4 * (qi >> 3), hsel = (qi >> 2) & 1;
                float v = acc[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) v = rsel == r ? acc[r] : v;
                u64 cand = 0;
                if (lh == hsel && n < N && n != ex_s[qi] && row_eligible(tag, mk_s[qi], vl_s[qi])) {
                    const u64 key = make_key(v, (unsigned)n);
                    cand = key >= thr_s[qi] ? key : 0;
                }
                u64 best = lists[wave][qi][lane];
                wave_offer(best, cand, K, lane);
                lists[wave][qi][lane] = best;
            }
        }
        __syncthreads();
        // wave w finishes queries w, w + 4, ...: merge the four wave lists, publish the partial list, take a ticket
        for (int qi = wave; qi < nq; qi += 4) {
            const int b = flagged[c0 + qi];
            u64 best = lists[0][qi][lane];
#pragma unroll 1
            for (int w = 1; w < 4; ++w) best = merge_sorted_desc(best, lists[w][qi][lane], lane);
            partial[((long)b * G + g) * 64 + lane] = best;
            __threadfence();
            int ticket = 0;
            if (lane == 0) ticket = atomicAdd(&done[b], 1);
            ticket = __builtin_amdgcn_readfirstlane(ticket);
            if (ticket == G - 1) {                                  // every other workgroup's partial list is visible (its fence precedes its ticket)
                __threadfence();
                u64 top = 0;
#pragma unroll 1
                for (int gg = 0; gg < G; ++gg) {
                    const u64 other = __hip_atomic_load(&partial[((long)b * G + gg) * 64 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    top = gg == 0 ? other : merge_sorted_desc(top, other, lane);
                }
                if (lane < K) write_key(top, idx_offset, out_scores + (long)b * K + lane, out_idx + (long)b * K + lane);
            }
        }
        __syncthreads();                                            // the lists are re-zeroed for the next chunk
    }
}

hipError_t launch_topk_sample_bound(const float* scores, long ld, int B, long S, int R, int K, const int* exclude, long exclude_off,
                                    u64* thr_key, int* count, int* flags, int* state, hipStream_t s, const float* q, int D, const float* meta,
                                    float* margin_out) {
    if (B <= 0) return hipSuccess;
    if (K < 1 || K > 64 || S < 0 || R < 1 || (q && (!meta || !margin_out || D <= 0))) return hipErrorInvalidValue;
    const BoundMargin mg{q, D, meta, margin_out};
    // keys per thread of the bisection (registers): the plan caps S at 32768 (api.hip: rank_plan)
    auto go = [&](auto kern, int nt) { FERN_LAUNCH(kern, dim3(B), dim3(nt), 0, s, scores, ld, S, R, K, exclude, exclude_off, thr_key, count, flags, state, mg); };
    if (S <= 1024) go(topk_sample_bound_kernel<4, 256>, 256);
    else if (S <= 4096) go(topk_sample_bound_kernel<16, 256>, 256);
    else if (S <= 16 * 1024) go(topk_sample_bound_kernel<16, 1024>, 1024);
    else if (S <= 32 * 1024) go(topk_sample_bound_kernel<32, 1024>, 1024);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_topk_candidates(const TopkFilter& f, int B, int K, long idx_offset, float* out_scores, int* out_idx, int* flags,
                                  int* state, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (K < 1 || K > 64 || f.cap < 1 || f.cap > 64) return hipErrorInvalidValue;
    FERN_LAUNCH(topk_candidates_kernel, dim3(B), dim3(256), 0, s, f, K, idx_offset, out_scores, out_idx, flags, state);
    return hipGetLastError();
}

hipError_t launch_topk_rescore(const TopkFilter& f, const float* q, const float* gallery, int D, const float* margin, int B, int K, long idx_offset,
                               float* out_scores, int* out_idx, int* flags, int* state, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (K < 1 || K > 64 || f.cap < 1 || f.cap > 64 || D < 64 || D % 64 || D > 1024 || !margin) return hipErrorInvalidValue;
    FERN_LAUNCH(topk_rescore_kernel, dim3(B), dim3(256), 0, s, f, q, gallery, D, margin, K, idx_offset, out_scores, out_idx, flags, state);
    return hipGetLastError();
}

hipError_t launch_topk_dense_rescore(const float* approx, long ld, long N, const float* q, const float* gallery, int D, const float* meta,
                                     int B, int K, const int* exclude, long exclude_off, long idx_offset, float* out_scores,
                                     int* out_idx, unsigned long long* thr_key, int* flags, int* state, int* done, hipStream_t s, int inline_exact,
                                     const float* tmax, long ldt, const RowTags* rtp) {
    if (B <= 0) return hipSuccess;
    RowTags rt;
    if (!row_tags_arg(rtp, rt)) return hipErrorInvalidValue;
    if (K < 1 || K > 64 || D < 64 || D % 64 || D > 1024 || N < 1 || (ld & 3) || !meta) return hipErrorInvalidValue;
    const BoundMargin mg{q, D, meta, nullptr};
    if (tmax && N >= TILES_MIN_N) {                  // selection on the sweep's tile maxima
        if (ld < ((N + 31) & ~31L) || ldt < (N + 31) / 32) return hipErrorInvalidValue;
        if ((N + 31) / 32 <= 256L * TILES_TB)
            FERN_LAUNCH(topk_tiles_rescore_kernel<true>, dim3(B), dim3(256), 0, s, approx, ld, tmax, ldt, N, q, gallery, D, mg, K, exclude, exclude_off,
                        idx_offset, out_scores, out_idx, thr_key, flags, state, done, inline_exact, rt);
        else
            FERN_LAUNCH(topk_tiles_rescore_kernel<false>, dim3(B), dim3(256), 0, s, approx, ld, tmax, ldt, N, q, gallery, D, mg, K, exclude, exclude_off,
                        idx_offset, out_scores, out_idx, thr_key, flags, state, done, inline_exact, rt);
        return hipGetLastError();
    }
    const long n4 = N & ~3L;
#define FERN_DENSE_GO(NB)                                                                                                                       \
    FERN_LAUNCH(topk_dense_rescore_kernel<NB>, dim3(B), dim3(256), 0, s, approx, ld, N, q, gallery, D, mg, K, exclude, exclude_off, idx_offset, \
                out_scores, out_idx, thr_key, flags, state, done, inline_exact, rt)
    if (n4 <= 1L * DENSE_BATCH) FERN_DENSE_GO(1);
    else if (n4 <= 2L * DENSE_BATCH) FERN_DENSE_GO(2);
    else if (n4 <= 3L * DENSE_BATCH) FERN_DENSE_GO(3);
    else FERN_DENSE_GO(0);
#undef FERN_DENSE_GO
    return hipGetLastError();
}

hipError_t launch_rank_exact(const float* q, const void* gallery, int gallery_bf16, int B, long N, int D, int K, const int* state,
                             const unsigned long long* thr_key, const int* exclude, long exclude_off, long idx_offset,
                             unsigned long long* partial, int groups, int* done, float* out_scores, int* out_idx, const int* gate,
                             hipStream_t s, const RowTags* rtp) {
    if (B <= 0 || N <= 0) return hipSuccess;
    RowTags rt;
    if (!row_tags_arg(rtp, rt)) return hipErrorInvalidValue;
    if (K < 1 || K > 64 || groups < 1 || B > 1024 || D % (gallery_bf16 ? 16 : 8)) return hipErrorInvalidValue;
    if (gallery_bf16)
        FERN_LAUNCH(rank_exact_kernel<true>, dim3(groups), dim3(256), 0, s, q, gallery, B, N, D, K, state, thr_key, exclude, exclude_off,
                    idx_offset, partial, done, out_scores, out_idx, gate, rt);
    else
        FERN_LAUNCH(rank_exact_kernel<false>, dim3(groups), dim3(256), 0, s, q, gallery, B, N, D, K, state, thr_key, exclude, exclude_off,
                    idx_offset, partial, done, out_scores, out_idx, gate, rt);
    return hipGetLastError();
}

hipError_t launch_topk_merge(const float* scores, const int* idx, float* out_scores, int* out_idx, int R, int B, int K, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (K < 1 || K > 64 || R < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_merge_kernel, dim3(B), dim3(64), 0, s, scores, idx, out_scores, out_idx, R, B, K);
    return hipGetLastError();
}

}  // namespace fern

// Deep exact top-K (64 < K <= 1024, any K >= 1 works): fern_sim_topk_deep and the wide form of fern_topk_merge.
//
// topk.hip's machinery keeps one sorted entry per lane of a wave, so it stops at K = 64.  The deep stage instead works on a STORED
// score row per query ([m, ld] fp32 workspace) and sorts in LDS:
//   scores    exact form: deep_exact_scores_kernel (the fp32 MFMA sequence of rank_exact_kernel: bit for bit the oracle/chain.c
//             order, whatever fern_set_precision says); pre-filtered and bf16 forms: launch_sweep_bf16 in its store form;
//   select    deep_select_kernel, one workgroup per query:
//               pass 1  the row in float4 batches; every thread keeps 16 running maxima (one per batch slot): 4 096 disjoint row groups.
//                       L = the K-th largest group maximum: K rows (one per group) score >= L, so the K-th best score T >= L;
//               pass 2  the rows with score >= L - margin are collected into LDS as ranking keys (<= cap of them);
//               sort    one bitonic sort of the collected keys (registers, lane shuffles, LDS only across waves);
//               margin 0 (exact and bf16 forms): the first K keys are the answer.  Pre-filter (margin = 2 eps_b, select.h):
//                       T~ = the K-th sorted approximate key, the survivors (s~ >= T~ - margin) are a prefix of the sorted keys; they
//                       get their exact chain scores (rescore.h) and are sorted again;
//   fallback  a query without room (more than `cap` collected rows: tie floods, near-constant galleries; a NaN score; a margin that is
//             not finite) is flagged (state[b], flags[0]).  Gated kernels then rewrite its row with exact scores (pre-filter form only)
//             and select on it by an 8-pass radix select over the 64-bit keys -- no capacity anywhere -- so the stage is exact whatever
//             the gallery looks like, with no read-back to the host.
// Keys are topk.hip's: orderable(score) << 32 | ~index, so the first K' <= 64 places are those of fern_sim_topk* bit for bit.
#include "kernels.h"
#include "rescore.h"
#include "select.h"

#include <algorithm>
#include <cstdlib>

namespace fern {

// ---- block bitonic sort (descending) of NT * P keys: thread t holds elements t * P .. t * P + P - 1 in registers -------------------
// Stages with J < P are register swaps, J < 64 P lane shuffles, the rest (a handful) go through `buf` (NT * P keys of LDS).
template <int NT, int P, int K, int J>
__device__ __forceinline__ void bsort_stage(u64 (&v)[P], u64* buf) {
    const int tid = threadIdx.x;
    if constexpr (J < P) {
#pragma unroll
        for (int r = 0; r < P; ++r) {
            if ((r & J) == 0) {
                const bool desc = ((tid * P + r) & K) == 0;
                const u64 a = v[r], c = v[r | J];
                const u64 mx = a > c ? a : c, mn = a > c ? c : a;
                v[r] = desc ? mx : mn;
                v[r | J] = desc ? mn : mx;
            }
        }
    } else if constexpr (J < 64 * P) {
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const u64 o = shfl_xor64(v[r], J / P);
            const int e = tid * P + r;
            const bool keep_max = ((e & K) == 0) == ((e & J) == 0);
            v[r] = keep_max ? (v[r] > o ? v[r] : o) : (v[r] > o ? o : v[r]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < P; ++r) buf[tid * P + r] = v[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const int e = tid * P + r;
            const u64 o = buf[e ^ J];
            const bool keep_max = ((e & K) == 0) == ((e & J) == 0);
            v[r] = keep_max ? (v[r] > o ? v[r] : o) : (v[r] > o ? o : v[r]);
        }
        __syncthreads();
    }
    if constexpr (J > 1) bsort_stage<NT, P, K, J / 2>(v, buf);
}
template <int NT, int P, int K>
__device__ __forceinline__ void bsort_level(u64 (&v)[P], u64* buf) {
    bsort_stage<NT, P, K, K / 2>(v, buf);
    if constexpr (K < NT * P) bsort_level<NT, P, K * 2>(v, buf);
}
// keys[0 .. n) sorted descending in place, keys[n .. NT * P) become 0.  Every thread calls it; `keys` holds NT * P entries.
template <int NT, int P>
__device__ __forceinline__ void sort_lds_desc(u64* keys, int n) {
    const int tid = threadIdx.x;
    u64 v[P];
#pragma unroll
    for (int r = 0; r < P; ++r) v[r] = tid * P + r < n ? keys[tid * P + r] : 0ull;
    __syncthreads();
    bsort_level<NT, P, 2>(v, keys);
#pragma unroll
    for (int r = 0; r < P; ++r) keys[tid * P + r] = v[r];
    __syncthreads();
}

// ---- exact scores ------------------------------------------------------------------------------------------------------------------
// S[b][n] = the fp32 score of query b and gallery row n from score_tile_f32 (select.h), as rank_exact_kernel takes it: the oracle/chain.c
// order.  Workgroup (x, y): queries 32 y .. 32 y + 31, wave w the 32-row tiles
// 4 x + w + j * 4 gridDim.x.  GATED: runs only if flags[0] is set and writes only the rows of flagged queries (state[b] != 0);
// otherwise it also zeroes flags[0..3] for the selection that follows.
// rt.tags != null (a per-query row filter, kernels.h: RowTags; kernel-uniform branch -- this kernel is MFMA-bound on fp32 operands, the
// predicate is 16 VALU compares per 32 x 32 tile): an ineligible (query, row) pair is stored as -inf, in the GATED rewrite as well, so
// neither the selection nor the radix fallback ever sees it.
template <bool GATED>
__global__ __launch_bounds__(256) void deep_exact_scores_kernel(const float* q, const float* gallery, int B, long N, int D, float* S, long ld,
                                                                int* flags, const int* state, RowTags rt) {
    __shared__ int qflag[32];
    __shared__ unsigned qmask[32], qvalue[32];
    __shared__ int any;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int q0 = blockIdx.y * 32, nq = B - q0 < 32 ? B - q0 : 32;
    if (GATED) {
        if (flags[0] == 0) return;
        if (tid == 0) any = 0;
        __syncthreads();
        if (tid < 32) {
            qflag[tid] = tid < nq && state[q0 + tid] != 0;
            if (qflag[tid]) any = 1;
        }
        __syncthreads();
        if (any == 0) return;
    } else {
        if (blockIdx.x == 0 && blockIdx.y == 0 && tid < 4) flags[tid] = 0;
        if (tid < 32) qflag[tid] = tid < nq;
        __syncthreads();
    }
    const bool tagged = rt.tags != nullptr;
    if (tagged) {
        if (tid < 32) { qmask[tid] = tid < nq ? rt.mask[q0 + tid] : 0u; qvalue[tid] = tid < nq ? rt.value[q0 + tid] : 1u; }
        __syncthreads();
    }
    const float* qrow = q + (long)(q0 + (l31 < nq ? l31 : 0)) * D;      // this lane's A row
    const long ntiles = (N + 31) / 32;
    for (long t = (long)blockIdx.x * 4 + wave; t < ntiles; t += (long)gridDim.x * 4) {
        const long n = t * 32 + l31;
        const float* grow = gallery + (n < N ? n : N - 1) * D;
        const unsigned tag = tagged ? rt.tags[n < N ? n : N - 1] : 0u;      // issued in front of the row's loads
        const f32x16 acc = score_tile_f32(qrow, grow, D, lh);
        if (n < N) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (qflag[qi]) S[(long)(q0 + qi) * ld + n] = (!tagged || row_eligible(tag, qmask[qi], qvalue[qi])) ? acc[r] : -INFINITY;
            }
        }
    }
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------
constexpr int DEEP_NT = 256;                    // threads per query (one wave per SIMD: the rescoring ring needs the registers)
constexpr int DEEP_CAP = DEEP_NT * 16;          // collected keys per query (LDS)
constexpr int DEEP_UB = 16;                     // float4 loads a thread keeps in flight while it walks the row
constexpr int DEEP_MAX_D = 768;                 // the pre-filter's query row in LDS (the bf16 sweep's limit)
constexpr int DEEP_WAVES = DEEP_NT / 64;

struct DeepMargin {
    const float* q;          // [B, D] fp32 queries; null: margin 0, the stored scores are the ranking scores
    const float* meta;       // fern_gallery_prepare: {E, G~, G}
    const float* gallery;    // [N, D] fp32: the survivors' exact chains
    int D;
};

template <int NT>
__device__ __forceinline__ void sort_keys_desc(u64* keys, int n) {      // keys: 16 NT entries
    if (n <= 2 * NT) sort_lds_desc<NT, 2>(keys, n);
    else if (n <= 4 * NT) sort_lds_desc<NT, 4>(keys, n);
    else if (n <= 8 * NT) sort_lds_desc<NT, 8>(keys, n);
    else sort_lds_desc<NT, 16>(keys, n);
}

// CEIL: ceil[b] is a ranking key with the GLOBAL row index; a row whose key is greater is masked to -inf where the row is loaded, so the group
// maxima, the collection and the fallback gate all see it as a row that takes no place (the fallback applies the same rule to its keys).
template <bool CEIL>
__global__ __launch_bounds__(DEEP_NT) void deep_select_kernel(const float* S, long ld, long N, int K, DeepMargin mg, const int* exclude, long idx_offset,
                                                              int cap, float* out_scores, int* out_idx, int* flags, int* state, const u64* ceil) {
    __shared__ __attribute__((aligned(16))) u64 ckey[DEEP_CAP];
    __shared__ unsigned surv[DEEP_CAP];
    __shared__ __attribute__((aligned(16))) float tiles[DEEP_WAVES * 2 * RESC_ROWS * RESC_TLD];
    __shared__ __attribute__((aligned(16))) float qrow[DEEP_MAX_D];
    __shared__ float fred[2 * DEEP_WAVES];
    __shared__ int ncoll, nsurv;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = S + (long)b * ld;
    float* os = out_scores + (long)b * K;
    int* oi = out_idx + (long)b * K;
    if (tid == 0) { ncoll = 0; nsurv = 0; state[b] = 0; }
    const long drop = excluded_local_row(exclude, b, idx_offset, N);
    const u64 ck = CEIL ? ceil[b] : ~0ull;
    const long n4 = N & ~3L;
    constexpr long STEP = (long)DEEP_NT * 4 * DEEP_UB;
    // one batch: DEEP_UB unconditional loads on clamped addresses, then masked (positions past the row and the excluded row -> -inf)
    auto load_batch = [&](long base, f32x4 (&v)[DEEP_UB]) {
#pragma unroll
        for (int u = 0; u < DEEP_UB; ++u) {
            const long i = base + ((long)u * DEEP_NT + tid) * 4;
            v[u] = *reinterpret_cast<const f32x4*>(row + (i < n4 ? i : 0));
        }
#pragma unroll
        for (int u = 0; u < DEEP_UB; ++u) {
            const long i = base + ((long)u * DEEP_NT + tid) * 4;
            const bool in = i < n4;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[u][e] = in ? v[u][e] : -INFINITY;
            if (drop >= i && drop < i + 4) v[u][drop - i] = -INFINITY;
            if constexpr (CEIL) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[u][e] = make_key(v[u][e], (unsigned)(i + e + idx_offset)) > ck ? -INFINITY : v[u][e];
            }
        }
    };
    // pass 1: sixteen running maxima per thread (one per batch slot); the running sum turns NaN if any score is NaN
    float gmax[16], nsum = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) gmax[g] = -INFINITY;
    for (long base = 0; base < n4; base += STEP) {
        f32x4 v[DEEP_UB];
        load_batch(base, v);
#pragma unroll
        for (int u = 0; u < DEEP_UB; ++u) {
            gmax[u % 16] = fmaxf(gmax[u % 16], fmaxf(fmaxf(v[u][0], v[u][1]), fmaxf(v[u][2], v[u][3])));
            nsum += (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
        }
    }
    const bool has_tail = tid < (int)(N - n4) && n4 + tid != drop;
    float tail = has_tail ? row[n4 + tid] : -INFINITY;
    if constexpr (CEIL) tail = make_key(tail, (unsigned)(n4 + tid + idx_offset)) > ck ? -INFINITY : tail;
    gmax[0] = fmaxf(gmax[0], tail);
    nsum += tail;
    // (uniform; fred is written once per query, and the vote below is a barrier)
    const float margin = mg.q ? margin_finish<DEEP_WAVES>(margin_accumulate<DEEP_NT>(mg.q + (long)b * mg.D, mg.D), mg.D, mg.meta, fred) : 0.0f;
    // no room for a NaN score or a margin that is not finite: the exact fallback ranks this query
    if (__syncthreads_or(nsum != nsum || !(margin < INFINITY))) {
        if (tid == 0) { state[b] = 1; flags[0] = 1; }
        return;
    }
    // L = K-th largest group maximum (0: fewer than K groups hold a row -- then every row is collected)
#pragma unroll
    for (int g = 0; g < 16; ++g) ckey[tid * 16 + g] = gmax[g] == -INFINITY ? 0ull : (u64)orderable(gmax[g]) << 32;
    __syncthreads();
    sort_lds_desc<DEEP_NT, 16>(ckey, DEEP_CAP);
    const unsigned lkey = (unsigned)(ckey[K - 1] >> 32);
    __syncthreads();                                 // ckey is reused for the collection
    const float cut0 = lkey != 0 ? unorderable(lkey) - margin : -INFINITY;
    // pass 2: rows with score >= cut0 (never -inf: padding / excluded) -> ranking keys in ckey (one LDS atomic per wave and hit ballot)
    auto collect = [&](float val, long n, bool hit) {
        wave_append_shared(hit, &ncoll, cap, [&](int pos) { ckey[pos] = make_key(val, (unsigned)n); });
    };
    for (long base = 0; base < n4; base += STEP) {
        f32x4 v[DEEP_UB];
        load_batch(base, v);
#pragma unroll
        for (int u = 0; u < DEEP_UB; ++u) {
            const float m4 = fmaxf(fmaxf(v[u][0], v[u][1]), fmaxf(v[u][2], v[u][3]));
            if (__ballot(m4 >= cut0 && m4 > -INFINITY) == 0) continue;
            const long i = base + ((long)u * DEEP_NT + tid) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) collect(v[u][e], i + e, v[u][e] >= cut0 && v[u][e] > -INFINITY);
        }
    }
    collect(tail, n4 + tid, tail >= cut0 && tail > -INFINITY);
    __syncthreads();
    const int nc = ncoll;
    if (nc > cap) {                                  // (uniform) no room: the exact fallback
        if (tid == 0) { state[b] = 1; flags[0] = 1; }
        return;
    }
    sort_keys_desc<DEEP_NT>(ckey, nc);
    if (!mg.q) {                                     // the collected keys are the ranking keys
        for (int r = tid; r < K; r += DEEP_NT) write_key(r < nc ? ckey[r] : 0ull, idx_offset, os + r, oi + r);
        return;
    }
    // pre-filter: survivors = approximate score >= T~ - margin, a prefix of the sorted keys (every collected row when nc < K)
    const float cut = nc >= K ? unorderable((unsigned)(ckey[K - 1] >> 32)) - margin : -INFINITY;
    int cnt = 0;
    for (int r = tid; r < nc; r += DEEP_NT) {
        const bool keep = !(unorderable((unsigned)(ckey[r] >> 32)) < cut);
        cnt += keep;
        if (keep) surv[r] = 0xFFFFFFFFu - (unsigned)ckey[r];
    }
    cnt = wave_sum_i32(cnt);
    if (lane == 0) atomicAdd(&nsurv, cnt);
    for (int i = tid; i < mg.D; i += DEEP_NT) qrow[i] = mg.q[(long)b * mg.D + i];
    __syncthreads();
    const int ns = nsurv;
    // exact chains of the survivors (32 per wave and round), written over the approximate keys
    float* tl = tiles + wave * (2 * RESC_ROWS * RESC_TLD);
    for (int s0 = wave * RESC_ROWS; s0 < ns; s0 += DEEP_WAVES * RESC_ROWS) rescore_keys(surv, s0, ns, qrow, mg.gallery, mg.D, tl, ckey);
    __syncthreads();
    sort_keys_desc<DEEP_NT>(ckey, ns);
    for (int r = tid; r < K; r += DEEP_NT) write_key(r < ns ? ckey[r] : 0ull, idx_offset, os + r, oi + r);
}

// ---- fallback: radix select on the stored (exact / bf16) row, no capacity ---------------------------------------------------------------
// Gated on flags[0] and state[b].  T = the K-th largest key of the row, one 8-bit digit per pass over the row (LDS histogram, one atomic per
// wave and digit value: wave_hist_add); the K keys >= T are collected and sorted.  A row's key is the row-key rule's (kernels.h:
// stored_row_key -- rows scoring -inf and the excluded row take no place, as in the selection kernel) on the LOCAL index, with the
// ceiling as a further condition.
__global__ __launch_bounds__(DEEP_NT) void deep_fallback_kernel(const float* S, long ld, long N, int K, const int* exclude, long idx_offset,
                                                                float* out_scores, int* out_idx, const int* flags, const int* state, const u64* ceil) {
    if (flags[0] == 0 || state[blockIdx.x] == 0) return;
    __shared__ __attribute__((aligned(16))) u64 ckey[4 * DEEP_NT];      // >= 1024: the K keys
    __shared__ int hist[256];
    __shared__ int need_s, sel_s, ncoll;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = S + (long)b * ld;
    float* os = out_scores + (long)b * K;
    int* oi = out_idx + (long)b * K;
    const long drop = excluded_local_row(exclude, b, idx_offset, N);
    const u64 ck = ceil ? ceil[b] : ~0ull;          // a key with the global index: compared with the row's global key, never rebased
    auto under = [&](float v, long n) { return !ceil || make_key(v, (unsigned)(n + idx_offset)) <= ck; };
    u64 prefix = 0, mask = 0;
    int need = K;
    for (int d = 7; d >= 0; --d) {
        for (int i = tid; i < 256; i += DEEP_NT) hist[i] = 0;
        __syncthreads();
        for (long n0 = 0; n0 < N; n0 += DEEP_NT) {
            const long n = n0 + tid;
            const float v = n < N ? row[n] : -INFINITY;
            const u64 key = stored_row_key(v, n, N, drop, 0);      // the select keys: on the LOCAL index
            const bool match = key != 0 && under(v, n) && (key & mask) == prefix;
            wave_hist_add(match, (int)((key >> (8 * d)) & 255), hist);
        }
        __syncthreads();
        if (tid == 0) {
            if (d == 7) {                            // keys in the row: fewer than K -> all of them rank
                int total = 0;
                for (int i = 0; i < 256; ++i) total += hist[i];
                need = total < need ? total : need;
            }
            int sel = 0, cum = 0;
            if (need > 0) {
                for (int i = 255; i >= 0; --i) {
                    if (cum + hist[i] >= need) { sel = i; break; }
                    cum += hist[i];
                }
            }
            need_s = need - cum;
            sel_s = sel;
            if (d == 7) ncoll = need;                // the number of keys that will be collected (need is final here)
        }
        __syncthreads();
        if (ncoll == 0) break;                       // (uniform) nothing ranks
        need = need_s;
        prefix |= (u64)sel_s << (8 * d);
        mask |= 255ull << (8 * d);
        __syncthreads();
    }
    const int want = ncoll;
    __syncthreads();
    if (tid == 0) ncoll = 0;
    __syncthreads();
    if (want > 0) {
        for (long n0 = 0; n0 < N; n0 += DEEP_NT) {
            const long n = n0 + tid;
            const float v = n < N ? row[n] : -INFINITY;
            const u64 key = stored_row_key(v, n, N, drop, 0);
            const bool hit = key != 0 && under(v, n) && key >= prefix;
            wave_append_shared(hit, &ncoll, 4 * DEEP_NT, [&](int pos) { ckey[pos] = key; });
        }
        __syncthreads();
    }
    sort_lds_desc<DEEP_NT, 4>(ckey, want);
    for (int r = tid; r < K; r += DEEP_NT) write_key(r < want ? ckey[r] : 0ull, idx_offset, os + r, oi + r);
}

// ---- merge of R ranked lists, K > 64 ---------------------------------------------------------------------------------------------------
constexpr int MERGE_NT = 1024;
constexpr int MERGE_MAX = MERGE_NT * 16;        // R * K keys of one query in LDS (128 KiB)
__global__ __launch_bounds__(MERGE_NT) void topk_merge_deep_kernel(const float* scores, const int* idx, float* out_scores, int* out_idx, int R, int B,
                                                                   int K) {
    __shared__ __attribute__((aligned(16))) u64 ck[MERGE_MAX];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = R * K;
    for (int i = tid; i < n; i += MERGE_NT) {
        const int r = i / K, j = i - r * K;
        const long o = ((long)r * B + b) * K + j;
        const int gi = idx[o];
        ck[i] = gi >= 0 ? make_key(scores[o], (unsigned)gi) : 0ull;
    }
    __syncthreads();
    if (n <= 2 * MERGE_NT) sort_lds_desc<MERGE_NT, 2>(ck, n);
    else if (n <= 4 * MERGE_NT) sort_lds_desc<MERGE_NT, 4>(ck, n);
    else if (n <= 8 * MERGE_NT) sort_lds_desc<MERGE_NT, 8>(ck, n);
    else sort_lds_desc<MERGE_NT, 16>(ck, n);
    for (int r = tid; r < K; r += MERGE_NT) write_key(ck[r], 0, out_scores + (long)b * K + r, out_idx + (long)b * K + r);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
hipError_t launch_deep_exact_scores(const float* q, const float* gallery, int B, long N, int D, float* S, long ld, int* flags, const int* state,
                                    int gated, hipStream_t s, const RowTags* rt) {
    if (B <= 0 || N <= 0) return hipSuccess;
    if (D <= 0 || D % 8 || ld < N || (gated && !state)) return hipErrorInvalidValue;
    const long ntiles = (N + 31) / 32;
    const int gy = (B + 31) / 32;
    const int gx = (int)std::min<long>((ntiles + 3) / 4, std::max(1, 2048 / gy));
    RowTags tags;
    if (!row_tags_arg(rt, tags)) return hipErrorInvalidValue;
    if (gated)
        FERN_LAUNCH(deep_exact_scores_kernel<true>, dim3(gx, gy), dim3(256), 0, s, q, gallery, B, N, D, S, ld, flags, state, tags);
    else
        FERN_LAUNCH(deep_exact_scores_kernel<false>, dim3(gx, gy), dim3(256), 0, s, q, gallery, B, N, D, S, ld, flags, state, tags);
    return hipGetLastError();
}

hipError_t launch_deep_select(const float* S, long ld, long N, int B, int K, const float* q, const float* meta, const float* gallery, int D,
                              const int* exclude, long idx_offset, float* out_scores, int* out_idx, int* flags, int* state, hipStream_t s,
                              const unsigned long long* ceil) {
    if (B <= 0) return hipSuccess;
    if (K < 1 || K > 1024 || N < 0 || (ld & 3) || ld < N || (ceil && q)) return hipErrorInvalidValue;
    if (q && (!meta || !gallery || D < 64 || D % 64 || D > DEEP_MAX_D)) return hipErrorInvalidValue;
    // test hook: FERN_RANK_DEEP_CAP=c shrinks the collection capacity so that tests reach the fallback
    static const int cap_override = [] { const char* e = std::getenv("FERN_RANK_DEEP_CAP"); return e ? std::atoi(e) : 0; }();
    const int cap = cap_override >= 1 && cap_override <= DEEP_CAP ? cap_override : DEEP_CAP;
    const DeepMargin mg{q, meta, gallery, D};
    if (ceil)
        FERN_LAUNCH(deep_select_kernel<true>, dim3(B), dim3(DEEP_NT), 0, s, S, ld, N, K, mg, exclude, idx_offset, cap, out_scores, out_idx, flags, state, ceil);
    else
        FERN_LAUNCH(deep_select_kernel<false>, dim3(B), dim3(DEEP_NT), 0, s, S, ld, N, K, mg, exclude, idx_offset, cap, out_scores, out_idx, flags, state, ceil);
    return hipGetLastError();
}

hipError_t launch_deep_fallback(const float* S, long ld, long N, int B, int K, const int* exclude, long idx_offset, float* out_scores, int* out_idx,
                                const int* flags, const int* state, hipStream_t s, const unsigned long long* ceil) {
    if (B <= 0) return hipSuccess;
    if (K < 1 || K > 1024 || N < 0 || ld < N) return hipErrorInvalidValue;
    FERN_LAUNCH(deep_fallback_kernel, dim3(B), dim3(DEEP_NT), 0, s, S, ld, N, K, exclude, idx_offset, out_scores, out_idx, flags, state, ceil);
    return hipGetLastError();
}

hipError_t launch_topk_merge_deep(const float* scores, const int* idx, float* out_scores, int* out_idx, int R, int B, int K, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (K < 1 || K > 1024 || R < 1 || (long)R * K > MERGE_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_merge_deep_kernel, dim3(B), dim3(MERGE_NT), 0, s, scores, idx, out_scores, out_idx, R, B, K);
    return hipGetLastError();
}

}  // namespace fern

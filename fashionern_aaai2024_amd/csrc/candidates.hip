// Candidate ranking (include/fern.h: fern_sim_topk_candidates): every query ranks the SET of gallery rows its own list names.
// One workgroup of 256 threads per query, one launch per query chunk, on every gallery form:
//   validity   an entry takes a place iff it names a row of this gallery (shard), is not the query's excluded row and is eligible under
//              the row filter (one gathered tag load); the survivors' local rows are compacted in entry order (ballots and a scan: no
//              atomics, nothing depends on arrival order);
//   scores     fp32 rows: each survivor's sequential fp32 chain (oracle/chain.c order), a wave taking 32 survivors per round through
//              rescore.h's ring (rescore_keys) when D is a whole, even number of 32-k steps, else 16 per round through its per-lane
//              form (chain_rows_lane, as rank.hip's key producer) -- the same chain;
//              bf16 rows: the sweep's v_mfma_f32_32x32x16_bf16 with the sweep's operand roles -- A = the query rounded to bf16 (every A
//              row holds it), B = 32 candidate rows per round, lane (l31, lh) loading row l31's 16-byte k fragments straight from the
//              gathered row, k ascending 16 at a time from a zero accumulator -- so a score has the sweep's bits;
//   order      the 64-bit ranking keys (global row index) are sorted by a bitonic network in LDS over the next power of two, equal
//              adjacent keys -- the same row named twice -- are dropped, the first K are written as (score, global index), and each
//              entry's place is the position of its key among the distinct keys.
// LDS is one dynamic object, sized by the list length: the survivors' keys, their rows, the entries' survivor numbers, then a scratch
// that is first the waves' chain tiles (fp32 form) and then the sorted copy of the keys.
#include "kernels.h"
#include "rescore.h"
#include "select.h"

#include <algorithm>

namespace fern {

typedef short bf16x8c __attribute__((ext_vector_type(8)));

constexpr int CAND_NT = 256;
constexpr int CAND_WAVES = CAND_NT / 64;
constexpr int CAND_TILE = 2 * RESC_ROWS * RESC_TLD;      // floats of one wave's chain tile (rescore.h: double buffered)
constexpr int CAND_ODD_T = CHAIN_T;                      // per-lane form (rescore.h: chain_rows_lane): rows per wave and round ...
constexpr int CAND_ODD_CH = 128;                         // ... k per step
static_assert(chain_tile_floats<CAND_ODD_CH>() <= CAND_TILE, "the per-lane form's rows and the query's step fit one wave's chain tile");
constexpr unsigned short CAND_NONE = 0xFFFFu;            // an entry that takes no place

enum CandForm : int { CAND_F32_RING = 0, CAND_F32_LANE = 1, CAND_BF16 = 2 };

// byte offsets inside the LDS object; the launcher sizes it with the same arithmetic
struct CandLds { int ckey, surv, ent, misc, qb, scratch, bytes; };
__host__ __device__ inline int cand_pow2(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}
__host__ __device__ inline CandLds cand_lds(int M, int D, int form) {
    CandLds l;
    const int per = form == CAND_F32_LANE ? CAND_ODD_T : RESC_ROWS;      // survivors per wave and round
    const int rounds = (M + per - 1) / per;
    const int waves = rounds < CAND_WAVES ? rounds : CAND_WAVES;          // waves that ever hold a round of survivors
    const int tiles = form == CAND_BF16 ? 0 : waves * CAND_TILE * 4, sorted = cand_pow2(M) * 8;
    l.scratch = 0;
    l.ckey = ((tiles > sorted ? tiles : sorted) + 15) & ~15;
    l.surv = l.ckey + ((M * 8 + 15) & ~15);
    l.ent = l.surv + ((M * 4 + 15) & ~15);
    l.misc = l.ent + ((M * 2 + 15) & ~15);
    l.qb = l.misc + 64;
    l.bytes = l.qb + (form == CAND_BF16 ? D * 2 : 0);
    return l;
}

template <int FORM>
__global__ __launch_bounds__(CAND_NT) void candidates_kernel(const float* __restrict__ q, const void* __restrict__ gallery, long N, int D,
                                                             const int* __restrict__ cand, int M, int K, long idx_offset,
                                                             const int* __restrict__ exclude, RowTags rt, float* out_scores, int* out_idx,
                                                             int* out_place) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cand_smem[];
    const CandLds L = cand_lds(M, D, FORM);
    u64* ckey = reinterpret_cast<u64*>(cand_smem + L.ckey);                       // [ns] the survivors' keys, in survivor order
    unsigned* surv = reinterpret_cast<unsigned*>(cand_smem + L.surv);             // [ns] their local rows
    unsigned short* ent = reinterpret_cast<unsigned short*>(cand_smem + L.ent);   // [M] entry -> survivor number, CAND_NONE: takes no place
    int* wtot = reinterpret_cast<int*>(cand_smem + L.misc);
    u64* skey = reinterpret_cast<u64*>(cand_smem + L.scratch);                    // the sorted copy, over the chain tiles
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int* list = cand + (long)b * M;
    const float* qrow = q + (long)b * D;

    // ---- validity: survivors compacted in entry order ----
    const int ex = exclude ? exclude[b] : -1;
    const bool tagged = rt.tags != nullptr;
    const QueryTags qt = query_tags(rt, b);
    if (FORM == CAND_BF16) {      // the query's bf16 image, rounded as the sweep rounds it
        unsigned short* qb = reinterpret_cast<unsigned short*>(cand_smem + L.qb);
        for (int i = tid; i < D; i += CAND_NT) qb[i] = f32_to_bf16_bits(qrow[i]);
    }
    int ns = 0;
    for (int j0 = 0; j0 < M; j0 += CAND_NT) {
        const int j = j0 + tid;
        const int c = j < M ? list[j] : -1;
        const long r = (long)c - idx_offset;
        bool ok = c >= 0 && r >= 0 && r < N && !(exclude && c == ex);
        if (ok && tagged) ok = row_eligible(rt.tags[r], qt.mask, qt.value);
        int total;
        const int p = ns + block_exclusive_scan<CAND_WAVES>(ok ? 1 : 0, wtot, total);
        __syncthreads();                                     // wtot is written again by the next round
        if (ok) surv[p] = (unsigned)r;
        if (j < M) ent[j] = ok ? (unsigned short)p : CAND_NONE;
        ns += total;
    }
    __syncthreads();

    // ---- scores -> ranking keys ckey[0 .. ns), local row index ----
    if (FORM == CAND_F32_RING) {
        float* tl = reinterpret_cast<float*>(cand_smem + L.scratch) + wave * CAND_TILE;
        for (int s0 = wave * RESC_ROWS; s0 < ns; s0 += CAND_WAVES * RESC_ROWS)
            rescore_keys(surv, s0, ns, qrow, reinterpret_cast<const float*>(gallery), D, tl, ckey);
    } else if (FORM == CAND_F32_LANE) {
        // 16 survivors per wave and round through the per-lane chain stager, 128 k per step (eight 16-byte loads per lane and one of
        // the query); the four waves run their rounds independently: the stager synchronises inside the wave only
        float* tl = reinterpret_cast<float*>(cand_smem + L.scratch) + wave * CAND_TILE;
        const float* g = reinterpret_cast<const float*>(gallery);
        for (int s0 = wave * CAND_ODD_T; s0 < ns; s0 += CAND_WAVES * CAND_ODD_T) {
            const float acc = chain_rows_lane<CAND_ODD_CH>([&](int t) { return g + (long)surv[s0 + t < ns ? s0 + t : s0] * D; }, qrow, D, tl);
            if (lane < CAND_ODD_T && s0 + lane < ns) ckey[s0 + lane] = make_key(acc, surv[s0 + lane]);
        }
    } else {
        const unsigned short* g = reinterpret_cast<const unsigned short*>(gallery);
        const unsigned short* qb = reinterpret_cast<const unsigned short*>(cand_smem + L.qb);
        const int l31 = lane & 31, lh = lane >> 5;
        for (int s0 = wave * 32; s0 < ns; s0 += CAND_WAVES * 32) {
            const int s = s0 + l31;
            const unsigned row = surv[s < ns ? s : s0];
            const unsigned short* grow = g + (long)row * D + lh * 8;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            auto steps = [&](int k0) {                       // D % 64 == 0: four k steps, their row fragments in flight together
                bf16x8c bfr[4];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) bfr[ks] = *reinterpret_cast<const bf16x8c*>(grow + k0 + ks * 16);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const bf16x8c afr = *reinterpret_cast<const bf16x8c*>(qb + k0 + ks * 16 + lh * 8);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr, bfr[ks], acc, 0, 0, 0);
                }
            };
            for (int k0 = 0; k0 < D - 64; k0 += 64) steps(k0);
            steps(D - 64);
            // The last four steps stand behind the loop, in the block that reads the accumulator.  With the read right behind the loop's
            // exit branch hipcc emitted v_accvgpr_read directly after the last MFMA, no wait states between them, and on the device the
            // last k step was missing from every score.  A 16-pass MFMA needs 19 wait states before a VALU read of its result: 32 here,
            // fenced against the scheduler, whatever the compiler adds itself.
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            // every A row is the query: register 0 of lane l31 (either half) is the score of candidate row l31
            if (lh == 0 && s < ns) ckey[s] = make_key(acc[0], row);
        }
    }
    __syncthreads();

    // ---- order: global indices into the keys, bitonic sort of a copy, equal neighbours dropped ----
    const int P = cand_pow2(ns);
    for (int i = tid; i < P; i += CAND_NT) {
        u64 k = 0ull;
        if (i < ns) {
            k = (ckey[i] & 0xFFFFFFFF00000000ull) | (u64)(0xFFFFFFFFu - (unsigned)((long)surv[i] + idx_offset));
            ckey[i] = k;
        }
        skey[i] = k;
    }
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < P / 2; i += CAND_NT) {
                const int lo = ((i & ~(jj - 1)) << 1) | (i & (jj - 1)), hi = lo | jj;
                const u64 a = skey[lo], c = skey[hi];
                if ((a < c) == ((lo & kk) == 0)) { skey[lo] = c; skey[hi] = a; }
            }
            __syncthreads();
        }
    }
    // thread t owns the sorted positions [t E, (t + 1) E): its distinct keys move down to their places (all read before any is written)
    const int E = (P + CAND_NT - 1) / CAND_NT;               // <= 16
    u64 mine[16];
    int keep = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int i = tid * E + e;
        const bool in = e < E && i < P;
        mine[e] = in ? skey[i] : 0ull;
        const u64 prev = in && i > 0 ? skey[i - 1] : ~0ull;
        if (mine[e] == prev) mine[e] = 0ull;                  // the same row again (a key of 0: padding)
        keep += mine[e] != 0ull ? 1 : 0;
    }
    int nd;
    int at = block_exclusive_scan<CAND_WAVES>(keep, wtot, nd);      // (its barrier: every read above is done)
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if (mine[e] != 0ull) skey[at++] = mine[e];
    __syncthreads();

    float* os = out_scores + (long)b * K;
    int* oi = out_idx + (long)b * K;
    for (int r = tid; r < K; r += CAND_NT) write_key(r < nd ? skey[r] : 0ull, 0, os + r, oi + r);
    if (out_place) {
        int* op = out_place + (long)b * M;
        for (int j = tid; j < M; j += CAND_NT) {
            const unsigned short p = ent[j];
            int place = -1;
            if (p != CAND_NONE) {                             // the number of distinct keys greater than the entry's
                const u64 key = ckey[p];
                int lo = 0, hi = nd;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (skey[mid] > key) lo = mid + 1; else hi = mid;
                }
                place = lo;
            }
            op[j] = place;
        }
    }
}

template <int FORM>
static hipError_t launch_form(const float* q, const void* gallery, int B, long N, int D, const int* cand, int M, int K, long idx_offset,
                              const int* exclude, const RowTags& rt, float* out_scores, int* out_idx, int* out_place, hipStream_t s) {
    // the attribute is set once, for the longest list: a later call inside a stream capture never has to raise it
    static bool attr_set = false;
    const size_t lds = (size_t)cand_lds(M, D, FORM).bytes;
    auto kern = candidates_kernel<FORM>;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           cand_lds(CAND_MAX_M, 768, FORM).bytes);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    FERN_LAUNCH(kern, dim3((unsigned)B), dim3(CAND_NT), lds, s, q, gallery, N, D, cand, M, K, idx_offset, exclude, rt, out_scores, out_idx, out_place);
    return hipGetLastError();
}

hipError_t launch_candidates(const float* q, const float* gallery, const unsigned short* gallery_bf16, int B, long N, int D, const int* cand, int M,
                             int K, long idx_offset, const int* exclude, const RowTags* rt, float* out_scores, int* out_idx, int* out_place,
                             hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (M < 1 || M > CAND_MAX_M || K < 1 || K > 1024 || D <= 0) return hipErrorInvalidValue;
    RowTags tags;
    if (!row_tags_arg(rt, tags)) return hipErrorInvalidValue;
    if (gallery || N <= 0) {      // (an empty gallery has no survivors: the form does not matter)
        if (D % 32) return hipErrorInvalidValue;
        if ((D / 32) % 2 == 0)
            return launch_form<CAND_F32_RING>(q, gallery, B, N, D, cand, M, K, idx_offset, exclude, tags, out_scores, out_idx, out_place, s);
        return launch_form<CAND_F32_LANE>(q, gallery, B, N, D, cand, M, K, idx_offset, exclude, tags, out_scores, out_idx, out_place, s);
    }
    if (D % 64 || D > 768) return hipErrorInvalidValue;
    return launch_form<CAND_BF16>(q, gallery_bf16, B, N, D, cand, M, K, idx_offset, exclude, tags, out_scores, out_idx, out_place, s);
}

}  // namespace fern

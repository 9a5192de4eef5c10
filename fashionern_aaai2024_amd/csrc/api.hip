// C-ABI layer of libfern.so: the ranking host layer -- one argument check and one score producer under the top-K forms (plain, bf16, pre-filtered,
// filtered, deep, candidates), the item forms, the target ranks and the ranking pages -- with the gallery copies, live-gallery entries, score gathers and list merges.
// Beside it: api_ctx / api_weights / api_fusion / api_towers / api_blocks.hip, over ctx.h.  (Named api.hip still: api_rank.hip is a pure rename away.)
#include <cstdio>
#include <cstdlib>
#include "ctx.h"
#include "live.h"
using namespace fern;
using namespace fern::api;

// Limits and launch shapes that every ranking form shares, each stated once.
static const size_t kRankQueryChunk = 1024;      // queries per plan: bounds cand[m][256][64] (128 KiB per query)
static const double kScoreBudget = 1.1e9;        // workspace bytes that the stored fp32 score rows of one query chunk (and its item table) may take
static const int64_t kMaxRows = 0x7FFFFFF0LL;    // gallery rows of one call: row indices are int32
// queries per launch of the bf16 sweep: 128 where the kernel has the two-block form (D = 64 / 128 / 256 / 512: second block's bf16 image
// in LDS), else 64
static long sweep_qblk(int D) { return (D == 64 || D == 128 || D == 256 || D == 512) ? 128 : 64; }
// the shapes the ranking forms hand to the bf16 sweep (its LDS ring needs >= 3 stages); fern_sim_topk_bf16 alone goes on to D = 1024
static bool sweep_shape_ok(int D) { return D > 0 && D % 64 == 0 && D <= 768; }
// the [B, N] fp32 score matrix of a query chunk is within the budget: the dense form can run
static bool dense_fits(int B, int64_t N) { return (double)std::min<long>(B, (long)kRankQueryChunk) * N * 4 <= kScoreBudget; }
// queries per chunk whose [m, ld] fp32 score rows, plus `extra` bytes per query, stay within the budget (0: one query alone exceeds it)
static long budget_chunk(long ld, double extra = 0) {
    return std::min<long>((long)kRankQueryChunk, (long)(kScoreBudget / ((double)ld * 4 + extra)));
}
static long score_ld(int64_t N) { return std::max<long>(4, (N + 3) & ~3L); }      // row stride of the deep / item / count stages' score rows

// One ranking call as every entry point of this section describes it.  at(o) is the same call from query o on: what a query chunk, or one
// sweep block inside it, is handed.  A null pointer stays null.
struct RankCall {
    const char* fn;                                  // the entry point, for messages
    const float* q; const float* gallery; const uint16_t* gallery_bf16; const float* meta;
    int B; int64_t N; int D;
    int64_t idx_offset; const int32_t* exclude;
    RowTags rt;                                      // tags null: unfiltered
    int K; float* out_scores; int32_t* out_idx;      // the top-K entry points' [B, K] outputs
    RankCall at(long o) const {
        RankCall r = *this;
        if (q) r.q += o * D;
        if (exclude) r.exclude += o;
        if (rt.mask) r.rt.mask += o;
        if (rt.value) r.rt.value += o;
        if (out_scores) r.out_scores += o * K;
        if (out_idx) r.out_idx += o * K;
        return r;
    }
};
static RowTags row_tags(const uint32_t* tags, const uint32_t* mask, const uint32_t* value) {
    return tags ? RowTags{tags, mask, value} : RowTags{nullptr, nullptr, nullptr};
}

// The argument check of every ranking entry point; nothing is dereferenced.  `outs_ok`: the caller's own result (and target / key)
// pointers are all given.  kmax > 0: `count` is K in [1, kmax]; kmax == 0: `count` is the targets per query, m >= 1.
enum GalleryRule {
    GALLERY_FP32, GALLERY_BF16, GALLERY_PREPARED,      // that form's pointers, needed once there is a (query, row) pair to score
    GALLERY_EITHER,                                    // fp32 rows, else bf16 rows: one of them always; both means pre-filtered and needs meta
    GALLERY_EITHER_OR_EMPTY,                           // ... no pointer needed for an empty gallery, which counts as the fp32 form
};
static int rank_check(fern_ctx* c, const RankCall& a, GalleryRule rule, bool outs_ok, int count, int kmax) {
    const std::string fn(a.fn);
    if (kmax && (count < 1 || count > kmax)) return fail(FERN_ERR_ARG, fn + ": need 1<=K<=" + std::to_string(kmax));
    if (!kmax && count < 1) return fail(FERN_ERR_ARG, fn + ": need m >= 1");
    if (a.B < 0 || a.N < 0 || a.D <= 0) return fail(FERN_ERR_ARG, fn + ": need B >= 0, N >= 0, D > 0");
    const bool pairs = a.B && a.N, either = rule == GALLERY_EITHER || rule == GALLERY_EITHER_OR_EMPTY;
    if (rule == GALLERY_FP32 && pairs && !a.gallery) return fail(FERN_ERR_ARG, fn + ": NULL argument");
    if (rule == GALLERY_BF16 && pairs && !a.gallery_bf16) return fail(FERN_ERR_ARG, fn + ": NULL argument");
    if (rule == GALLERY_PREPARED && pairs && (!a.gallery || !a.gallery_bf16 || !a.meta)) return fail(FERN_ERR_ARG, fn + ": NULL argument");
    if (either && !a.gallery && !a.gallery_bf16 && !(rule == GALLERY_EITHER_OR_EMPTY && a.N == 0))
        return fail(FERN_ERR_ARG, fn + ": gallery and gallery_bf16 are both NULL");
    if (rule == GALLERY_EITHER && a.gallery && a.gallery_bf16 && !a.meta)
        return fail(FERN_ERR_ARG, fn + ": the pre-filtered form needs meta from fern_gallery_prepare");
    if (rule == GALLERY_BF16) {      // fern_sim_topk_bf16: the lists form of the sweep, which has no stored rows and takes D up to 1024
        if (a.D % 64 || a.D > 1024) return fail(FERN_ERR_ARG, fn + ": need D % 64 == 0, D <= 1024");
    } else if (!either || a.gallery || (rule == GALLERY_EITHER_OR_EMPTY && a.N == 0)) {
        if (a.D % 32) return fail(FERN_ERR_ARG, fn + ": the fp32 form needs D % 32 == 0");
    } else if (!sweep_shape_ok(a.D)) {
        return fail(FERN_ERR_ARG, fn + ": a bf16-only gallery needs D % 64 == 0, D <= 768");
    }
    if (a.B && (!a.q || !outs_ok)) return fail(FERN_ERR_ARG, fn + ": NULL argument");
    if (a.rt.tags && a.B && (!a.rt.mask || !a.rt.value)) return fail(FERN_ERR_ARG, fn + ": mask or value is NULL");
    if (a.N > kMaxRows) return fail(FERN_ERR_ARG, fn + ": N too large for int32 indices");
    if (!c) return fail(FERN_ERR_ARG, fn + ": ctx is NULL");      // last, as the deep stage always had it: a NULL context hides no other refusal
    return FERN_OK;
}
// budget_chunk() < 1: what one query alone stores (its score row; `table`: the item forms' table too) is past the budget
static int over_budget(const RankCall& a, bool table = false) {
    char gb[16];
    std::snprintf(gb, sizeof gb, "%.1f", kScoreBudget / 1e9);
    return fail(FERN_ERR_ARG, std::string(a.fn) + ": one query's score row" + (table ? " and item table exceed the " : " exceeds the ") + gb + " GB workspace budget");
}

// The bf16 sweep's store form: the scores of m queries against every gallery row into S [m, ld], one launch per qblk queries (64, or
// sweep_qblk(D) without tile maxima).  a: the call at the first of the m queries; its row filter, if any, masks ineligible (query, row)
// pairs to -inf.  flags (optional): zeroed by the first launch.  tmax (optional, [m, ldt]): one maximum per 32-row tile.  st (optional)
// is credited the bytes each launch moves: the bf16 copy once, the block's queries, its [mb, N] fp32 scores out.
static int store_scores(const RankCall& a, int m, float* S, long ld, long qblk, int* flags, float* tmax, long ldt, StageTimer* st, hipStream_t s) {
    for (long b0 = 0; b0 < m; b0 += qblk) {
        const int mb = (int)std::min<long>(qblk, m - b0);
        const RankCall b = a.at(b0);
        HIP_TRY(launch_sweep_bf16(b.q, a.gallery_bf16, S + b0 * ld, ld, mb, a.N, a.D, a.N, 1, nullptr, nullptr, s, b0 == 0 ? flags : nullptr,
                                  tmax ? tmax + b0 * ldt : nullptr, ldt, &b.rt));
        if (st) st->sweep_end((double)a.N * a.D * 2 + (double)mb * a.D * 4 + (double)mb * a.N * 4);
    }
    return FERN_OK;
}

// Score rows of one query chunk, as the deep and the item stages select on: S [m, ld] holds every row's score, -inf for the pairs the
// row filter refuses; flags (4 ints) are zero on the stream behind it (SCORES_EXACT over an empty gallery launches nothing: nothing
// gated follows there).  a: the call at the chunk's first query.
enum ScoreForm {
    SCORES_NONE,       // an empty gallery: only the flags are zeroed
    SCORES_EXACT,      // the fp32 MFMA chain from the fp32 rows
    SCORES_SWEEP,      // the bf16 sweep's store form
};
struct ScoreRows { float* S; int *flags, *state; };
static int score_rows(fern_ctx* c, const RankCall& a, int m, long ld, ScoreForm form, StageTimer& st, hipStream_t s, ScoreRows* R) {
    FERN_TRY(ws_get(c, (size_t)m * ld, &R->S));
    FERN_TRY(ws_get(c, (size_t)4, &R->flags));
    FERN_TRY(ws_get(c, (size_t)m, &R->state));
    st.sweep_begin();
    if (form == SCORES_NONE) {
        HIP_TRY(hipMemsetAsync(R->flags, 0, 4 * sizeof(int), s));
    } else if (form == SCORES_EXACT) {
        HIP_TRY(launch_deep_exact_scores(a.q, a.gallery, m, a.N, a.D, R->S, ld, R->flags, R->state, 0, s, &a.rt));      // also zeroes flags
        st.sweep_end((double)a.N * a.D * 4 + (double)m * a.D * 4 + (double)m * a.N * 4);
    } else {
        FERN_TRY(store_scores(a, m, R->S, ld, 64, R->flags, nullptr, 0, &st, s));
    }
    return FERN_OK;
}

// Fused sweep + selection (kernels.h: TopkFilter): plan and workspace of one query chunk.
//   sample pass   S = max(N / 64, min(N, 4096)) rows, one per run of R = N / S rows, scores stored [m, S]   -> PROF_TOPK
//   bound         per query the K-th best sample key, a lower bound of the true K-th best                   -> PROF_TOPK
//   sweep         the full pass: nothing stored, ~K*R survivors per query appended to its 256 lists         -> PROF_SWEEP
//   select        exact top-K of the lists; a query with an overflowed list is handed to the exact pass     -> PROF_TOPK
//   exact pass    gated on flags[0] (an empty launch unless a list overflowed): streams the gallery for the
//                 flagged queries through sorted wave lists -- no capacity, so the stage is exact whatever
//                 the gallery looks like                                                                    -> PROF_TOPK
struct RankPlan {
    long S; int R; int cap; int groups;
    float* sample; long ld;
    unsigned long long* thr; int* count; int* flags; int* state; int* done;
    unsigned long long* partial;
    TopkFilter filt;
};
static int rank_plan(fern_ctx* c, int m, int64_t N, int K, const int32_t* exclude, int64_t idx_offset, RankPlan* P, long sample_rows = 0) {
    P->S = sample_rows > 0 ? sample_rows : std::min<long>(std::max<long>(N / 64, std::min<long>(N, 4096)), 32768);      // the bound kernel holds a query's sample in registers
    P->R = P->S > 0 ? (int)(N / P->S) : 1;
    // a list sees ~K * R / 256 survivors (<= 16 at K = R = 64; beyond N = 2M rows R grows past 64 and lists start to overflow:
    // those queries are then ranked by the exact pass -- still exact, a gallery pass slower); 64 entries is what one wave load of
    // the select kernel covers
    P->cap = 64;
    static const int cap_override = [] { const char* e = std::getenv("FERN_RANK_CAP"); return e ? std::atoi(e) : 0; }();
    if (cap_override >= 1 && cap_override <= 64) P->cap = cap_override;     // test hook: tiny lists force the overflow -> exact pass path
    P->ld = (std::max<long>(P->S, 4) + 3) & ~3L;
    P->groups = (int)std::min<long>(256, std::max<long>(1, (N + 4095) / 4096));
    FERN_TRY(ws_get(c, (size_t)m * P->ld, &P->sample));
    FERN_TRY(ws_get(c, (size_t)m, &P->thr));
    FERN_TRY(ws_get(c, (size_t)m * RANK_SLOTS, &P->count));
    FERN_TRY(ws_get(c, (size_t)4, &P->flags));
    FERN_TRY(ws_get(c, (size_t)2 * m, &P->state));
    P->done = P->state + m;
    FERN_TRY(ws_get(c, (size_t)m * P->groups * 64, &P->partial));
    unsigned long long* cand;
    FERN_TRY(ws_get(c, (size_t)m * RANK_SLOTS * P->cap, &cand));
    P->filt = TopkFilter{cand, P->thr, P->count, exclude, (long)idx_offset, P->cap};
    return FERN_OK;
}

extern "C" int fern_sim_topk(fern_ctx* c, const float* q, const float* gallery, int B, int64_t N, int D, int K, float* out_scores,
                             int32_t* out_idx, int64_t idx_offset, const int32_t* exclude_idx, void* stream) {
    const RankCall call{"fern_sim_topk", q, gallery, nullptr, nullptr, B, N, D, idx_offset, exclude_idx, {}, K, out_scores, out_idx};
    FERN_TRY(rank_check(c, call, GALLERY_FP32, out_scores && out_idx, K, 64));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, B, (long)kRankQueryChunk, [&](long o, int m) -> int {
        const RankCall a = call.at(o);
        RankPlan P;
        FERN_TRY(rank_plan(c, m, N, K, a.exclude, idx_offset, &P));
        int stage;
        FERN_TRY(prof_open(c, PROF_STAGE, 0, s, &stage));      // the whole stage of this chunk: one marker pair (round 4: three pairs charged their overhead to a ~90 us stage)
        if (P.S > 0) {      // sample pass: the same GEMM, W rows = jittered 1-in-R sample of the gallery
            GemmParams p{};
            p.A = a.q; p.lda = D; p.W = gallery; p.ldw = D; p.C = P.sample; p.ldc = P.ld;
            p.M = m; p.N = (int)P.S; p.K = D; p.epi = EPI_BIAS; p.aload = ALOAD_PLAIN; p.w_sample = P.R;
            HIP_TRY(launch_gemm(p, s));
        }
        HIP_TRY(launch_topk_sample_bound(P.sample, P.ld, m, P.S, P.R, K, a.exclude, idx_offset, P.thr, P.count, P.flags, P.state, s));
        GemmParams p{};
        p.A = a.q; p.lda = D; p.W = gallery; p.ldw = D; p.ldc = 4;
        p.M = m; p.N = (int)N; p.K = D; p.epi = EPI_TOPK_FILTER; p.aload = ALOAD_PLAIN; p.filt = P.filt;
        // algorithmic bytes of the sweep: gallery once, queries, results
        if (N > 0) FERN_TRY(run_gemm(c, p, s, PROF_SWEEP, (double)N * D * 4 + (double)m * D * 4 + (double)m * K * 8));
        HIP_TRY(launch_topk_candidates(P.filt, m, K, idx_offset, a.out_scores, a.out_idx, P.flags, P.state, s));
        HIP_TRY(launch_rank_exact(a.q, gallery, 0, m, N, D, K, P.state, P.thr, a.exclude, idx_offset, idx_offset, P.partial, P.groups, P.done,
                                  a.out_scores, a.out_idx, P.flags, s));
        return prof_close(c, stage, s);
    });
}

// BASELINE config 5 ("bf16 similarity"): the gallery is stored in bf16 (half the HBM bytes), queries are rounded to bf16 in
// the kernel, products accumulate in fp32.  Same outputs and tie rule as fern_sim_topk.
extern "C" int fern_gallery_to_bf16(fern_ctx* c, const float* src, uint16_t* dst, int64_t n, int d, void* stream) {
    if (!c || n < 0 || d <= 0 || (n && (!src || !dst))) return fail(FERN_ERR_ARG, "fern_gallery_to_bf16: bad argument");
    if (d % 4) return fail(FERN_ERR_ARG, "fern_gallery_to_bf16: D must be a multiple of 4");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_f32_to_bf16(src, dst, (long)n * d, (hipStream_t)stream));
    return FERN_OK;
}

// One query chunk of the LISTS form over a bf16 copy: sample pass, bound, filtered sweep into the candidate lists, selection, gated exact
// pass (the plan above), one sweep launch per sweep_qblk(D) queries on shared plan buffers.  a: the call at the chunk's first query.
//   a.gallery null    fern_sim_topk_bf16: the bf16 scores are the ranking scores; the lists' own top-K, the exact pass streams the bf16 rows
//   a.gallery given   the certified pre-filter of fern_sim_topk_prefiltered: a denser sample, the bound lowered by the certified margin,
//                     the survivors rescored with the exact fp32 chain from the fp32 rows, which the exact pass streams too
static long prefilter_sample_rows(int64_t N) {
    // a denser sample than the plain plan's (1 in 32 instead of 1 in 64 beyond 131k rows): the margin lowers the bound by ~0.1 sigma of the
    // score distribution, a tighter sample bound pays that back; 32768 is what the bound kernel holds in registers
    return std::min<long>(std::max<long>(N / 32, std::min<long>(N, 4096)), 32768);
}
static int rank_lists_chunk(fern_ctx* c, const RankCall& a, int m, hipStream_t s) {
    const bool certified = a.gallery != nullptr;
    const int64_t N = a.N;
    const int D = a.D, K = a.K;
    RankPlan P;
    FERN_TRY(rank_plan(c, m, N, K, a.exclude, a.idx_offset, &P, certified ? prefilter_sample_rows(N) : 0));
    float* margin = nullptr;
    if (certified) FERN_TRY(ws_get(c, (size_t)m, &margin));
    const long QBLK = sweep_qblk(D);
    auto block_filter = [&](long b0) {
        TopkFilter f = P.filt;
        f.cand += b0 * RANK_SLOTS * P.cap; f.thr_key += b0; f.count += b0 * RANK_SLOTS;
        if (f.exclude) f.exclude += b0;
        return f;
    };
    StageTimer st(c, s);
    for (long b0 = 0; b0 < m; b0 += QBLK)
        HIP_TRY(launch_sweep_bf16(a.at(b0).q, a.gallery_bf16, P.sample + b0 * P.ld, P.ld, (int)std::min<long>(QBLK, m - b0), N, D, P.S, P.R, nullptr,
                                  nullptr, s));
    HIP_TRY(launch_topk_sample_bound(P.sample, P.ld, m, P.S, P.R, K, a.exclude, a.idx_offset, P.thr, P.count, P.flags, P.state, s,
                                     certified ? a.q : nullptr, certified ? D : 0, certified ? a.meta : nullptr, margin));
    st.sweep_begin();
    for (long b0 = 0; b0 < m; b0 += QBLK) {
        const int mb = (int)std::min<long>(QBLK, m - b0);
        const TopkFilter f = block_filter(b0);
        HIP_TRY(launch_sweep_bf16(a.at(b0).q, a.gallery_bf16, nullptr, 0, mb, N, D, 0, 1, &f, nullptr, s));
        // bytes this kernel streams: the bf16 copy once, the queries, the results; nothing stored (the STAGE's algorithmic bytes -- SURVEY 8d,
        // an fp32 gallery: N D 4 -- are the caller's to quote against the stage time)
        st.sweep_end((double)N * D * 2 + (double)mb * D * 4 + (double)mb * K * 8);
    }
    if (certified)
        HIP_TRY(launch_topk_rescore(P.filt, a.q, a.gallery, D, margin, m, K, a.idx_offset, a.out_scores, a.out_idx, P.flags, P.state, s));
    else
        HIP_TRY(launch_topk_candidates(P.filt, m, K, a.idx_offset, a.out_scores, a.out_idx, P.flags, P.state, s));
    HIP_TRY(launch_rank_exact(a.q, certified ? (const void*)a.gallery : (const void*)a.gallery_bf16, certified ? 0 : 1, m, N, D, K, P.state, P.thr,
                              a.exclude, a.idx_offset, a.idx_offset, P.partial, P.groups, P.done, a.out_scores, a.out_idx, P.flags, s));
    st.commit(m, (int)N, D);
    return FERN_OK;
}

extern "C" int fern_sim_topk_bf16(fern_ctx* c, const float* q, const uint16_t* gallery, int B, int64_t N, int D, int K, float* out_scores,
                                  int32_t* out_idx, int64_t idx_offset, const int32_t* exclude_idx, void* stream) {
    const RankCall call{"fern_sim_topk_bf16", q, nullptr, gallery, nullptr, B, N, D, idx_offset, exclude_idx, {}, K, out_scores, out_idx};
    FERN_TRY(rank_check(c, call, GALLERY_BF16, out_scores && out_idx, K, 64));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, B, (long)kRankQueryChunk, [&](long o, int m) -> int { return rank_lists_chunk(c, call.at(o), m, s); });
}

// The bf16 copy and the three norms that certify it as a pre-filter (include/fern.h): what fern_sim_topk_prefiltered takes.
extern "C" int fern_gallery_prepare(fern_ctx* c, const float* gallery, int64_t N, int D, uint16_t* out_bf16, float* out_meta, void* stream) {
    if (!c || N < 0 || D <= 0 || !out_meta || (N && (!gallery || !out_bf16))) return fail(FERN_ERR_ARG, "fern_gallery_prepare: bad argument");
    if (D % 4) return fail(FERN_ERR_ARG, "fern_gallery_prepare: D must be a multiple of 4");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_gallery_prepare(gallery, out_bf16, (long)N, D, out_meta, (hipStream_t)stream));
    return FERN_OK;
}

// ---- live gallery (include/fern.h; kernels: live.hip) ---------------------------------------------------------------------------
// A slot outside [0, capacity) cannot raise from inside a kernel: the wave writes nothing and stores 1 + its position in the entry's
// host-mapped flag; it is turned into FERN_ERR_ARG here, at fern_sync and at the next call of one of the three entries -- the scheme of
// check_token_flag, without a synchronisation on the launch path.
enum { LIVE_UPSERT = 0, LIVE_MOVE = 1, LIVE_SCATTER = 2, LIVE_ENTRIES = 3 };
static const char* const kLiveNames[LIVE_ENTRIES] = {"fern_gallery_upsert", "fern_gallery_move", "fern_scatter_u32"};
int fern::api::check_live_flags(fern_ctx* c, const char* fn) {
    if (!c->live_flag) return FERN_OK;
    for (int e = 0; e < LIVE_ENTRIES; ++e) {
        const int v = __atomic_load_n(c->live_flag + e, __ATOMIC_RELAXED);
        if (v == 0) continue;
        for (int k = 0; k < LIVE_ENTRIES; ++k) __atomic_store_n(c->live_flag + k, 0, __ATOMIC_RELAXED);
        return fail(FERN_ERR_ARG, std::string(fn) + ": an earlier " + kLiveNames[e] + " on this context was given a slot outside [0, capacity) at position " +
                                      std::to_string(v - 1) + " of its call: that row was not written, the other rows of the call were");
    }
    return FERN_OK;
}
// Common head of the three entries: device, the flags (allocated on first use), the error an earlier call left behind.
static int live_begin(fern_ctx* c, const char* fn) {
    HIP_TRY(hipSetDevice(c->device));
    if (!c->live_flag) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->live_flag), LIVE_ENTRIES * sizeof(int), hipHostMallocMapped));
        for (int e = 0; e < LIVE_ENTRIES; ++e) c->live_flag[e] = 0;
    }
    return check_live_flags(c, fn);
}

extern "C" int fern_gallery_upsert(fern_ctx* c, const float* rows, int64_t ld, const int32_t* slots, int m, float* gallery, uint16_t* gallery_bf16,
                                   float* meta, int64_t capacity, int D, int normalize, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_gallery_upsert: ctx is NULL");
    if (m < 0 || capacity < 0 || D <= 0 || (m && (!rows || !slots))) return fail(FERN_ERR_ARG, "fern_gallery_upsert: bad argument");
    if (!gallery && !gallery_bf16) return fail(FERN_ERR_ARG, "fern_gallery_upsert: give gallery, gallery_bf16 or both");
    if (meta && (!gallery || !gallery_bf16)) return fail(FERN_ERR_ARG, "fern_gallery_upsert: meta belongs to the prepared form (gallery + gallery_bf16 + meta)");
    if (D % 4) return fail(FERN_ERR_ARG, "fern_gallery_upsert: D must be a multiple of 4");
    if (ld < D || ld % 4) return fail(FERN_ERR_ARG, "fern_gallery_upsert: need ld >= D and ld % 4 == 0");
    if (normalize && D > 1280) return fail(FERN_ERR_ARG, "fern_gallery_upsert: normalize needs D <= 1280 (fern_l2_normalize's limit)");
    FERN_TRY(live_begin(c, "fern_gallery_upsert"));
    HIP_TRY(launch_gallery_upsert(rows, (long)ld, slots, m, gallery, gallery_bf16, meta, (long)capacity, D, normalize != 0, c->live_flag + LIVE_UPSERT,
                                  (hipStream_t)stream));
    return FERN_OK;
}

extern "C" int fern_gallery_move(fern_ctx* c, const int32_t* src, const int32_t* dst, int m, float* gallery, uint16_t* gallery_bf16, uint32_t* tags,
                                 int32_t* items, int64_t capacity, int D, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_gallery_move: ctx is NULL");
    if (m < 0 || capacity < 0 || D <= 0 || (m && (!src || !dst))) return fail(FERN_ERR_ARG, "fern_gallery_move: bad argument");
    if (!gallery && !gallery_bf16) return fail(FERN_ERR_ARG, "fern_gallery_move: give gallery, gallery_bf16 or both");
    if (D % 4) return fail(FERN_ERR_ARG, "fern_gallery_move: D must be a multiple of 4");
    FERN_TRY(live_begin(c, "fern_gallery_move"));
    HIP_TRY(launch_gallery_move(src, dst, m, gallery, gallery_bf16, tags, items, (long)capacity, D, c->live_flag + LIVE_MOVE, (hipStream_t)stream));
    return FERN_OK;
}

extern "C" int fern_scatter_u32(fern_ctx* c, const uint32_t* src, const int32_t* slots, int m, uint32_t* dst, int64_t capacity, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_scatter_u32: ctx is NULL");
    if (m < 0 || capacity < 0 || (m && (!src || !slots || !dst))) return fail(FERN_ERR_ARG, "fern_scatter_u32: bad argument");
    FERN_TRY(live_begin(c, "fern_scatter_u32"));
    HIP_TRY(launch_scatter_u32(src, slots, m, dst, (long)capacity, c->live_flag + LIVE_SCATTER, (hipStream_t)stream));
    return FERN_OK;
}

// The bf16 sweep's score matrix and tile maxima on their own (include/fern.h): what the dense form of fern_sim_topk_prefiltered selects on.
extern "C" int fern_sweep_bf16_scores(fern_ctx* c, const float* q, const uint16_t* gallery_bf16, int B, int64_t N, int D, float* scores, int64_t ld,
                                      float* tile_max, int64_t ldt, void* stream) {
    if (!c || B < 0 || N < 0 || !sweep_shape_ok(D)) return fail(FERN_ERR_ARG, "fern_sweep_bf16_scores: need D % 64 == 0, D <= 768");
    if ((long)B * N && (!q || !gallery_bf16 || !scores || ld < N || (tile_max && ldt < (N + 31) / 32)))
        return fail(FERN_ERR_ARG, "fern_sweep_bf16_scores: NULL argument or leading dimension too small");
    HIP_TRY(hipSetDevice(c->device));
    const RankCall a{"fern_sweep_bf16_scores", q, nullptr, gallery_bf16, nullptr, B, N, D, 0, nullptr, {}, 0, nullptr, nullptr};
    return store_scores(a, B, scores, ld, 64, nullptr, tile_max, ldt, nullptr, (hipStream_t)stream);
}

// Which form of the stage runs (results are identical, bit for bit): FERN_RANK_PLAIN = fern_sim_topk's fp32-MFMA sweep;
// FERN_RANK_LISTS = bf16 sample pass + bound - margin + filtered bf16 sweep into candidate lists + rescoring (five launches; for
// galleries whose [B, N] score matrix would be real traffic); FERN_RANK_DENSE = bf16 sweep that stores its scores + one
// select-and-rescore kernel (three launches; small galleries, where the stage is launch boundaries, not bytes).
static int rank_strategy_for(const fern_ctx* c, int B, int64_t N, int D) {
    const bool dense_ok = dense_fits(B, N);      // the [B, N] fp32 score matrix of a query chunk: workspace
    if (c->rank_strategy != FERN_RANK_AUTO) return (c->rank_strategy == FERN_RANK_DENSE && !dense_ok) ? (int)FERN_RANK_LISTS : c->rank_strategy;
    // microseconds, fitted to tools/rank_bench.py on MI355X (profiles/r05_rank_bench.txt): one bf16 pass streams at ~5.8 TB/s behind ~14 us of
    // ramp; the dense sweep also writes its [B, N] scores (~4 TB/s); its select kernel reads N / 32 tile maxima per query when the sweep left
    // them (one 64-query block per launch, >= 16 384 rows: fern_sim_topk_prefiltered), else walks the row twice with ONE workgroup (~60 GB/s)
    const long QBLK2 = sweep_qblk(D);
    const bool tiles = N >= 16384 && (B <= 64 || QBLK2 == 64 || N >= 131072);
    const long qblk = tiles ? 64 : QBLK2;
    const double sweep_us = std::max(17.0, (double)N * D * 2 / 5.8e6 + 14.0), rounds = (double)((B + 255) / 256);
    const double plain = 38.0 + 2.0 * B * (double)N * D / 95e6;                                        // launches + fp32 MFMA at ~95 TFLOP/s (skinny M)
    const double dense = (double)((B + qblk - 1) / qblk) * (sweep_us + (double)std::min<long>(B, qblk) * N * 4 / 4e6) +
                         rounds * (tiles ? 22.0 + (double)N * 3e-5 : 14.0 + (double)N * 8 / 6e4) + 5.0;
    const double lists = (double)((B + QBLK2 - 1) / QBLK2) * (sweep_us + 25.0) + 16.0 * rounds + 45.0;
    int best = FERN_RANK_PLAIN;
    double t = plain;
    if (lists < t) { best = FERN_RANK_LISTS; t = lists; }
    if (dense_ok && dense < t) best = FERN_RANK_DENSE;
    return best;
}

// One query chunk (m <= kRankQueryChunk) of the DENSE form: the bf16 sweep stores its [m, N] scores (and tile maxima), one kernel per query
// selects, rescores and ranks.  a: the call at the chunk's first query.  With a row filter (fern_sim_topk_filtered) the sweep masks
// ineligible (query, row) pairs to -inf, the exact fallbacks apply the same predicate -- the select kernels run as they are on the masked rows.
static int rank_dense_chunk(fern_ctx* c, const RankCall& a, int m, hipStream_t s) {
    const int64_t N = a.N;
    const int D = a.D, K = a.K;
    const long ld = (N + 31) & ~31L, ldt = (((N + 31) >> 5) + 3) & ~3L;      // whole 32-row tiles; one maximum per tile
    // the sweep leaves tile maxima for the select kernel when it runs one 64-query block per launch; two-block sweeps (65..128
    // queries, D a power of two) have no registers for it: kept below 131 072 rows, where walking the rows costs less than a second
    // gallery pass
    const long QBLK = (m > 64 && N < 131072) ? sweep_qblk(D) : 64;
    const bool tiles = QBLK == 64 && N >= 16384;
    const int groups = (int)std::min<long>(256, std::max<long>(1, (N + 4095) / 4096));
    float *approx, *tmax; unsigned long long *thr, *partial; int *flags, *state;
    FERN_TRY(ws_get(c, (size_t)m * ld, &approx));
    FERN_TRY(ws_get(c, (size_t)m * ldt, &tmax));
    FERN_TRY(ws_get(c, (size_t)m, &thr));
    FERN_TRY(ws_get(c, (size_t)4, &flags));
    FERN_TRY(ws_get(c, (size_t)2 * m, &state));
    FERN_TRY(ws_get(c, (size_t)m * groups * 64, &partial));
    StageTimer st(c, s);
    st.sweep_begin();
    FERN_TRY(store_scores(a, m, approx, ld, QBLK, flags, tiles ? tmax : nullptr, ldt, &st, s));
    // small galleries: a query without room is ranked by its own workgroup inside the kernel (one CU streams <= 128 MB of fp32 rows:
    // <= ~2 ms in a case that almost never happens) and the gated exact-pass launch -- ~4.5 us of every call -- is not made
    const bool inline_exact = (double)N * D * 4 <= 128e6;
    HIP_TRY(launch_topk_dense_rescore(approx, ld, N, a.q, a.gallery, D, a.meta, m, K, a.exclude, a.idx_offset, a.idx_offset, a.out_scores, a.out_idx, thr,
                                      flags, state, state + m, s, inline_exact ? 1 : 0, tiles ? tmax : nullptr, ldt, &a.rt));
    if (!inline_exact)
        HIP_TRY(launch_rank_exact(a.q, a.gallery, 0, m, N, D, K, state, thr, a.exclude, a.idx_offset, a.idx_offset, partial, groups, state + m,
                                  a.out_scores, a.out_idx, flags, s, &a.rt));
    st.commit(m, (int)N, D);
    return FERN_OK;
}

extern "C" int fern_rank_set_strategy(fern_ctx* c, int strategy) {
    if (!c || strategy < FERN_RANK_AUTO || strategy > FERN_RANK_DENSE) return fail(FERN_ERR_ARG, "fern_rank_set_strategy: unknown strategy");
    c->rank_strategy = strategy;
    return FERN_OK;
}

// Certified bf16 pre-filter + exact fp32 rescoring (include/fern.h: fern_sim_topk_prefiltered) in the form rank_strategy_for picks: per
// query chunk rank_lists_chunk or rank_dense_chunk.  Shapes the bf16 sweep does not cover run fern_sim_topk (same results by definition).
extern "C" int fern_sim_topk_prefiltered(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, const float* meta, int B,
                                         int64_t N, int D, int K, float* out_scores, int32_t* out_idx, int64_t idx_offset,
                                         const int32_t* exclude_idx, void* stream) {
    const RankCall call{"fern_sim_topk_prefiltered", q, gallery, gallery_bf16, meta, B, N, D, idx_offset, exclude_idx, {}, K, out_scores, out_idx};
    FERN_TRY(rank_check(c, call, GALLERY_PREPARED, out_scores && out_idx, K, 64));
    const int strategy = (!sweep_shape_ok(D) || N == 0 || B == 0) ? (int)FERN_RANK_PLAIN : rank_strategy_for(c, B, N, D);
    if (strategy == FERN_RANK_PLAIN)
        return fern_sim_topk(c, q, gallery, B, N, D, K, out_scores, out_idx, idx_offset, exclude_idx, stream);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, B, (long)kRankQueryChunk, [&](long o, int m) -> int {
        return strategy == FERN_RANK_DENSE ? rank_dense_chunk(c, call.at(o), m, s) : rank_lists_chunk(c, call.at(o), m, s);
    });
}

extern "C" int fern_gather_scores(fern_ctx* c, const float* q, const float* gallery, const int32_t* idx, float* out, int B, int m, int D,
                                  void* stream) {
    if (!c || B < 0 || m < 0 || D <= 0 || ((long)B * m && (!q || !gallery || !idx || !out))) return fail(FERN_ERR_ARG, "fern_gather_scores: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_gather_scores(q, gallery, idx, out, B, m, D, (hipStream_t)stream));
    return FERN_OK;
}

extern "C" int fern_topk_merge(fern_ctx* c, const float* scores, const int32_t* idx, float* out_scores, int32_t* out_idx, int R, int B, int K,
                               void* stream) {
    if (!c || R < 1 || B < 0 || K < 1 || K > 1024 || (B && (!scores || !idx || !out_scores || !out_idx))) return fail(FERN_ERR_ARG, "fern_topk_merge: bad argument");
    if (K > 64 && (long)R * K > 16384) return fail(FERN_ERR_ARG, "fern_topk_merge: need R * K <= 16384 for K > 64");
    HIP_TRY(hipSetDevice(c->device));
    if (K <= 64) HIP_TRY(launch_topk_merge(scores, idx, out_scores, out_idx, R, B, K, (hipStream_t)stream));
    else HIP_TRY(launch_topk_merge_deep(scores, idx, out_scores, out_idx, R, B, K, (hipStream_t)stream));
    return FERN_OK;
}

// Deep ranking (include/fern.h: fern_sim_topk_deep), per query chunk: scores of every row into a [m, ld] workspace (exact: the fp32 MFMA
// chain; pre-filtered / bf16: the bf16 sweep's store form), one select kernel per query (topk_deep.hip), then the gated exact rows
// (pre-filter only) and the gated radix-select fallback for the queries the select kernel had no room for.  Nothing is read back.
// With a row filter (fern_sim_topk_filtered) both score producers store -inf for ineligible (query, row) pairs -- the gated rewrite of
// flagged rows too -- and rows scoring -inf take no place in the select kernel (never collected, so never rescored) or in the radix
// fallback.  `call` has passed rank_check (GALLERY_EITHER, K <= 1024).
static int sim_topk_deep_impl(fern_ctx* c, const RankCall& call, void* stream) {
    const int64_t N = call.N;
    const int D = call.D, K = call.K;
    const long ld = score_ld(N);
    const long chunk = budget_chunk(ld);      // the [m, ld] fp32 score matrix of a chunk stays within the dense form's budget
    if (chunk < 1) return over_budget(call);
    const bool pre = call.gallery && call.gallery_bf16 && sweep_shape_ok(D) && c->rank_strategy != FERN_RANK_PLAIN && N > 0;
    // an empty gallery has no scores to compute (the exact chain launches nothing): the select kernel writes the -inf / -1 rows
    const ScoreForm form = (call.gallery || N == 0) && !pre ? SCORES_EXACT : SCORES_SWEEP;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, call.B, chunk, [&](long o, int m) -> int {
        const RankCall a = call.at(o);
        ScoreRows r;
        StageTimer st(c, s);
        FERN_TRY(score_rows(c, a, m, ld, form, st, s, &r));
        HIP_TRY(launch_deep_select(r.S, ld, N, m, K, pre ? a.q : nullptr, pre ? a.meta : nullptr, pre ? a.gallery : nullptr, D, a.exclude, a.idx_offset,
                                   a.out_scores, a.out_idx, r.flags, r.state, s));
        if (N > 0) {
            if (pre) HIP_TRY(launch_deep_exact_scores(a.q, a.gallery, m, N, D, r.S, ld, r.flags, r.state, 1, s, &a.rt));
            HIP_TRY(launch_deep_fallback(r.S, ld, N, m, K, a.exclude, a.idx_offset, a.out_scores, a.out_idx, r.flags, r.state, s));
        }
        st.commit(m, (int)N, D);
        return FERN_OK;
    });
}

extern "C" int fern_sim_topk_deep(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, const float* meta, int B,
                                  int64_t N, int D, int K, float* out_scores, int32_t* out_idx, int64_t idx_offset, const int32_t* exclude_idx,
                                  void* stream) {
    const RankCall call{"fern_sim_topk_deep", q, gallery, gallery_bf16, meta, B, N, D, idx_offset, exclude_idx, {}, K, out_scores, out_idx};
    FERN_TRY(rank_check(c, call, GALLERY_EITHER, out_scores && out_idx, K, 1024));
    return sim_topk_deep_impl(c, call, stream);
}

// Candidate ranking (include/fern.h: fern_sim_topk_candidates; candidates.hip): one launch per query chunk, one workgroup per query, no
// workspace and nothing read back.  fp32 rows rank when they are given: a bf16 copy beside them is not looked at.
extern "C" int fern_sim_topk_candidates(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D,
                                        const int32_t* cand, int M, int K, float* out_scores, int32_t* out_idx, int32_t* out_place,
                                        int64_t idx_offset, const int32_t* exclude_idx, const uint32_t* tags, const uint32_t* mask,
                                        const uint32_t* value, void* stream) {
    const RankCall call{"fern_sim_topk_candidates", q, gallery, gallery ? nullptr : gallery_bf16, nullptr, B, N, D, idx_offset, exclude_idx,
                        row_tags(tags, mask, value), K, out_scores, out_idx};
    if (M < 1 || M > CAND_MAX_M) return fail(FERN_ERR_ARG, std::string(call.fn) + ": need 1<=M<=" + std::to_string(CAND_MAX_M));
    FERN_TRY(rank_check(c, call, GALLERY_EITHER_OR_EMPTY, cand && out_scores && out_idx, K, 1024));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, B, (long)kRankQueryChunk, [&](long o, int m) -> int {
        const RankCall a = call.at(o);
        StageTimer st(c, s);
        st.sweep_begin();
        HIP_TRY(launch_candidates(a.q, a.gallery, a.gallery_bf16, m, N, D, cand + o * M, M, K, idx_offset, a.exclude, &a.rt, a.out_scores, a.out_idx,
                                  out_place ? out_place + o * M : nullptr, s));
        // bytes the launch must move: every named row once per query, the queries, the lists, the results
        st.sweep_end((double)m * M * D * (a.gallery ? 4 : 2) + (double)m * D * 4 + (double)m * M * (out_place ? 8 : 4) + (double)m * K * 8);
        st.commit(m, (int)N, D);
        return FERN_OK;
    });
}

// Item-level ranking (include/fern.h: fern_sim_topk_items, fern_item_rank; items.hip), per query chunk: the deep stage's score rows S [m, ld]
// (exact: the fp32 MFMA chain; bf16: the sweep's store form), the table best [m, G] of every item's greatest key, then
//   top-K    every row but its item's representative becomes -inf and the deep stage's select + radix fallback run unchanged on the rows
//            (margin 0: the stored scores are the ranking scores), out_item is gathered from out_idx;
//   ranks    a count over the table per target.
// A chunk keeps its score rows plus its table inside the deep stage's budget.  Nothing is read back.
struct ItemCall {
    RankCall call; const int32_t* items; int G;
    long ld() const { return score_ld(call.N); }
    long chunk() const { return budget_chunk(ld(), (double)G * 8); }      // ... and the [m, G] 64-bit table
};
static ItemCall item_call(const char* fn, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D,
                          const int32_t* items, int G, int64_t idx_offset, const int32_t* exclude_idx, const uint32_t* tags, const uint32_t* mask,
                          const uint32_t* value, int K = 0, float* out_scores = nullptr, int32_t* out_idx = nullptr) {
    // fp32 rows rank when they are given: the item forms have no pre-filtered form, so a bf16 copy beside them is not looked at
    return ItemCall{{fn, q, gallery, gallery ? nullptr : gallery_bf16, nullptr, B, N, D, idx_offset, exclude_idx, row_tags(tags, mask, value), K, out_scores, out_idx},
                    items, G};
}
static int item_check(fern_ctx* c, const ItemCall& a, bool outs_ok, int count, int kmax) {
    const std::string fn(a.call.fn);
    FERN_TRY(rank_check(c, a.call, GALLERY_EITHER, outs_ok, count, kmax));
    if (a.G < 1) return fail(FERN_ERR_ARG, fn + ": need G >= 1");
    if (!a.items) return fail(FERN_ERR_ARG, fn + ": items is NULL");
    return a.chunk() < 1 ? over_budget(a.call, true) : FERN_OK;
}
// score rows of the m queries `a` starts at and their table; the flags are zero on the stream for the selection that may follow
struct ItemTable { ScoreRows r; unsigned long long* best; ItemRows rows; };
static int item_chunk_table(fern_ctx* c, const RankCall& a, const ItemCall& it, int m, StageTimer& st, hipStream_t s, ItemTable* T) {
    FERN_TRY(score_rows(c, a, m, it.ld(), a.N == 0 ? SCORES_NONE : a.gallery ? SCORES_EXACT : SCORES_SWEEP, st, s, &T->r));
    FERN_TRY(ws_get(c, (size_t)m * it.G, &T->best));
    T->rows = ItemRows{it.items, it.G, (long)a.N, (long)a.idx_offset, a.exclude, a.rt, 0};
    HIP_TRY(hipMemsetAsync(T->best, 0, (size_t)m * it.G * sizeof(unsigned long long), s));      // on the stream, behind the score kernels: inside the timed stage, re-run by a replayed graph
    HIP_TRY(launch_item_best(T->r.S, it.ld(), m, T->rows, T->best, s));
    return FERN_OK;
}

extern "C" int fern_sim_topk_items(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D, int K,
                                   const int32_t* items, int G, float* out_scores, int32_t* out_idx, int32_t* out_item, int64_t idx_offset,
                                   const int32_t* exclude_idx, const uint32_t* tags, const uint32_t* mask, const uint32_t* value, void* stream) {
    const ItemCall it = item_call("fern_sim_topk_items", q, gallery, gallery_bf16, B, N, D, items, G, idx_offset, exclude_idx, tags, mask, value, K,
                                  out_scores, out_idx);
    FERN_TRY(item_check(c, it, out_scores && out_idx && out_item, K, 1024));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, B, it.chunk(), [&](long o, int m) -> int {
        const RankCall a = it.call.at(o);
        ItemTable T;
        StageTimer st(c, s);
        FERN_TRY(item_chunk_table(c, a, it, m, st, s, &T));
        HIP_TRY(launch_item_keep_best(T.r.S, it.ld(), m, T.rows, T.best, s));
        HIP_TRY(launch_deep_select(T.r.S, it.ld(), N, m, K, nullptr, nullptr, nullptr, D, a.exclude, idx_offset, a.out_scores, a.out_idx, T.r.flags, T.r.state, s));
        if (N > 0) HIP_TRY(launch_deep_fallback(T.r.S, it.ld(), N, m, K, a.exclude, idx_offset, a.out_scores, a.out_idx, T.r.flags, T.r.state, s));
        HIP_TRY(launch_item_gather(a.out_idx, m, K, items, N, G, idx_offset, out_item + o * K, s));
        st.commit(m, (int)N, D);
        return FERN_OK;
    });
}

// keys_in null: the targets' own keys (best[b][target_items[b][j]]); out_keys / out_rank may be null (fern_item_keys / fern_item_count)
static int item_rank_impl(fern_ctx* c, const ItemCall& it, bool outs_ok, const int32_t* target_items, const uint64_t* keys_in, int m, uint64_t* out_keys,
                          int32_t* out_rank, void* stream) {
    FERN_TRY(item_check(c, it, outs_ok, m, 0));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, it.call.B, it.chunk(), [&](long o, int mq) -> int {
        ItemTable T;
        unsigned long long* keys;
        StageTimer st(c, s);
        FERN_TRY(item_chunk_table(c, it.call.at(o), it, mq, st, s, &T));
        if (keys_in) {
            keys = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(keys_in)) + o * m;
        } else {
            if (out_keys) keys = reinterpret_cast<unsigned long long*>(out_keys) + o * m;
            else FERN_TRY(ws_get(c, (size_t)mq * m, &keys));
            HIP_TRY(launch_item_keys(T.best, it.G, target_items + o * m, mq, m, keys, s));
        }
        if (out_rank) HIP_TRY(launch_item_count(T.best, it.G, keys, mq, m, out_rank + o * m, s));
        st.commit(mq, (int)it.call.N, it.call.D);
        return FERN_OK;
    });
}

extern "C" int fern_item_rank(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D,
                              const int32_t* items, int G, const int32_t* target_items, int m, int64_t idx_offset, const int32_t* exclude_idx,
                              int32_t* out_rank, const uint32_t* tags, const uint32_t* mask, const uint32_t* value, void* stream) {
    const ItemCall it = item_call("fern_item_rank", q, gallery, gallery_bf16, B, N, D, items, G, idx_offset, exclude_idx, tags, mask, value);
    return item_rank_impl(c, it, target_items && out_rank, target_items, nullptr, m, nullptr, out_rank, stream);
}

extern "C" int fern_item_keys(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D,
                              const int32_t* items, int G, const int32_t* target_items, int m, int64_t idx_offset, const int32_t* exclude_idx,
                              uint64_t* out_keys, const uint32_t* tags, const uint32_t* mask, const uint32_t* value, void* stream) {
    const ItemCall it = item_call("fern_item_keys", q, gallery, gallery_bf16, B, N, D, items, G, idx_offset, exclude_idx, tags, mask, value);
    return item_rank_impl(c, it, target_items && out_keys, target_items, nullptr, m, out_keys, nullptr, stream);
}

extern "C" int fern_item_count(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D,
                               const int32_t* items, int G, const uint64_t* keys, int m, int64_t idx_offset, const int32_t* exclude_idx,
                               int32_t* out_count, const uint32_t* tags, const uint32_t* mask, const uint32_t* value, void* stream) {
    const ItemCall it = item_call("fern_item_count", q, gallery, gallery_bf16, B, N, D, items, G, idx_offset, exclude_idx, tags, mask, value);
    return item_rank_impl(c, it, keys && out_count, nullptr, keys, m, nullptr, out_count, stream);
}

// Filtered ranking (include/fern.h: fern_sim_topk_filtered): the exact ranking of the rows that are eligible for each query.  Two forms,
// the same bits from both:
//   masked dense form   K <= 64, a prepared gallery (fp32 + bf16 copy + meta), a shape the bf16 sweep takes, the dense form's score budget,
//                       strategy not PLAIN: rank_dense_chunk with the row filter -- the masked store-form sweep + the tiles / dense select kernels;
//   deep stage          everything else: sim_topk_deep_impl on masked rows (exact, pre-filtered or bf16 by the pointers given).
extern "C" int fern_sim_topk_filtered(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, const float* meta, int B,
                                      int64_t N, int D, int K, float* out_scores, int32_t* out_idx, int64_t idx_offset, const int32_t* exclude_idx,
                                      const uint32_t* tags, const uint32_t* mask, const uint32_t* value, void* stream) {
    if (!tags) return fail(FERN_ERR_ARG, "fern_sim_topk_filtered: tags is NULL (unfiltered callers use fern_sim_topk_deep and its siblings)");
    const RankCall call{"fern_sim_topk_filtered", q, gallery, gallery_bf16, meta, B, N, D, idx_offset, exclude_idx, row_tags(tags, mask, value), K, out_scores, out_idx};
    FERN_TRY(rank_check(c, call, GALLERY_EITHER, out_scores && out_idx, K, 1024));
    const bool dense = K <= 64 && B > 0 && N > 0 && gallery && gallery_bf16 && sweep_shape_ok(D) && c->rank_strategy != FERN_RANK_PLAIN && dense_fits(B, N);
    if (!dense) return sim_topk_deep_impl(c, call, stream);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, B, (long)kRankQueryChunk, [&](long o, int m) -> int { return rank_dense_chunk(c, call.at(o), m, s); });
}

// Exact target ranks (include/fern.h: fern_rank_keys, fern_rank_count).  A rank is the number of rows whose key is greater than the
// target's, so the stage is one more sweep with a counting epilogue: no list, no capacity, no fallback, nothing read back.
//   fp32 form   keys: the fma chain on the gathered rows (rank.hip); counts: the fp32 sweep with EPI_RANK_COUNT through run_gemm -- the
//               tuner and the profiling hooks apply, the f32x3 split never does (PROF_SWEEP, and split_ok() does not list the epilogue)
//   bf16 form   keys: the targets' rows as a small gallery through the bf16 sweep's store form; counts: the sweep's store form per query
//               chunk (the deep stage's budget) + a kernel that reads each stored score row once per RANKC_T targets
extern "C" int fern_rank_keys(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D,
                              const int32_t* targets, int m, int64_t idx_offset, uint64_t* out_keys, void* stream) {
    const RankCall call{"fern_rank_keys", q, gallery, gallery_bf16, nullptr, B, N, D, idx_offset, nullptr, {}, 0, nullptr, nullptr};
    FERN_TRY(rank_check(c, call, GALLERY_EITHER_OR_EMPTY, targets && out_keys, m, 0));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) return FERN_OK;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(out_keys);
    if (gallery || N == 0) {
        int stage;
        FERN_TRY(prof_open(c, PROF_STAGE, 0, s, &stage));
        HIP_TRY(launch_rank_keys(q, gallery, targets, B, N, D, m, idx_offset, keys, s));
        return prof_close(c, stage, s);
    }
    // bf16 form: 64-query blocks, each against the 64 m gathered rows of its own targets (a gallery of its own per block: not store_scores)
    const long ld = ((long)64 * m + 3) & ~3L;
    const long chunk = std::max<long>(64, std::min<long>((long)kRankQueryChunk, ((long)(256e6 / ((double)m * D * 2))) & ~63L));
    return for_query_chunks(c, s, B, chunk, [&](long o, int mq) -> int {
        unsigned short* rows; float* S;
        FERN_TRY(ws_get(c, (size_t)mq * m * D, &rows));
        FERN_TRY(ws_get(c, (size_t)mq * ld, &S));
        StageTimer st(c, s);
        HIP_TRY(launch_rank_gather_bf16(gallery_bf16, targets + o * m, (long)mq * m, N, D, idx_offset, rows, s));
        st.sweep_begin();
        for (long b0 = 0; b0 < mq; b0 += 64) {
            const int mb = (int)std::min<long>(64, mq - b0);
            HIP_TRY(launch_sweep_bf16(call.at(o + b0).q, rows + b0 * m * D, S + b0 * ld, ld, mb, (long)mb * m, D, (long)mb * m, 1, nullptr, nullptr, s));
            st.sweep_end((double)mb * m * D * 2 + (double)mb * D * 4 + (double)mb * mb * m * 4);
        }
        HIP_TRY(launch_rank_keys_from_scores(S, ld, targets + o * m, mq, N, m, idx_offset, keys + o * m, s));
        st.commit(mq, (int)N, D);
        return FERN_OK;
    });
}

// With a row filter (fern_rank_count_filtered) a row that is ineligible for a query carries key 0 for it, like the excluded row.
static int rank_count_impl(fern_ctx* c, const RankCall& call, const uint64_t* keys_in, int m, int32_t* out_count, void* stream) {
    FERN_TRY(rank_check(c, call, GALLERY_EITHER_OR_EMPTY, keys_in && out_count, m, 0));
    const int64_t N = call.N;
    const int D = call.D;
    const bool bf16_form = !call.gallery && N > 0;
    const long ld = score_ld(N);
    long chunk = (long)kRankQueryChunk;
    if (bf16_form) {      // the [m, ld] fp32 score matrix of a chunk stays within the dense form's budget, in whole 64-query sweep blocks
        chunk = budget_chunk(ld);
        if (chunk < 1) return over_budget(call);
        if (chunk > 64) chunk &= ~63L;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(keys_in);
    return for_query_chunks(c, s, call.B, chunk, [&](long o, int mq) -> int {
        const RankCall a = call.at(o);
        int* partial;
        FERN_TRY(ws_get(c, (size_t)RANKC_P * mq * RANKC_T, &partial));
        const size_t partial_bytes = (size_t)RANKC_P * mq * RANKC_T * sizeof(int);
        auto pass = [&](int t0) {
            return RankCount{keys + o * m + t0, partial, a.exclude, (long)a.idx_offset, (long)a.idx_offset, m, std::min(RANKC_T, m - t0), a.rt};
        };
        if (!bf16_form) {
            int stage;
            FERN_TRY(prof_open(c, PROF_STAGE, 0, s, &stage));
            for (int t0 = 0; t0 < m; t0 += RANKC_T) {
                GemmParams p{};
                p.A = a.q; p.lda = D; p.W = a.gallery; p.ldw = D; p.ldc = 4;
                p.M = mq; p.N = (int)N; p.K = D; p.epi = EPI_RANK_COUNT; p.aload = ALOAD_PLAIN; p.rankc = pass(t0);
                HIP_TRY(hipMemsetAsync(partial, 0, partial_bytes, s));
                if (N > 0) FERN_TRY(run_gemm(c, p, s, PROF_SWEEP, (double)N * D * 4 + (double)mq * D * 4 + (double)mq * p.rankc.nt * 12));
                HIP_TRY(launch_rank_finalize(p.rankc, mq, out_count + o * m + t0, m, s));
            }
            return prof_close(c, stage, s);
        }
        float* S;
        FERN_TRY(ws_get(c, (size_t)mq * ld, &S));
        StageTimer st(c, s);
        st.sweep_begin();
        FERN_TRY(store_scores(a, mq, S, ld, 64, nullptr, nullptr, 0, &st, s));
        for (int t0 = 0; t0 < m; t0 += RANKC_T) {
            const RankCount rc = pass(t0);
            HIP_TRY(hipMemsetAsync(partial, 0, partial_bytes, s));
            HIP_TRY(launch_rank_count_rows(S, ld, mq, N, rc, s));
            HIP_TRY(launch_rank_finalize(rc, mq, out_count + o * m + t0, m, s));
        }
        st.commit(mq, (int)N, D);
        return FERN_OK;
    });
}

extern "C" int fern_rank_count(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D,
                               const uint64_t* keys_in, int m, int64_t idx_offset, const int32_t* exclude_idx, int32_t* out_count, void* stream) {
    const RankCall call{"fern_rank_count", q, gallery, gallery_bf16, nullptr, B, N, D, idx_offset, exclude_idx, {}, 0, nullptr, nullptr};
    return rank_count_impl(c, call, keys_in, m, out_count, stream);
}

extern "C" int fern_rank_count_filtered(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D,
                                        const uint64_t* keys_in, int m, int64_t idx_offset, const int32_t* exclude_idx, int32_t* out_count,
                                        const uint32_t* tags, const uint32_t* mask, const uint32_t* value, void* stream) {
    if (!tags) return fail(FERN_ERR_ARG, "fern_rank_count_filtered: tags is NULL (unfiltered callers use fern_rank_count)");
    const RankCall call{"fern_rank_count_filtered", q, gallery, gallery_bf16, nullptr, B, N, D, idx_offset, exclude_idx, row_tags(tags, mask, value), 0, nullptr, nullptr};
    return rank_count_impl(c, call, keys_in, m, out_count, stream);
}

// Ranking pages (include/fern.h: fern_rank_select, fern_sim_topk_from, fern_sim_topk_page; page.hip), per query chunk: the deep stage's
// score rows S [m, ld] once (exact: the fp32 MFMA chain; bf16: the sweep's store form; ineligible pairs stored as -inf), then
//   select   the multi-workgroup radix select on the rows: the key at each place, SEL_T places per walk;
//   from     the deep stage's select + radix fallback with a per-query key ceiling (margin 0: the stored scores are the ranking scores);
//   page     both on the same rows: the select writes the key at place offsets[b] into workspace, which is the selection's ceiling.
// A chunk keeps its score rows plus the select's histograms inside the deep stage's budget.  Nothing is read back.
struct PageCall {
    RankCall call;
    long ld() const { return score_ld(call.N); }
    long chunk() const { return budget_chunk(ld(), (double)SEL_T * (8 * 256 * sizeof(unsigned) + 9 * sizeof(SelectState) + 8)); }      // ... and the select's workspace
    ScoreForm form() const { return call.N == 0 ? SCORES_NONE : call.gallery ? SCORES_EXACT : SCORES_SWEEP; }
};
static PageCall page_call(const char* fn, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D, int64_t idx_offset,
                          const int32_t* exclude_idx, const uint32_t* tags, const uint32_t* mask, const uint32_t* value, int K = 0,
                          float* out_scores = nullptr, int32_t* out_idx = nullptr) {
    // fp32 rows rank when they are given: there is no pre-filtered form, so a bf16 copy beside them is not looked at
    return PageCall{{fn, q, gallery, gallery ? nullptr : gallery_bf16, nullptr, B, N, D, idx_offset, exclude_idx, row_tags(tags, mask, value), K, out_scores, out_idx}};
}
static int page_check(fern_ctx* c, const PageCall& p, bool outs_ok, int count, int kmax) {
    FERN_TRY(rank_check(c, p.call, GALLERY_EITHER, outs_ok, count, kmax));
    return p.chunk() < 1 ? over_budget(p.call) : FERN_OK;
}
// keys[b][j] = the key at place places[b][j] of the m queries `a` starts at, on their score rows r (an empty gallery has no places)
static int select_places(fern_ctx* c, const RankCall& a, int mq, const ScoreRows& r, long ld, const int32_t* places, int m, int clamp,
                         unsigned long long* keys, hipStream_t s) {
    if (a.N == 0) {
        HIP_TRY(hipMemsetAsync(keys, 0, (size_t)mq * m * sizeof(unsigned long long), s));
        return FERN_OK;
    }
    SelectState* states; unsigned* hist; unsigned long long* found;
    FERN_TRY(ws_get(c, (size_t)9 * mq * SEL_T, &states));
    FERN_TRY(ws_get(c, (size_t)mq * SEL_T * 8 * 256, &hist));
    FERN_TRY(ws_get(c, (size_t)mq * SEL_T, &found));
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)mq * SEL_T * 8 * 256 * sizeof(unsigned), s));      // on the stream: re-run by a replayed graph
    for (int t0 = 0; t0 < m; t0 += SEL_T)
        HIP_TRY(launch_rank_select(r.S, ld, mq, a.N, places + t0, m, std::min(SEL_T, m - t0), clamp, a.exclude, a.idx_offset, states, hist, found,
                                   keys + t0, m, s));
    return FERN_OK;
}
// the deep stage's selection of the chunk under per-query ceilings
static int select_under(const RankCall& a, int mq, const ScoreRows& r, long ld, const unsigned long long* ceil, hipStream_t s) {
    HIP_TRY(launch_deep_select(r.S, ld, a.N, mq, a.K, nullptr, nullptr, nullptr, a.D, a.exclude, a.idx_offset, a.out_scores, a.out_idx, r.flags, r.state, s, ceil));
    if (a.N > 0) HIP_TRY(launch_deep_fallback(r.S, ld, a.N, mq, a.K, a.exclude, a.idx_offset, a.out_scores, a.out_idx, r.flags, r.state, s, ceil));
    return FERN_OK;
}

extern "C" int fern_rank_select(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D,
                                const int32_t* places, int m, int64_t idx_offset, const int32_t* exclude_idx, uint64_t* out_keys,
                                const uint32_t* tags, const uint32_t* mask, const uint32_t* value, void* stream) {
    const PageCall p = page_call("fern_rank_select", q, gallery, gallery_bf16, B, N, D, idx_offset, exclude_idx, tags, mask, value);
    FERN_TRY(page_check(c, p, places && out_keys, m, 0));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, B, p.chunk(), [&](long o, int mq) -> int {
        const RankCall a = p.call.at(o);
        ScoreRows r;
        StageTimer st(c, s);
        FERN_TRY(score_rows(c, a, mq, p.ld(), p.form(), st, s, &r));
        FERN_TRY(select_places(c, a, mq, r, p.ld(), places + o * m, m, 0, reinterpret_cast<unsigned long long*>(out_keys) + o * m, s));
        st.commit(mq, (int)N, D);
        return FERN_OK;
    });
}

extern "C" int fern_sim_topk_from(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D, int K,
                                  const uint64_t* from_keys, float* out_scores, int32_t* out_idx, int64_t idx_offset, const int32_t* exclude_idx,
                                  const uint32_t* tags, const uint32_t* mask, const uint32_t* value, void* stream) {
    const PageCall p = page_call("fern_sim_topk_from", q, gallery, gallery_bf16, B, N, D, idx_offset, exclude_idx, tags, mask, value, K, out_scores, out_idx);
    FERN_TRY(page_check(c, p, from_keys && out_scores && out_idx, K, 1024));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, B, p.chunk(), [&](long o, int mq) -> int {
        const RankCall a = p.call.at(o);
        ScoreRows r;
        StageTimer st(c, s);
        FERN_TRY(score_rows(c, a, mq, p.ld(), p.form(), st, s, &r));
        FERN_TRY(select_under(a, mq, r, p.ld(), reinterpret_cast<const unsigned long long*>(from_keys) + o, s));
        st.commit(mq, (int)N, D);
        return FERN_OK;
    });
}

extern "C" int fern_sim_topk_page(fern_ctx* c, const float* q, const float* gallery, const uint16_t* gallery_bf16, int B, int64_t N, int D, int K,
                                  const int32_t* offsets, float* out_scores, int32_t* out_idx, int64_t idx_offset, const int32_t* exclude_idx,
                                  const uint32_t* tags, const uint32_t* mask, const uint32_t* value, void* stream) {
    const PageCall p = page_call("fern_sim_topk_page", q, gallery, gallery_bf16, B, N, D, idx_offset, exclude_idx, tags, mask, value, K, out_scores, out_idx);
    FERN_TRY(page_check(c, p, offsets && out_scores && out_idx, K, 1024));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, B, p.chunk(), [&](long o, int mq) -> int {
        const RankCall a = p.call.at(o);
        ScoreRows r;
        unsigned long long* ceil;      // the key at place offsets[b]: 0 past the end of the ranking, which makes nothing eligible
        StageTimer st(c, s);
        FERN_TRY(score_rows(c, a, mq, p.ld(), p.form(), st, s, &r));
        FERN_TRY(ws_get(c, (size_t)mq, &ceil));
        FERN_TRY(select_places(c, a, mq, r, p.ld(), offsets + o, 1, 1, ceil, s));
        FERN_TRY(select_under(a, mq, r, p.ld(), ceil, s));
        st.commit(mq, (int)N, D);
        return FERN_OK;
    });
}

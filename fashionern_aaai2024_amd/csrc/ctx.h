// Private header of the C-ABI layer of libfern.so (api_*.hip; include/fern.h has the contract): what two or more of its files share.
// Everything that is not a template or a macro is defined once, in api_ctx.hip unless its line names another file.  Kernel files do
// not include this header; the generic names (fail, ...) live in fern::api so that they cannot meet a kernel file's.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <vector>
#include "../../include/fern.h"
#include "kernels.h"

namespace fern::api {
// ---- errors -------------------------------------------------------------------------------------
int fail(int code, const std::string& msg);      // sets this thread's fern_last_error() text, returns code

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return ::fern::api::fail(e_ == hipErrorInvalidValue ? FERN_ERR_ARG : FERN_ERR_HIP,          \
                        std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
    } while (0)
#define FERN_TRY(expr)              \
    do {                            \
        int r_ = (expr);            \
        if (r_ != FERN_OK) return r_; \
    } while (0)

// ---- weights ------------------------------------------------------------------------------------
struct HostTensor { std::vector<float> f; std::vector<int64_t> shape; };
struct LinearW { const float* w = nullptr; const float* b = nullptr; int out = 0, in = 0; const unsigned short* wb = nullptr; /* bf16 copy of w (encoder blocks) */
                 const unsigned char* w8 = nullptr; const float* sw = nullptr; /* fp8 copy + per-output-channel scales */
                 const unsigned char* wm = nullptr; const unsigned char* swm = nullptr; long swm_rows = 0; /* MX fp8 copy + E8M0 block scales */ };
struct LNW { const float* g = nullptr; const float* b = nullptr; };
struct CombinerW {
    LinearW text, image, hidden;
    const float* w2 = nullptr;
    const float* b2 = nullptr;
    // query-side combiners (DVR.*): their hidden layer runs at M = batch (64) where an unsplit k chain of 4096 leaves 192 CUs
    // idle, so K is cut into 512-wide slices -- for EVERY batch size (kernels.h: GemmParams.ksplit): the split belongs to the
    // module, not to M.  The gallery-side combiner (M = thousands of rows per tile) stays unsplit.
    int ksplit = 1;
};
struct SRW {
    LinearW local, global;
    const float *bn13_mean = nullptr, *bn13_inv = nullptr, *bn13_beta = nullptr;   // per patch
    const float *bnd_scale = nullptr, *bnd_shift = nullptr;                         // per column
    const float *wc = nullptr, *bc = nullptr;
};
struct BertLayerW { LinearW qkv, attn_out, inter, out; LNW ln1, ln2; };
struct Clip4CirW { bool ready = false; int width = 0; LinearW text, image, comb, outl, hidden; const float* w2 = nullptr; const float* b2 = nullptr; };
struct FusionW {
    int parts = 0;      // FERN_PART_* bits that are finalised
    int D = 0;
    const float *cls = nullptr, *pos = nullptr, *type = nullptr;
    LNW emb_ln;
    BertLayerW layer[2];
    LinearW mha_q, mha_kv, mha_out;
    SRW sr[2];          // fern_sr_id
    CombinerW comb[4];  // fern_combiner_id
};
struct ClipBlockW { LNW ln1, ln2; LinearW qkv, out, fc, proj; };
struct ConvW { const float* w = nullptr; const float* b = nullptr; int cout = 0, k = 0; };   // BatchNorm folded; w [cout][k]
struct BottleneckW { ConvW c1, c2, c3, down; bool has_down = false; int stride = 1, cin = 0, planes = 0; };
struct ResNetW {
    ConvW stem1, stem2, stem3;
    int stem_c = 0;              // stem channel count padded to a multiple of 16 (RN50x4: 40 -> 48)
    std::vector<BottleneckW> blocks;
    const float* pos = nullptr;
    LinearW q, kv, cproj;
    const float* zeros = nullptr;
};
struct ClipW {
    bool ready = false;
    ResNetW res;
    fern_clip_config cfg{};
    const float *conv_w = nullptr, *cls = nullptr, *vpos = nullptr, *vproj_t = nullptr;
    const float* conv_wp = nullptr;  // patch sides outside the 16-byte patch loaders (patch % 4 or 3 * patch^2 % 32, e.g. 14): conv1 as [width, conv_kp], zero padded
    int conv_kp = 0;                 // 3 * patch^2 rounded up to 32 (588 -> 608); 0 = the im2col loaders take this patch
    LinearW conv_mx;                 // conv1 as a [width, 3 * patch * patch] linear layer: its block-scaled copy (FERN_PREC_MX8 patch embedding) and its bf16 copy (bf16-operand modes)
    LNW ln_pre, ln_post, ln_final;
    std::vector<ClipBlockW> vblocks, tblocks;
    const float *tok_emb = nullptr, *tpos = nullptr, *tproj_t = nullptr;
    int act = FERN_ACT_GELU;         // MLP activation of BOTH towers (fern_clip_set_activation); lives with the weights: forks read the root's
};

// ---- profiling records --------------------------------------------------------------------------
enum ProfKind { PROF_GEMM = 0, PROF_ATTN = 1, PROF_TOPK = 2, PROF_SWEEP = 3, PROF_STAGE = 4 };
struct ProfRec { hipEvent_t a, b; int kind; double work; int m, n, k, tag; int dispatches;
                 std::vector<hipEvent_t> kev; /* kernel-precise (start, stop) pairs of the launch's dispatches (kernels.h: LaunchTimer); empty: a, b are stream events */
                 /* span records (the ranking stage, round 5): kev holds EVERY dispatch of the stage in launch order; the stage's time is first
                    dispatch begin -> last dispatch end (launch boundaries between them included), the dispatches [sweep_lo, sweep_hi) are its
                    full-gallery sweep(s), `work` their bytes */
                 bool span = false; int sweep_lo = 0, sweep_hi = 0;
                 double extra_flops = 0.0; /* run_gemm_b_pair: the flops of `work` that belong to the second (bf16) problem */
                 double extra_alg_bytes = 0.0; /* a GEMM PAIR record (run_gemm_pair): the second problem's algorithmic bytes (m, n, k are the first's) */ };

}  // namespace fern::api

// ---- context ------------------------------------------------------------------------------------
struct fern_ctx {
    int device = 0;
    std::map<std::string, fern::api::HostTensor> host;
    // device weight buffers, per weight group: re-finalising a group frees its previous generation
    enum { G_CLIP = 0, G_DVR, G_TARGET_SR, G_TARGET_COMBINER, G_CLIP4CIR, G_COUNT };
    std::vector<void*> owned[G_COUNT];
    int cur_group = G_CLIP;          // group the upload helpers currently allocate into
    // forks point into the parent's buffers: `generation` counts the parent's re-finalisations, a fork remembers the value
    // it was created at and every weight-reading entry point refuses to run on a stale fork
    unsigned generation = 0;
    const fern_ctx* parent = nullptr;
    unsigned parent_generation = 0;
    int* tok_flag = nullptr;         // host-mapped: set by the text embedding kernel when a token id is out of range
    int* live_flag = nullptr;        // host-mapped [3]: set by the live-gallery kernels (upsert, move, scatter) when a slot is out of range
    fern::api::FusionW fusion;
    fern::api::ClipW clip;
    fern::api::Clip4CirW c4c;
    int precision = FERN_PREC_FP32;  // operand precision of the CLIP towers' token-level GEMMs (fern_set_precision)
    int rank_strategy = 0;           // fern_rank_set_strategy (FERN_RANK_AUTO)
    bool f32x3 = false;              // FERN_PREC_F32X3: `precision` stays FP32 (same buffers, same code paths), GEMMs run split (run_gemm)
    // workspace arena (bump allocator; blocks are consolidated at the start of the next op)
    struct Block { char* p; size_t cap; };
    std::vector<Block> blocks;
    size_t used = 0;                 // offset into blocks.back()
    // bumped whenever workspace memory handed out earlier is FREED (the consolidation in ws_begin): addresses baked into a
    // captured hipGraph of this context are dead from then on -- fern_ws_generation lets the owner of the graph notice
    unsigned long long ws_generation = 0;
    // profiling
    bool prof_on = false;
    std::vector<fern::api::ProfRec> recs;
    std::vector<hipEvent_t> ev_pool;
    fern::LaunchTimer timer;
};

namespace fern::api {
// ---- workspace arena ----------------------------------------------------------------------------
int ws_begin(fern_ctx* c, hipStream_t s);                   // a fresh frame: everything handed out earlier is free again
int ws_alloc(fern_ctx* c, size_t bytes, void** out);
template <class T>
int ws_get(fern_ctx* c, size_t count, T** out) {
    void* p = nullptr;
    FERN_TRY(ws_alloc(c, count * sizeof(T), &p));
    *out = reinterpret_cast<T*>(p);
    return FERN_OK;
}
// The chunk loop of the entry points that walk a batch: a fresh workspace frame per chunk, body(o, m) for rows o .. o + m.
template <class Body>
int for_query_chunks(fern_ctx* c, hipStream_t s, long B, long chunk, Body body) {
    for (long o = 0; o < B; o += chunk) {
        FERN_TRY(ws_begin(c, s));
        FERN_TRY(body(o, (int)std::min<long>(chunk, B - o)));
    }
    return FERN_OK;
}

// ---- profiling hooks ----------------------------------------------------------------------------
int prof_open(fern_ctx* c, int kind, double work, hipStream_t s, int* slot, int m = 0, int n = 0, int k = 0, int tag = 0);
int prof_close(fern_ctx* c, int slot, hipStream_t s);
void prof_abort(fern_ctx* c, int slot);                     // a launch that failed after prof_open
#define HIP_TRY_PROF(le, c, slot)                               \
    do {                                                        \
        const hipError_t le__ = (le);                           \
        if (le__ != hipSuccess) ::fern::api::prof_abort(c, slot); \
        HIP_TRY(le__);                                          \
    } while (0)

// The ranking stage timed by its dispatches' own timestamps (round 5): while a StageTimer is live every launch of the stage goes through
// FERN_LAUNCH with an event pair; commit() turns them into ONE span record.  A stage that fails (or a stream being captured) leaves
// nothing behind.  [The stream-marker interval of rounds 3-4 charged two marker packets + dispatch latencies, ~8 us, to a stage that is
// now ~46 us of kernels.]
struct StageTimer {
    fern_ctx* c;
    bool on = false, done = false;
    int sweep_lo = 0, sweep_hi = 0;
    double sweep_bytes = 0;
    StageTimer(fern_ctx* ctx, hipStream_t s);
    void sweep_begin() { if (on) sweep_lo = (int)c->timer.events.size() / 2; }
    void sweep_end(double bytes) { if (on) { sweep_hi = (int)c->timer.events.size() / 2; sweep_bytes += bytes; } }
    void commit(int m, int n, int k);
    ~StageTimer();
};

// ---- launch wrappers (one profile record per launch) and the descriptors of a layer's GEMM in each operand form ---------------
int run_gemm(fern_ctx* c, const GemmParams& p, hipStream_t s, int kind = PROF_GEMM, double work = -1.0);
int run_gemm_pair(fern_ctx* c, const GemmParams& p1, const GemmParams& p2, hipStream_t s);
int run_gemm_b(fern_ctx* c, const GemmParams& p, hipStream_t s);
int run_gemm_b_pair(fern_ctx* c, const GemmParams& p1, const GemmParams& p2, hipStream_t s);
int run_attention(fern_ctx* c, const AttnParams& a, hipStream_t s);
int run_pooled_attention(fern_ctx* c, const PooledAttnParams& p, hipStream_t s);      // qt / u come from the arena
GemmParams gemm_desc(const float* A, long lda, const LinearW& L, float* C, long ldc, int M, int epi);
GemmParams gemm_desc_b(const unsigned short* A, long lda, const LinearW& L, void* C, long ldc, int M, int epi, bool out_bf16);
GemmParams gemm_desc_f8(const unsigned char* A8, const float* sa, long lda, const LinearW& L, void* C, long ldc, int M, int epi, bool out_bf16);
GemmParams gemm_desc_mx(const unsigned char* A8, const unsigned char* sa, long srows, long lda, const LinearW& L, void* C, long ldc, int M, int epi, bool out_bf16);
int clip_mlp_epi(const fern_ctx* c);      // c_fc epilogue of the CLIP towers' MLPs
// the ModifiedResNet's convolutions over NHWC pixel rows (api_towers.hip): a 1x1 as a plain GEMM, a 3x3 / stride 1 / pad 1 through the window loader
GemmParams conv_desc(const float* A, const ConvW& W, float* C, int M, int epi);
GemmParams conv3x3_desc(const float* A, const ConvW& W, float* C, int b, int H, int Wd, int cin, const float* zeros);

// ---- checks that entry points of several files make ---------------------------------------------
int check_fresh(fern_ctx* c, const char* fn);            // weight-reading entry points: a fork made before the parent's last re-finalisation must not run
int check_token_flag(fern_ctx* c, const char* fn);       // api_towers.hip
int check_live_flags(fern_ctx* c, const char* fn);       // api.hip

}  // namespace fern::api

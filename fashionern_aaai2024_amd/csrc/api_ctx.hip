// C-ABI layer of libfern.so (include/fern.h has the contract), the part every other api_*.hip file stands on (ctx.h): errors, context lifetime,
// the workspace arena, the profiling hooks and fern_prof_*, the launch wrappers, the precision / activation switches, the tuner pass-throughs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ctx.h"

using namespace fern;
using namespace fern::api;

// ---- errors ---------------------------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;
int fern::api::fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
extern "C" int fern_abi_version(void) { return FERN_ABI_VERSION; }
extern "C" const char* fern_last_error(void) { return g_last_error.c_str(); }

// ---- the launch timer (kernels.h: LaunchTimer, FERN_LAUNCH) ---------------------------------------------------------------------
namespace fern {
thread_local LaunchTimer* g_launch_timer = nullptr;
hipEvent_t launch_timer_event() {
    LaunchTimer* t = g_launch_timer;
    hipEvent_t e = nullptr;
    if (t && t->pool && !t->pool->empty()) { e = t->pool->back(); t->pool->pop_back(); }
    else (void)hipEventCreate(&e);
    return e;
}
}  // namespace fern

// armed: the launches that follow on this thread go through hipExtLaunchKernelGGL with an event pair each (kernels.h: FERN_LAUNCH)
static void timer_arm(fern_ctx* c) { c->timer.events.clear(); c->timer.pool = &c->ev_pool; g_launch_timer = &c->timer; }
// events that are done with go back to the context's pool; timer_drop: disarmed, the events of the dispatches that went out handed back
static void recycle(fern_ctx* c, std::vector<hipEvent_t>& ev) { c->ev_pool.insert(c->ev_pool.end(), ev.begin(), ev.end()); ev.clear(); }
static void timer_drop(fern_ctx* c) { g_launch_timer = nullptr; recycle(c, c->timer.events); }

// ---- context lifetime -----------------------------------------------------------------------------------------------------------
extern "C" int fern_ctx_create(int device, fern_ctx** out) {
    if (!out) return fail(FERN_ERR_ARG, "fern_ctx_create: out is NULL");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(FERN_ERR_ARG, "fern_ctx_create: no such device " + std::to_string(device));
    HIP_TRY(hipSetDevice(device));
    auto* c = new fern_ctx();
    c->device = device;
    *out = c;
    return FERN_OK;
}
// A fork shares the parent's finalised device weights (read-only) but has its own workspace, tuner-independent launch
// state and profiling records, so several forks can run concurrently on different HIP streams of the same device.
extern "C" int fern_ctx_fork(fern_ctx* parent, fern_ctx** out) {
    if (!parent || !out) return fail(FERN_ERR_ARG, "fern_ctx_fork: NULL argument");
    auto* c = new fern_ctx();
    c->device = parent->device;
    if (parent->parent) return fail(FERN_ERR_ARG, "fern_ctx_fork: fork the root context, not a fork");
    c->parent = parent;
    c->parent_generation = parent->generation;
    c->fusion = parent->fusion;      // pointers into the parent's `owned` buffers; the parent must outlive its forks
    c->clip = parent->clip;
    c->c4c = parent->c4c;
    c->precision = parent->precision;
    c->rank_strategy = parent->rank_strategy;
    c->f32x3 = parent->f32x3;
    *out = c;
    return FERN_OK;
}

extern "C" int fern_ctx_destroy(fern_ctx* c) {
    if (!c) return FERN_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (auto& grp : c->owned)
        for (void* p : grp) (void)hipFree(p);
    if (c->tok_flag) (void)hipHostFree(c->tok_flag);
    if (c->live_flag) (void)hipHostFree(c->live_flag);
    for (auto& b : c->blocks) (void)hipFree(b.p);
    for (auto& r : c->recs) {
        if (r.a) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        for (hipEvent_t e : r.kev) (void)hipEventDestroy(e);
    }
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    delete c;
    return FERN_OK;
}
extern "C" int fern_sync(fern_ctx* c, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_sync: ctx is NULL");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    FERN_TRY(check_token_flag(c, "fern_sync"));
    return check_live_flags(c, "fern_sync");
}
int fern::api::check_fresh(fern_ctx* c, const char* fn) {
    if (c->parent && c->parent->generation != c->parent_generation)
        return fail(FERN_ERR_STATE, std::string(fn) + ": this fork predates the parent's last fern_finalize_*: its weight pointers are stale "
                                                       "(fork again after loading weights)");
    return FERN_OK;
}

// ---- workspace arena ------------------------------------------------------------------------------------------------------------
int fern::api::ws_begin(fern_ctx* c, hipStream_t s) {
    if (c->blocks.size() > 1) {      // grew during the previous op: merge into one block (outside capture only)
        size_t total = 0;
        for (auto& b : c->blocks) total += b.cap;
        HIP_TRY(hipStreamSynchronize(s));
        for (auto& b : c->blocks) HIP_TRY(hipFree(b.p));
        c->blocks.clear();
        ++c->ws_generation;
        char* p = nullptr;
        HIP_TRY(hipMalloc(&p, total));
        c->blocks.push_back({p, total});
    }
    c->used = 0;
    return FERN_OK;
}
int fern::api::ws_alloc(fern_ctx* c, size_t bytes, void** out) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (c->blocks.empty() || c->used + bytes > c->blocks.back().cap) {
        size_t cap = bytes;
        if (!c->blocks.empty()) cap = std::max(bytes, c->blocks.back().cap);   // geometric growth
        cap = std::max(cap, (size_t)64 << 20);
        char* p = nullptr;
        HIP_TRY(hipMalloc(&p, cap));
        c->blocks.push_back({p, cap});
        c->used = 0;
    }
    *out = c->blocks.back().p + c->used;
    c->used += bytes;
    return FERN_OK;
}
extern "C" uint64_t fern_ws_generation(const fern_ctx* c) { return c ? c->ws_generation : 0; }

// ---- profiling hooks ------------------------------------------------------------------------------------------------------------
// GEMM and attention launches (kinds whose roofline is a per-KERNEL figure): timed by the dispatches' own timestamps
// (the sweep kernel of the ranking stage too; the STAGE around it -- sample pass, bound, sweep, select, exact gate, launch boundaries
// included -- is ONE stream-marker interval, PROF_STAGE)
static bool prof_kernel_precise(int kind) { return kind == PROF_GEMM || kind == PROF_ATTN || kind == PROF_SWEEP; }
int fern::api::prof_open(fern_ctx* c, int kind, double work, hipStream_t s, int* slot, int m, int n, int k, int tag) {
    *slot = -1;
    if (!c->prof_on) return FERN_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (prof_kernel_precise(kind) && hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) {
        c->recs.push_back({nullptr, nullptr, kind, work, m, n, k, tag, 1, {}});
        *slot = (int)c->recs.size() - 1;
        timer_arm(c);
        return FERN_OK;
    }
    hipEvent_t ev[2];
    for (int i = 0; i < 2; ++i) {
        if (!c->ev_pool.empty()) { ev[i] = c->ev_pool.back(); c->ev_pool.pop_back(); }
        else HIP_TRY(hipEventCreate(&ev[i]));
    }
    HIP_TRY(hipEventRecord(ev[0], s));
    c->recs.push_back({ev[0], ev[1], kind, work, m, n, k, tag, 1, {}});
    *slot = (int)c->recs.size() - 1;
    return FERN_OK;
}
int fern::api::prof_close(fern_ctx* c, int slot, hipStream_t s) {
    if (slot < 0) return FERN_OK;
    if (!c->recs[slot].a) {              // kernel-precise record: collect the event pairs of its dispatches, disarm
        g_launch_timer = nullptr;
        c->recs[slot].kev.swap(c->timer.events);
        return FERN_OK;
    }
    HIP_TRY(hipEventRecord(c->recs[slot].b, s));
    return FERN_OK;
}

// A launch that failed after prof_open: disarm the timer, hand the events of the dispatches that did go out back to the pool and
// drop the record -- left in place it would count as a 0 ms launch carrying its full flops.  Records are appended and
// closed in order on one thread, so an open record is always the last one.
void fern::api::prof_abort(fern_ctx* c, int slot) {
    timer_drop(c);
    if (slot < 0 || slot != (int)c->recs.size() - 1) return;
    ProfRec& r = c->recs[slot];
    if (r.a) c->ev_pool.push_back(r.a);
    if (r.b) c->ev_pool.push_back(r.b);
    c->recs.pop_back();
}

StageTimer::StageTimer(fern_ctx* ctx, hipStream_t s) : c(ctx) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (c->prof_on && hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) {
        timer_arm(c);
        on = true;
    }
}
void StageTimer::commit(int m, int n, int k) {
    if (!on) return;
    g_launch_timer = nullptr;
    done = true;
    if (c->timer.events.size() < 2) return;
    ProfRec r{nullptr, nullptr, PROF_STAGE, sweep_bytes, m, n, k, 0, 1, {}};
    r.span = true; r.sweep_lo = sweep_lo; r.sweep_hi = sweep_hi;
    r.kev.swap(c->timer.events);
    c->recs.push_back(std::move(r));
}
StageTimer::~StageTimer() {
    if (on && !done) timer_drop(c);
}

extern "C" int fern_prof_enable(fern_ctx* c, int on) {
    if (!c) return fail(FERN_ERR_ARG, "fern_prof_enable: ctx is NULL");
    c->prof_on = on != 0;
    return FERN_OK;
}
extern "C" int fern_prof_collect(fern_ctx* c, fern_prof_stats* out) {
    if (!c || !out) return fail(FERN_ERR_ARG, "fern_prof_collect: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    std::memset(out, 0, sizeof(*out));
    // FERN_PROF_DUMP=<path>: append one CSV line per instrumented launch (kind,m,n,k,tag,ms,work) for shape-level analysis
    double stage_ms = 0.0;
    const char* dump_path = std::getenv("FERN_PROF_DUMP");
    FILE* dump = dump_path ? std::fopen(dump_path, "a") : nullptr;
    for (auto& r : c->recs) {
        float ms = 0.f;
        if (r.span) {                    // the ranking stage: first dispatch begin -> last dispatch end; its sweep dispatches on their own
            HIP_TRY(hipEventElapsedTime(&ms, r.kev.front(), r.kev.back()));
            for (int i = r.sweep_lo; i < r.sweep_hi; ++i) {
                float one = 0.f;
                HIP_TRY(hipEventElapsedTime(&one, r.kev[2 * i], r.kev[2 * i + 1]));
                out->sweep_ms += one;
                out->sweep_launches++;
            }
            out->sweep_bytes += r.work;
            recycle(c, r.kev);
        } else if (!r.a) {               // kernel-precise: the sum of the dispatches' own durations
            for (size_t i = 0; i + 1 < r.kev.size(); i += 2) {
                float one = 0.f;
                HIP_TRY(hipEventElapsedTime(&one, r.kev[i], r.kev[i + 1]));
                ms += one;
            }
            recycle(c, r.kev);
        } else
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        if (dump) std::fprintf(dump, "%d,%d,%d,%d,%d,%.6f,%.0f\n", r.kind, r.m, r.n, r.k, r.tag, ms, r.work);
        switch (r.kind) {
            case PROF_GEMM:
                if (r.tag >= 300) { out->gemm_mx8_ms += ms; out->gemm_mx8_flops += r.work; out->gemm_mx8_launches++; out->gemm_mx8_bf16_flops += r.extra_flops; }
                else if (r.tag >= 200) { out->gemm_fp8_ms += ms; out->gemm_fp8_flops += r.work; out->gemm_fp8_launches++; }
                else if (r.tag >= 100) { out->gemm_bf16_ms += ms; out->gemm_bf16_flops += r.work; out->gemm_bf16_launches++; }
                else { out->gemm_ms += ms; out->gemm_flops += r.work; out->gemm_launches++;
                       out->gemm_alg_bytes += 4.0 * ((double)r.m * r.k + (double)r.n * r.k + (double)r.m * r.n) + r.extra_alg_bytes;
                       out->gemm_dispatches += r.dispatches; }
                break;
            case PROF_ATTN: out->attn_ms += ms; out->attn_flops += r.work; out->attn_launches++; break;
            case PROF_TOPK: out->topk_ms += ms; out->topk_launches++; break;
            case PROF_STAGE: stage_ms += ms; out->topk_launches++; break;      // whole ranking stage of a query chunk (a span record, or one marker pair)
            default: out->sweep_ms += ms; out->sweep_bytes += r.work; out->sweep_launches++; break;
        }
        if (r.a) { c->ev_pool.push_back(r.a); c->ev_pool.push_back(r.b); }
    }
    c->recs.clear();
    // topk_ms = the rest of the ranking stage = (stage intervals, launch boundaries included) - (the sweep kernels' own durations)
    if (stage_ms > 0.0) out->topk_ms += stage_ms > out->sweep_ms ? stage_ms - out->sweep_ms : 0.0;
    if (dump) std::fclose(dump);
    return FERN_OK;
}

// ---- launch wrappers: one profile record per launch -----------------------------------------------------------------------------
int fern::api::run_gemm(fern_ctx* c, const GemmParams& p, hipStream_t s, int kind, double work) {
    int slot;
    FERN_TRY(prof_open(c, kind, work >= 0 ? work : 2.0 * p.M * (double)p.N * p.K, s, &slot, p.M, p.N, p.K, p.epi));
    hipError_t le;
    if (c->f32x3 && kind == PROF_GEMM && p.w_sample <= 1) {      // FERN_PREC_F32X3: never the ranking stage (PROF_SWEEP / sample pass)
        GemmParams q = p;
        q.split = 3;                                             // launch_gemm falls back to the fp32 kernels where the split family does not apply
        le = launch_gemm(q, s);
    } else {
        le = launch_gemm(p, s);
    }
    HIP_TRY_PROF(le, c, slot);                                   // (a failed launch must not leave the timer armed, nor a 0 ms record behind)
    if (slot >= 0) c->recs[slot].dispatches = gemm_last_dispatches();
    return prof_close(c, slot, s);
}
// Two plain GEMMs of the fp32 data flow in ONE launch where the family can (gemm.hip: launch_gemm_pair; two launches otherwise): the
// image tower's GEMM of a layer and the text tower's GEMM of the same kind.  One profile record for both (shape = the first's, the
// flops of both): the launch is what the roofline prices.
int fern::api::run_gemm_pair(fern_ctx* c, const GemmParams& p1, const GemmParams& p2, hipStream_t s) {
    int slot;
    FERN_TRY(prof_open(c, PROF_GEMM, 2.0 * p1.M * (double)p1.N * p1.K + 2.0 * p2.M * (double)p2.N * p2.K, s, &slot, p1.M, p1.N, p1.K, 50 + p1.epi));
    GemmParams a = p1, b = p2;
    if (c->f32x3) { a.split = 3; b.split = 3; }
    const hipError_t le = launch_gemm_pair(a, b, s);
    HIP_TRY_PROF(le, c, slot);
    if (slot >= 0) {
        c->recs[slot].dispatches = gemm_last_dispatches();
        c->recs[slot].extra_alg_bytes = 4.0 * ((double)p2.M * p2.K + (double)p2.N * p2.K + (double)p2.M * p2.N);
    }
    return prof_close(c, slot, s);
}
GemmParams fern::api::gemm_desc(const float* A, long lda, const LinearW& L, float* C, long ldc, int M, int epi) {
    GemmParams p{};
    p.A = A; p.lda = lda; p.W = L.w; p.ldw = L.in; p.bias = L.b; p.C = C; p.ldc = ldc;
    p.M = M; p.N = L.out; p.K = L.in; p.epi = epi; p.aload = ALOAD_PLAIN;
    return p;
}
// bf16-operand GEMM of the encoder "perf mode": A is a bf16 activation buffer, the weight is the layer's bf16 copy
GemmParams fern::api::gemm_desc_b(const unsigned short* A, long lda, const LinearW& L, void* C, long ldc, int M, int epi, bool out_bf16) {
    GemmParams p{};
    p.Ab = A; p.lda = lda; p.Wb = L.wb; p.ldw = L.in; p.bias = L.b; p.C = reinterpret_cast<float*>(C); p.ldc = ldc;
    p.M = M; p.N = L.out; p.K = L.in; p.epi = epi; p.aload = ALOAD_PLAIN; p.out_bf16 = out_bf16 ? 1 : 0;
    return p;
}
// fp8-operand GEMM: A8 [M, K] e4m3fn with per-row scales sa, the layer's fp8 weight copy with per-channel scales
GemmParams fern::api::gemm_desc_f8(const unsigned char* A8, const float* sa, long lda, const LinearW& L, void* C, long ldc, int M, int epi,
                                   bool out_bf16) {
    GemmParams p = gemm_desc_b(reinterpret_cast<const unsigned short*>(A8), lda, L, C, ldc, M, epi, out_bf16);
    p.Wb = reinterpret_cast<const unsigned short*>(L.w8); p.fp8 = 1; p.scale_a = sa; p.scale_w = L.sw;
    return p;
}
// block-scaled (MX) fp8 GEMM: A8 [M, K] e4m3fn with E8M0 block scales sa (srows rows), the layer's MX weight copy
GemmParams fern::api::gemm_desc_mx(const unsigned char* A8, const unsigned char* sa, long srows, long lda, const LinearW& L, void* C, long ldc, int M,
                                   int epi, bool out_bf16) {
    GemmParams p = gemm_desc_b(reinterpret_cast<const unsigned short*>(A8), lda, L, C, ldc, M, epi, out_bf16);
    p.Wb = reinterpret_cast<const unsigned short*>(L.wm); p.fp8 = 2; p.mxa = sa; p.mxa_rows = srows; p.mxw = L.swm; p.mxw_rows = L.swm_rows;
    return p;
}
int fern::api::run_gemm_b(fern_ctx* c, const GemmParams& p, hipStream_t s) {
    int slot;
    FERN_TRY(prof_open(c, PROF_GEMM, 2.0 * p.M * (double)p.N * p.K, s, &slot, p.M, p.N, p.K, (p.fp8 == 2 ? 300 : p.fp8 ? 200 : 100) + p.epi));
    const hipError_t le = launch_gemm_bf16(p, s);
    HIP_TRY_PROF(le, c, slot);
    return prof_close(c, slot, s);
}
// The image tower's block-scaled GEMM of a layer and the text tower's bf16 GEMM of the same kind in ONE launch where that wins
// (gemm_bf16.hip: launch_gemm_mxbf_pair; two launches otherwise).  One profile record, as run_gemm_pair.
int fern::api::run_gemm_b_pair(fern_ctx* c, const GemmParams& p1, const GemmParams& p2, hipStream_t s) {
    int slot;
    FERN_TRY(prof_open(c, PROF_GEMM, 2.0 * p1.M * (double)p1.N * p1.K + 2.0 * p2.M * (double)p2.N * p2.K, s, &slot, p1.M, p1.N, p1.K, 350 + p1.epi));
    const hipError_t le = launch_gemm_mxbf_pair(p1, p2, s);
    HIP_TRY_PROF(le, c, slot);
    if (slot >= 0) {
        c->recs[slot].dispatches = gemm_last_dispatches();
        c->recs[slot].extra_flops = 2.0 * p2.M * (double)p2.N * p2.K;
    }
    return prof_close(c, slot, s);
}
int fern::api::run_attention(fern_ctx* c, const AttnParams& a, hipStream_t s) {
    int slot;
    FERN_TRY(prof_open(c, PROF_ATTN, 4.0 * a.batch * a.heads * (double)a.s_q * a.s_k * a.hd, s, &slot, a.batch * a.heads, a.s_q, a.hd, a.causal));
    const hipError_t le = launch_attention(a, s);
    HIP_TRY_PROF(le, c, slot);
    return prof_close(c, slot, s);
}
// The pooled single-query attention (attn.hip): its two [batch, heads, E] scratch rows come from the arena, its three dispatches are ONE
// attention record priced at the flops they do: the fold and the value projection (2 b E^2 each), the scores and the weighted token
// sum (2 b heads S E each).  p.qt / p.u are filled in here.
int fern::api::run_pooled_attention(fern_ctx* c, const PooledAttnParams& p, hipStream_t s) {
    PooledAttnParams a = p;
    const double E = (double)a.heads * a.hd;
    if (a.batch <= 0 || a.heads <= 0 || a.hd <= 0) return fail(FERN_ERR_ARG, "pooled attention: bad shape");
    FERN_TRY(ws_get(c, (size_t)a.batch * a.heads * (size_t)E, &a.qt));
    FERN_TRY(ws_get(c, (size_t)a.batch * a.heads * (size_t)E, &a.u));
    int slot;
    FERN_TRY(prof_open(c, PROF_ATTN, 4.0 * a.batch * E * E + 4.0 * a.batch * a.heads * (double)a.S * E, s, &slot, a.batch * a.heads, 1, (int)E, 2));
    const hipError_t le = launch_pooled_attention(a, s);
    HIP_TRY_PROF(le, c, slot);
    return prof_close(c, slot, s);
}

// ---- precision and activation of the CLIP towers --------------------------------------------------------------------------------
extern "C" int fern_set_precision(fern_ctx* c, int precision) {
    if (!c) return fail(FERN_ERR_ARG, "fern_set_precision: ctx is NULL");
    if (precision != FERN_PREC_FP32 && precision != FERN_PREC_BF16 && precision != FERN_PREC_FP8 && precision != FERN_PREC_MX8 &&
        precision != FERN_PREC_F32X3 && precision != FERN_PREC_MX8_MLP && precision != FERN_PREC_MX8_IMG)
        return fail(FERN_ERR_ARG, "fern_set_precision: unknown precision");
    const bool split = precision == FERN_PREC_F32X3;
    if (split) precision = FERN_PREC_FP32;         // fp32 data flow; only the GEMM arithmetic changes
    auto every_layer_has = [&](const unsigned char* LinearW::*copy) {      // the quantised copy of every layer of both towers
        for (const auto* blocks : {&c->clip.vblocks, &c->clip.tblocks})
            for (const auto& b : *blocks)
                if (!(b.qkv.*copy) || !(b.out.*copy) || !(b.fc.*copy) || !(b.proj.*copy)) return false;
        return true;
    };
    if ((precision == FERN_PREC_MX8 || precision == FERN_PREC_MX8_MLP || precision == FERN_PREC_MX8_IMG) && c->clip.ready && !every_layer_has(&LinearW::wm))
        return fail(FERN_ERR_ARG, "fern_set_precision: mx8 needs tower widths and MLP widths that are multiples of 128 (<= 4096)");
    if (precision == FERN_PREC_FP8 && c->clip.ready && !every_layer_has(&LinearW::w8))
        return fail(FERN_ERR_ARG, "fern_set_precision: fp8 needs tower widths and MLP widths that are multiples of 64 (<= 4096)");
    c->precision = precision;                      // both fields are committed together, after every check has passed
    c->f32x3 = split;
    return FERN_OK;
}
extern "C" int fern_get_precision(fern_ctx* c) { return !c ? FERN_ERR_ARG : c->f32x3 ? FERN_PREC_F32X3 : c->precision; }
// The MLP activation of the CLIP towers (open_clip's quick_gelu / force_quick_gelu, HF's hidden_act): a property of the weights, so it
// is set on the context that owns them and its forks follow it (clip_mlp_epi reads the root's value at every launch).
extern "C" int fern_clip_set_activation(fern_ctx* c, int act) {
    if (!c) return fail(FERN_ERR_ARG, "fern_clip_set_activation: ctx is NULL");
    if (act != FERN_ACT_GELU && act != FERN_ACT_QUICK_GELU)
        return fail(FERN_ERR_ARG, "fern_clip_set_activation: unknown activation " + std::to_string(act) + " (FERN_ACT_GELU = 0, FERN_ACT_QUICK_GELU = 1)");
    if (c->parent) return fail(FERN_ERR_ARG, "fern_clip_set_activation: set it on the root context, its forks follow");
    c->clip.act = act;
    return FERN_OK;
}
// c_fc epilogue of the CLIP towers' MLPs, every walker and precision mode (the fusion BERT keeps exact-erf GELU)
int fern::api::clip_mlp_epi(const fern_ctx* c) {
    const fern_ctx* root = c->parent ? c->parent : c;
    return root->clip.act == FERN_ACT_QUICK_GELU ? EPI_BIAS_QUICKGELU : EPI_BIAS_GELU;
}

// ---- the GEMM tuners' choices (gemm_tuner.hip): process-wide, every context shares them -----------------------------------------
// The choices as text, one line per choice (gemm_tuner.hip has the fields):
//   "f32 M N K epilogue loader cfg rows_a cfg_b" / "f32x3 M N K epilogue cfg rows_a cfg_b"      a shape's tile plan, fp32 / f32x3 family
//   "bf16 | fp8 | mx8 M N K epilogue outflags cfg"                                               a shape's tile, reduced-precision families
//   "pair <fp32 shape> <fp32 shape> one" / "pairb <mx8 shape> <bf16 shape> choice"               one launch or two for a pair of shapes
// Returns the number of bytes the full text needs (excluding the terminator); writes at most cap - 1 bytes + NUL.  A file of these
// lines, named by FERN_GEMM_TILES, pins the choices.
extern "C" int64_t fern_tuner_export(char* buf, int64_t cap) {
    std::string text;
    gemm_tuner_export(text);
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>(text.size(), (size_t)cap - 1);
        std::memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return (int64_t)text.size();
}

// The reverse of fern_tuner_export: `text` (NUL-terminated lines of the export format) replaces this process's choices for the
// shapes it lists -- e.g. rank 0's export broadcast to every rank, so that all ranks of a job run identical kernels.  Unknown or
// inapplicable lines are skipped.  Every configuration is bit-identical, so this never changes a result.
extern "C" int fern_tuner_import(const char* text) {
    if (!text) return fail(FERN_ERR_ARG, "fern_tuner_import: text is NULL");
    gemm_tuner_import(text);
    return FERN_OK;
}

// How many batches the caller keeps in flight on separate streams (process-wide, like the tile choices themselves): the
// reduced-precision GEMM families then score a trial by duration x (share of the chip it fills)^0.75 instead of duration alone.
// Set before the first launch of a shape; shapes already tuned keep their choice.  Never changes a result.
extern "C" int fern_tuner_set_concurrency(int lanes) {
    if (lanes < 1) return fail(FERN_ERR_ARG, "fern_tuner_set_concurrency: lanes must be >= 1");
    gemm_tuner_set_concurrency(lanes);
    return FERN_OK;
}

// Force ONE tile configuration of a GEMM family, process-wide, until released (cfg < 0): what FERN_GEMM_CFG / FERN_GEMM_SPLIT_CFG /
// FERN_GEMM_BF16_CFG / FERN_GEMM_FP8_CFG / FERN_GEMM_MX8_CFG do from the environment, switchable at run time so that a test process can walk
// every variant.  A configuration that cannot serve a call (k tile does not divide K, ...) falls back to the family's own choice.
extern "C" int fern_tuner_force_config(const char* family, int cfg) {
    if (family && gemm_force_cfg(family, cfg)) return FERN_OK;
    return fail(FERN_ERR_ARG, "fern_tuner_force_config: family is one of f32, f32x3, bf16, fp8, mx8");
}

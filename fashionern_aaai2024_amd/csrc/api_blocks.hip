// C-ABI layer of libfern.so: the entry points that are one kernel launch behind an argument check -- the image side's resampling
// passes and the public building blocks (GEMMs, LayerNorm, attention, the quantisers, the fused producers of the towers' operands).
#include "ctx.h"

using namespace fern;
using namespace fern::api;

// ---- image side: PIL-exact 8-bit resampling + ToTensor/Normalize ---------------------------------------------------------------
extern "C" int fern_resample_u8_horizontal(fern_ctx* c, const uint8_t* src, int64_t src_ld, int x0, int y0, int rows, uint8_t* dst, int ow,
                                           const int32_t* bounds, const int32_t* coeffs, int ksize, void* stream) {
    if (!c || !src || !dst || !bounds || !coeffs || rows < 0 || ow < 0 || ksize < 1) return fail(FERN_ERR_ARG, "fern_resample_u8_horizontal: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_resample_h(src, src_ld, x0, y0, rows, dst, ow, bounds, coeffs, ksize, (hipStream_t)stream));
    return FERN_OK;
}
extern "C" int fern_resample_u8_vertical(fern_ctx* c, const uint8_t* src, int64_t src_ld, int x0, int y0, int cols, uint8_t* dst, int oh,
                                         const int32_t* bounds, const int32_t* coeffs, int ksize, void* stream) {
    if (!c || !src || !dst || !bounds || !coeffs || cols < 0 || oh < 0 || ksize < 1) return fail(FERN_ERR_ARG, "fern_resample_u8_vertical: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_resample_v(src, src_ld, x0, y0, cols, dst, oh, bounds, coeffs, ksize, (hipStream_t)stream));
    return FERN_OK;
}
extern "C" int fern_u8_to_normalized_chw(fern_ctx* c, const uint8_t* src, int64_t src_ld, int x0, int y0, int64_t src_image_stride, float* dst,
                                         int n, int oh, int ow, const float* host_mean, const float* host_std, void* stream) {
    if (!c || !src || !dst || !host_mean || !host_std || n < 0 || oh < 0 || ow < 0) return fail(FERN_ERR_ARG, "fern_u8_to_normalized_chw: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_u8_to_chw(src, src_ld, x0, y0, dst, n, src_image_stride, oh, ow, host_mean, host_std, (hipStream_t)stream));
    return FERN_OK;
}

// ---- building blocks ------------------------------------------------------------------------------------------------------------
// fern_epilogue -> GemmEpi: the first four values coincide, FERN_EPI_BIAS_QUICKGELU has its own (kernels.h)
static bool public_epi_ok(int e) { return (e >= FERN_EPI_BIAS && e <= FERN_EPI_BIAS_RESIDUAL) || e == FERN_EPI_BIAS_QUICKGELU; }
static int gemm_epi_of(int e) { return e == FERN_EPI_BIAS_QUICKGELU ? (int)EPI_BIAS_QUICKGELU : e; }

// Common head of the five GEMM entries: what they refuse, in the order they refuse it, then the device; GemmFacts is what differs between the
// families.  Nothing is dereferenced.  GEMM_EMPTY: M == 0 || N == 0, found before any pointer is looked at -- the entry returns FERN_OK without a launch.
enum { GEMM_EMPTY = 1 };
struct GemmFacts {
    const char* fn;
    bool scales_ok;                                               // the family's scale pointers are all given
    bool relu_ok, residual_ok; const char* epi_text;              // epilogues beside BIAS, BIAS_GELU, BIAS_QUICKGELU; the refusal of every other
    bool residual_fp32; const char* residual_text;                // the residual epilogue needs fp32 output; its refusal
    int k_mult, ld_mult; bool rows_ok; const char* mult_text;     // K % k_mult, lda and ldw % ld_mult, the family's own (scale rows, N, ldc)
};
static const char* const kEpiList = "epilogue must be BIAS, BIAS_GELU, BIAS_QUICKGELU or BIAS_RESIDUAL";
static int gemm_begin(fern_ctx* c, const GemmFacts& f, const void* A, int64_t lda, const void* W, int64_t ldw, const void* residual, const void* C,
                      int64_t ldc, int M, int N, int K, int epilogue, int out_bf16) {
    const std::string fn = std::string(f.fn) + ": ";
    if (!c || M < 0 || N < 0 || K <= 0) return fail(FERN_ERR_ARG, fn + "bad argument");
    if (M == 0 || N == 0) return GEMM_EMPTY;
    if (!A || !W || !C || !f.scales_ok) return fail(FERN_ERR_ARG, fn + "NULL argument");
    if (!public_epi_ok(epilogue) || (epilogue == FERN_EPI_BIAS_RELU && !f.relu_ok) || (epilogue == FERN_EPI_BIAS_RESIDUAL && !f.residual_ok))
        return fail(FERN_ERR_ARG, fn + f.epi_text);
    if (epilogue == FERN_EPI_BIAS_RESIDUAL && (!residual || (f.residual_fp32 && out_bf16))) return fail(FERN_ERR_ARG, fn + f.residual_text);
    if (K % f.k_mult || lda % f.ld_mult || ldw % f.ld_mult || !f.rows_ok) return fail(FERN_ERR_ARG, fn + f.mult_text);
    if (lda < K || ldw < K || ldc < N) return fail(FERN_ERR_ARG, fn + "need lda >= K, ldw >= K, ldc >= N (rows must not overlap)");
    HIP_TRY(hipSetDevice(c->device));
    return FERN_OK;
}
// The operand and output fields that the five fill alike.  reduced: A and W are bf16 or fp8 operands (GemmParams.Ab / Wb).
static GemmParams gemm_entry_desc(bool reduced, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* residual,
                                  void* C, int64_t ldc, int M, int N, int K, int epilogue, int out_bf16) {
    GemmParams p{};
    if (reduced) { p.Ab = static_cast<const unsigned short*>(A); p.Wb = static_cast<const unsigned short*>(W); }
    else { p.A = static_cast<const float*>(A); p.W = static_cast<const float*>(W); }
    p.lda = lda; p.ldw = ldw; p.bias = bias; p.R = residual; p.C = static_cast<float*>(C); p.ldc = ldc;
    p.M = M; p.N = N; p.K = K; p.epi = gemm_epi_of(epilogue); p.aload = ALOAD_PLAIN; p.out_bf16 = out_bf16 ? 1 : 0;
    return p;
}

extern "C" int fern_gemm(fern_ctx* c, const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, const float* residual,
                         float* C, int64_t ldc, int M, int N, int K, int epilogue, void* stream) {
    const GemmFacts f{"fern_gemm", /*scales_ok*/ true, /*relu_ok*/ true, /*residual_ok*/ true, "unknown epilogue", /*residual_fp32*/ false, "residual is NULL",
                      /*k_mult*/ 32, /*ld_mult*/ 1, /*rows_ok*/ true, "K must be a multiple of 32"};
    if (const int r = gemm_begin(c, f, A, lda, W, ldw, residual, C, ldc, M, N, K, epilogue, 0)) return r == GEMM_EMPTY ? FERN_OK : r;
    return run_gemm(c, gemm_entry_desc(false, A, lda, W, ldw, bias, residual, C, ldc, M, N, K, epilogue, 0), (hipStream_t)stream);
}

extern "C" int fern_gemm_bf16(fern_ctx* c, const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, const float* bias,
                              const float* residual, void* C, int64_t ldc, int M, int N, int K, int epilogue, int out_bf16, void* stream) {
    const GemmFacts f{"fern_gemm_bf16", /*scales_ok*/ true, /*relu_ok*/ true, /*residual_ok*/ true, "unknown epilogue", /*residual_fp32*/ true,
                      "the residual epilogue needs a residual and fp32 output", /*k_mult*/ 32, /*ld_mult*/ 8, /*rows_ok*/ true, "K % 32, lda % 8 and ldw % 8 must be 0"};
    if (const int r = gemm_begin(c, f, A, lda, W, ldw, residual, C, ldc, M, N, K, epilogue, out_bf16)) return r == GEMM_EMPTY ? FERN_OK : r;
    return run_gemm_b(c, gemm_entry_desc(true, A, lda, W, ldw, bias, residual, C, ldc, M, N, K, epilogue, out_bf16), (hipStream_t)stream);
}

extern "C" int fern_gemm_fp8(fern_ctx* c, const uint8_t* A, int64_t lda, const float* scale_a, const uint8_t* W, int64_t ldw, const float* scale_w,
                             const float* bias, const float* residual, void* C, int64_t ldc, int M, int N, int K, int epilogue, int out_bf16,
                             void* stream) {
    const GemmFacts f{"fern_gemm_fp8", /*scales_ok*/ scale_a && scale_w, /*relu_ok*/ false, /*residual_ok*/ true, kEpiList, /*residual_fp32*/ true,
                      "the residual epilogue needs a residual and fp32 output", /*k_mult*/ 64, /*ld_mult*/ 16, /*rows_ok*/ true, "K % 64, lda % 16 and ldw % 16 must be 0"};
    if (const int r = gemm_begin(c, f, A, lda, W, ldw, residual, C, ldc, M, N, K, epilogue, out_bf16)) return r == GEMM_EMPTY ? FERN_OK : r;
    GemmParams p = gemm_entry_desc(true, A, lda, W, ldw, bias, residual, C, ldc, M, N, K, epilogue, out_bf16);
    p.fp8 = 1; p.scale_a = scale_a; p.scale_w = scale_w;
    return run_gemm_b(c, p, (hipStream_t)stream);
}

extern "C" int fern_gemm_mx8(fern_ctx* c, const uint8_t* A, int64_t lda, const uint8_t* scales_a, int64_t scale_rows_a, const uint8_t* W,
                             int64_t ldw, const uint8_t* scales_w, int64_t scale_rows_w, const float* bias, const float* residual, void* C,
                             int64_t ldc, int M, int N, int K, int epilogue, int out_bf16, void* stream) {
    const GemmFacts f{"fern_gemm_mx8", /*scales_ok*/ scales_a && scales_w, /*relu_ok*/ false, /*residual_ok*/ true, kEpiList, /*residual_fp32*/ false,
                      "the residual epilogue needs a residual", /*k_mult*/ 128, /*ld_mult*/ 16, /*rows_ok*/ scale_rows_a >= M && scale_rows_w >= N, "K % 128, lda % 16 and ldw % 16 must be 0, scale_rows >= rows"};
    if (const int r = gemm_begin(c, f, A, lda, W, ldw, residual, C, ldc, M, N, K, epilogue, out_bf16)) return r == GEMM_EMPTY ? FERN_OK : r;
    GemmParams p = gemm_entry_desc(true, A, lda, W, ldw, bias, residual, C, ldc, M, N, K, epilogue, out_bf16);
    p.fp8 = 2; p.mxa = scales_a; p.mxa_rows = scale_rows_a; p.mxw = scales_w; p.mxw_rows = scale_rows_w;
    if (out_bf16 && epilogue == FERN_EPI_BIAS_RESIDUAL) { p.Rb = reinterpret_cast<const unsigned short*>(residual); p.R = nullptr; }      // bf16 residual stream
    return run_gemm_b(c, p, (hipStream_t)stream);
}

extern "C" int fern_gemm_mx8_quant(fern_ctx* c, const uint8_t* A, int64_t lda, const uint8_t* scales_a, int64_t scale_rows_a, const uint8_t* W,
                                   int64_t ldw, const uint8_t* scales_w, int64_t scale_rows_w, const float* bias, uint8_t* C8, int64_t ldc,
                                   uint8_t* scales_c, int64_t scale_rows_c, int M, int N, int K, int epilogue, void* stream) {
    const GemmFacts f{"fern_gemm_mx8_quant", /*scales_ok*/ scales_a && scales_w && scales_c, /*relu_ok*/ false, /*residual_ok*/ false,
                      "epilogue must be BIAS, BIAS_GELU or BIAS_QUICKGELU", /*residual_fp32*/ false, "", /*k_mult*/ 128, /*ld_mult*/ 16, /*rows_ok*/ N % 128 == 0 && ldc % 16 == 0 && scale_rows_a >= M && scale_rows_w >= N && scale_rows_c >= M,
                      "K % 128, N % 128, lda / ldw / ldc % 16 must be 0, scale_rows >= rows"};
    if (const int r = gemm_begin(c, f, A, lda, W, ldw, nullptr, C8, ldc, M, N, K, epilogue, 0)) return r == GEMM_EMPTY ? FERN_OK : r;
    GemmParams p = gemm_entry_desc(true, A, lda, W, ldw, bias, nullptr, C8, ldc, M, N, K, epilogue, 0);
    p.fp8 = 2; p.mxa = scales_a; p.mxa_rows = scale_rows_a; p.mxw = scales_w; p.mxw_rows = scale_rows_w;
    p.out_mx8 = 1; p.mxc = scales_c; p.mxc_rows = scale_rows_c;
    return run_gemm_b(c, p, (hipStream_t)stream);
}

// Common head of the two quantiser entries, refusals then device: their operands, the shape (`shape_ok`, worded by the entry), rows that would overlap.
static int quant_begin(fern_ctx* c, const char* name, const void* x, const void* y, const void* scales, int64_t rows, bool shape_ok,
                       const char* shape_text, int64_t ldx, int64_t ldy, int d) {
    const std::string fn = std::string(name) + ": ";
    if (!c || rows < 0 || (rows && (!x || !y || !scales))) return fail(FERN_ERR_ARG, fn + "bad argument");
    if (!shape_ok) return fail(FERN_ERR_ARG, fn + shape_text);
    if (ldx < d || ldy < d) return fail(FERN_ERR_ARG, fn + "need ldx >= d and ldy >= d (rows must not overlap)");
    HIP_TRY(hipSetDevice(c->device));
    return FERN_OK;
}
// the rows a quantiser reads: bf16 or fp32 behind one pointer, the other form's pointer null
static const unsigned short* rows_bf16(const void* x, int x_is_bf16) { return x_is_bf16 ? static_cast<const unsigned short*>(x) : nullptr; }
static const float* rows_f32(const void* x, int x_is_bf16) { return x_is_bf16 ? nullptr : static_cast<const float*>(x); }

extern "C" int fern_quantize_rows_fp8(fern_ctx* c, const void* x, int x_is_bf16, int64_t ldx, uint8_t* y, int64_t ldy, float* scale, int64_t rows,
                                      int d, void* stream) {
    FERN_TRY(quant_begin(c, "fern_quantize_rows_fp8", x, y, scale, rows, !(d <= 0 || d % 8 || d > 4096 || ldx % 8 || ldy % 8),
                         "need d % 8 == 0, d <= 4096, ld % 8 == 0", ldx, ldy, d));
    HIP_TRY(launch_quantize_rows_fp8(rows_bf16(x, x_is_bf16), rows_f32(x, x_is_bf16), ldx, y, ldy, scale, rows, d, (hipStream_t)stream));
    return FERN_OK;
}

extern "C" int fern_quantize_mx8(fern_ctx* c, const void* x, int x_is_bf16, int64_t ldx, uint8_t* y, int64_t ldy, uint8_t* scales,
                                 int64_t scale_rows, int64_t rows, int d, void* stream) {
    FERN_TRY(quant_begin(c, "fern_quantize_mx8", x, y, scales, rows, !(d <= 0 || d % 128 || d > 4096 || ldx % 8 || ldy % 8 || scale_rows < rows),
                         "need d % 128 == 0, d <= 4096, ld % 8 == 0, scale_rows >= rows", ldx, ldy, d));
    HIP_TRY(launch_quantize_mx8(rows_bf16(x, x_is_bf16), rows_f32(x, x_is_bf16), ldx, y, ldy, scales, scale_rows, rows, d, (hipStream_t)stream));
    return FERN_OK;
}

extern "C" int fern_layernorm(fern_ctx* c, const float* x, const float* residual, const float* gamma, const float* beta, float* y,
                              int64_t rows, int d, float eps, void* stream) {
    if (!c || !x || !gamma || !beta || !y || rows < 0) return fail(FERN_ERR_ARG, "fern_layernorm: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_layernorm(x, residual, gamma, beta, y, rows, d, d, d, eps, (hipStream_t)stream));
    return FERN_OK;
}

// Common head of fern_attention and fern_attention_bf16, refusals then device: a missing operand, rows of heads * head_dim values that would overlap.
// (heads <= 0 or head_dim <= 0 is not refused here: the launcher refuses it.)
static int attn_begin(fern_ctx* c, const std::string& fn, const void* q, const void* k, const void* v, const void* out, int64_t ldq, int64_t ldk,
                      int64_t ldv, int64_t ldo, int heads, int head_dim) {
    if (!c || !q || !k || !v || !out) return fail(FERN_ERR_ARG, fn + ": NULL argument");
    const int64_t w = (int64_t)heads * head_dim;
    if (heads > 0 && head_dim > 0 && (ldq < w || ldk < w || ldv < w || ldo < w))
        return fail(FERN_ERR_ARG, fn + ": need ldq, ldk, ldv, ldo >= heads * head_dim (rows must not overlap)");
    HIP_TRY(hipSetDevice(c->device));
    return FERN_OK;
}
// attention on bf16 operands; `out` is the bf16 output, null where the caller sets another one
static AttnParams attn_desc_b(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v, int64_t ldv, uint16_t* out, int64_t ldo,
                              int batch, int heads, int head_dim, int s_q, int s_k, int causal, float scale) {
    return AttnParams{nullptr, nullptr, nullptr, nullptr, (long)ldq, (long)ldk, (long)ldv, (long)ldo, batch, heads, head_dim, s_q, s_k, causal, scale,
                      out, q, k, v};
}

extern "C" int fern_attention(fern_ctx* c, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* out,
                              int64_t ldo, int batch, int heads, int head_dim, int s_q, int s_k, int causal, float scale, void* stream) {
    FERN_TRY(attn_begin(c, "fern_attention", q, k, v, out, ldq, ldk, ldv, ldo, heads, head_dim));
    AttnParams a{q, k, v, out, (long)ldq, (long)ldk, (long)ldv, (long)ldo, batch, heads, head_dim, s_q, s_k, causal, scale};
    return run_attention(c, a, (hipStream_t)stream);
}

extern "C" int fern_attention_bf16(fern_ctx* c, const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v, int64_t ldv,
                                   uint16_t* out, int64_t ldo, int batch, int heads, int head_dim, int s_q, int s_k, int causal, float scale,
                                   void* stream) {
    FERN_TRY(attn_begin(c, "fern_attention_bf16", q, k, v, out, ldq, ldk, ldv, ldo, heads, head_dim));
    return run_attention(c, attn_desc_b(q, ldq, k, ldk, v, ldv, out, ldo, batch, heads, head_dim, s_q, s_k, causal, scale), (hipStream_t)stream);
}

static bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// One query per (image, head) over tokens whose K / V are not projected: the launch of the fp32 towers' last ViT block and of the
// ResNet's attention pool.  Its scratch is a fresh workspace frame of this context.
extern "C" int fern_pooled_attention(fern_ctx* c, const float* q, int64_t ldq, const float* tokens, int64_t ldt, int64_t image_stride,
                                     const float* wk, const float* wv, const float* bv, float* out, int64_t ldo, int batch, int heads,
                                     int head_dim, int s, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_pooled_attention: ctx is NULL");
    if (!q || !tokens || !wk || !wv || !bv || !out) return fail(FERN_ERR_ARG, "fern_pooled_attention: NULL argument");
    const int64_t E = (int64_t)heads * head_dim;
    if (batch <= 0 || heads <= 0 || head_dim <= 0 || head_dim % 4 || head_dim > 128 || E > POOLED_MAX_E || s <= 0 || s > POOLED_MAX_KEYS)
        return fail(FERN_ERR_ARG, "fern_pooled_attention: need head_dim % 4 == 0, head_dim <= 128, heads * head_dim <= " +
                                      std::to_string(POOLED_MAX_E) + ", 1 <= s <= " + std::to_string(POOLED_MAX_KEYS));
    if (ldq < E || ldt < E || ldo < E || ldq % 4 || ldt % 4 || ldo % 4 || image_stride % 4 || image_stride < (int64_t)(s - 1) * ldt + E)
        return fail(FERN_ERR_ARG, "fern_pooled_attention: need ldq, ldt, ldo >= heads * head_dim, strides % 4 == 0, image_stride >= (s - 1) * ldt + heads * head_dim");
    if (misaligned16(q) || misaligned16(tokens) || misaligned16(wk) || misaligned16(wv) || misaligned16(bv) || misaligned16(out))
        return fail(FERN_ERR_ARG, "fern_pooled_attention: pointers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t st = (hipStream_t)stream;
    FERN_TRY(ws_begin(c, st));
    PooledAttnParams a{q, (long)ldq, tokens, (long)ldt, (long)image_stride, wk, wv, (long)E, bv, out, (long)ldo, nullptr, nullptr,
                       batch, heads, head_dim, s, 1.0f / std::sqrt((float)head_dim)};
    return run_pooled_attention(c, a, st);
}

// ---- the fused producers of the towers' operands (kernel-level parity tests): the launchers the blocks call, nothing else ----

extern "C" int fern_layernorm_q(fern_ctx* c, const void* x, int x_is_bf16, int64_t ldx, const float* gamma, const float* beta, int out_form,
                                void* y, int64_t ldy, void* scales, int64_t scale_rows, int64_t rows, int d, float eps, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_layernorm_q: ctx is NULL");
    if (rows < 0 || (out_form != FERN_QFORM_BF16 && out_form != FERN_QFORM_FP8 && out_form != FERN_QFORM_MX8))
        return fail(FERN_ERR_ARG, "fern_layernorm_q: bad argument");
    if (rows == 0) return FERN_OK;
    if (!x || !gamma || !beta || !y || (out_form != FERN_QFORM_BF16 && !scales)) return fail(FERN_ERR_ARG, "fern_layernorm_q: NULL argument");
    if (d <= 0 || d % 4 || d > 1280 || ldx < d || ldy < d || ldx % 4 || ldy % 4)
        return fail(FERN_ERR_ARG, "fern_layernorm_q: need d % 4 == 0, d <= 1280, ld % 4 == 0, ld >= d");
    if (misaligned16(x) || misaligned16(gamma) || misaligned16(beta) || misaligned16(y) || (scales && misaligned16(scales)))
        return fail(FERN_ERR_ARG, "fern_layernorm_q: pointers must be 16-byte aligned");
    if (out_form == FERN_QFORM_MX8 && (d % 128 || scale_rows < rows))
        return fail(FERN_ERR_ARG, "fern_layernorm_q: the MX form needs d % 128 == 0 and scale_rows >= rows");
    if (out_form != FERN_QFORM_MX8 && x_is_bf16) return fail(FERN_ERR_ARG, "fern_layernorm_q: bf16 rows are read by the MX form only");
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t s = (hipStream_t)stream;
    if (out_form == FERN_QFORM_BF16)
        HIP_TRY(launch_layernorm_bf16(static_cast<const float*>(x), gamma, beta, static_cast<unsigned short*>(y), rows, d, ldx, ldy, eps, s));
    else if (out_form == FERN_QFORM_FP8)
        HIP_TRY(launch_layernorm_fp8(static_cast<const float*>(x), gamma, beta, static_cast<unsigned char*>(y), static_cast<float*>(scales), rows, d,
                                     ldx, ldy, eps, s));
    else
        HIP_TRY(launch_layernorm_mx8(rows_f32(x, x_is_bf16), gamma, beta, static_cast<unsigned char*>(y), static_cast<unsigned char*>(scales), scale_rows,
                                     rows, d, ldx, ldy, eps, s, rows_bf16(x, x_is_bf16)));
    return FERN_OK;
}

extern "C" int fern_attention_mx8(fern_ctx* c, const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v, int64_t ldv,
                                  uint8_t* out, int64_t ldo, uint8_t* scales, int64_t scale_rows, int batch, int heads, int head_dim, int s_q,
                                  int s_k, int causal, float scale, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_attention_mx8: ctx is NULL");
    if (batch <= 0 || heads <= 0 || s_q <= 0 || s_k <= 0 || (causal && s_q != s_k) || s_k > (causal ? 96 : ATTN_MAX_KEYS))
        return fail(FERN_ERR_ARG, "fern_attention_mx8: bad shape");
    const int64_t w = (int64_t)heads * head_dim;
    if (head_dim <= 0 || head_dim % 32 || head_dim > 96 || w % 128)
        return fail(FERN_ERR_ARG, "fern_attention_mx8: need head_dim % 32 == 0, head_dim <= 96, heads * head_dim % 128 == 0");
    if (!q || !k || !v || !out || !scales) return fail(FERN_ERR_ARG, "fern_attention_mx8: NULL argument");
    if (ldq % 8 || ldk % 8 || ldv % 8 || ldq < w || ldk < w || ldv < w || ldo % 16 || ldo < w || scale_rows < (int64_t)batch * s_q)
        return fail(FERN_ERR_ARG, "fern_attention_mx8: need ldq / ldk / ldv % 8 == 0, ldo % 16 == 0, ld >= heads * head_dim, scale_rows >= batch * s_q");
    if (misaligned16(q) || misaligned16(k) || misaligned16(v) || misaligned16(out))
        return fail(FERN_ERR_ARG, "fern_attention_mx8: pointers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    AttnParams a = attn_desc_b(q, ldq, k, ldk, v, ldv, nullptr, ldo, batch, heads, head_dim, s_q, s_k, causal, scale);
    a.out_q8 = out; a.out_scales = scales; a.out_srows = scale_rows;
    return run_attention(c, a, (hipStream_t)stream);
}

extern "C" int fern_im2col_q(fern_ctx* c, const float* images, int b, int img, int patch, int out_form, void* y, void* scales, int64_t scale_rows,
                             void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_im2col_q: ctx is NULL");
    if (b < 0 || (out_form != FERN_QFORM_BF16 && out_form != FERN_QFORM_MX8)) return fail(FERN_ERR_ARG, "fern_im2col_q: bad argument");
    if (b == 0) return FERN_OK;
    if (!images || !y || (out_form == FERN_QFORM_MX8 && !scales)) return fail(FERN_ERR_ARG, "fern_im2col_q: NULL argument");
    const int d = 3 * patch * patch;
    if (patch <= 0 || patch % 4 || img <= 0 || img % patch || d > 1280 || d % (out_form == FERN_QFORM_MX8 ? 128 : 32))
        return fail(FERN_ERR_ARG, "fern_im2col_q: need patch % 4 == 0, img % patch == 0, 3 * patch^2 <= 1280 and % 32 (BF16) / % 128 (MX8) == 0");
    const int grid = img / patch;
    const int64_t rows = (int64_t)b * grid * grid;
    if (out_form == FERN_QFORM_MX8 && scale_rows < rows) return fail(FERN_ERR_ARG, "fern_im2col_q: scale_rows >= rows");
    if (misaligned16(images) || misaligned16(y) || (scales && misaligned16(scales)))
        return fail(FERN_ERR_ARG, "fern_im2col_q: pointers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    if (out_form == FERN_QFORM_BF16)
        HIP_TRY(launch_im2col_bf16(images, static_cast<unsigned short*>(y), b, img, patch, grid, (hipStream_t)stream));
    else
        HIP_TRY(launch_im2col_mx8(images, static_cast<unsigned char*>(y), static_cast<unsigned char*>(scales), scale_rows, b, img, patch, grid,
                                  (hipStream_t)stream));
    return FERN_OK;
}

// ---- the ModifiedResNet's kernels (kernel-level parity tests): the tower's own descriptors and launchers behind an argument check ----

// b * H * W pixel rows as an int, or -1
static int pixel_rows(int b, int H, int W) {
    const int64_t m = (int64_t)b * H * W;
    return m > INT32_MAX ? -1 : (int)m;
}

extern "C" int fern_conv3x3_nhwc(fern_ctx* c, const float* x, const float* w, const float* bias, float* out, int b, int H, int W, int cin, int cout,
                                 void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_conv3x3_nhwc: ctx is NULL");
    if (b < 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0) return fail(FERN_ERR_ARG, "fern_conv3x3_nhwc: bad argument");
    if (b == 0) return FERN_OK;
    if (!x || !w || !bias || !out) return fail(FERN_ERR_ARG, "fern_conv3x3_nhwc: NULL argument");
    const int M = pixel_rows(b, H, W);
    if (cin % 16 || cin > INT32_MAX / 9 || M < 0) return fail(FERN_ERR_ARG, "fern_conv3x3_nhwc: need cin % 16 == 0 and b * H * W < 2^31");
    if (misaligned16(x) || misaligned16(w)) return fail(FERN_ERR_ARG, "fern_conv3x3_nhwc: x and w must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t st = (hipStream_t)stream;
    // the out-of-image taps' source: the finalised tower uploads one with its weights, here it is a zeroed piece of a fresh workspace frame
    float* zeros;
    FERN_TRY(ws_begin(c, st));
    FERN_TRY(ws_get(c, (size_t)64, &zeros));
    HIP_TRY(hipMemsetAsync(zeros, 0, 64 * sizeof(float), st));
    const ConvW cw{w, bias, cout, 9 * cin};
    return run_gemm(c, conv3x3_desc(x, cw, out, b, H, W, cin, zeros), st);
}

extern "C" int fern_conv1x1_nhwc(fern_ctx* c, const float* x, const float* w, const float* bias, const float* residual, float* out, int M, int cin,
                                 int cout, int relu, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_conv1x1_nhwc: ctx is NULL");
    if (M < 0 || cin <= 0 || cout <= 0) return fail(FERN_ERR_ARG, "fern_conv1x1_nhwc: bad argument");
    if (M == 0) return FERN_OK;
    if (!x || !w || !bias || !out) return fail(FERN_ERR_ARG, "fern_conv1x1_nhwc: NULL argument");
    if (residual && !relu) return fail(FERN_ERR_ARG, "fern_conv1x1_nhwc: a residual is added before the ReLU only (fern_gemm has BIAS_RESIDUAL)");
    if (cin % 16) return fail(FERN_ERR_ARG, "fern_conv1x1_nhwc: need cin % 16 == 0");
    if (misaligned16(x) || misaligned16(w)) return fail(FERN_ERR_ARG, "fern_conv1x1_nhwc: x and w must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    const ConvW cw{w, bias, cout, cin};
    GemmParams p = conv_desc(x, cw, out, M, residual ? EPI_BIAS_RESIDUAL_RELU : relu ? EPI_BIAS_RELU : EPI_BIAS);
    p.R = residual;
    return run_gemm(c, p, (hipStream_t)stream);
}

extern "C" int fern_stem_conv(fern_ctx* c, const float* images, const float* w, const float* bias, float* out, int b, int S, int cout_pad,
                              void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_stem_conv: ctx is NULL");
    if (b < 0 || S <= 0 || cout_pad <= 0) return fail(FERN_ERR_ARG, "fern_stem_conv: bad argument");
    if (b == 0) return FERN_OK;
    if (!images || !w || !bias || !out) return fail(FERN_ERR_ARG, "fern_stem_conv: NULL argument");
    if (S % 2 || cout_pad % 4 || pixel_rows(b, S / 2, S / 2) < 0) return fail(FERN_ERR_ARG, "fern_stem_conv: need S % 2 == 0, cout_pad % 4 == 0 and b * (S / 2)^2 < 2^31");
    if (misaligned16(bias) || misaligned16(out)) return fail(FERN_ERR_ARG, "fern_stem_conv: bias and out must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_stem_conv(images, w, bias, out, b, S, cout_pad, (hipStream_t)stream));
    return FERN_OK;
}

extern "C" int fern_avgpool_nhwc(fern_ctx* c, const float* x, float* y, int b, int H, int W, int C, int k, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_avgpool_nhwc: ctx is NULL");
    if (b < 0 || H <= 0 || W <= 0 || C <= 0 || k < 1) return fail(FERN_ERR_ARG, "fern_avgpool_nhwc: bad argument");
    if (b == 0) return FERN_OK;
    if (!x || !y) return fail(FERN_ERR_ARG, "fern_avgpool_nhwc: NULL argument");
    if (C % 4 || H % k || W % k || pixel_rows(b, H, W) < 0) return fail(FERN_ERR_ARG, "fern_avgpool_nhwc: need C % 4 == 0, H % k == 0, W % k == 0 and b * H * W < 2^31");
    if (misaligned16(x) || misaligned16(y)) return fail(FERN_ERR_ARG, "fern_avgpool_nhwc: pointers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_avgpool_nhwc(x, y, b, H, W, C, k, (hipStream_t)stream));
    return FERN_OK;
}

extern "C" int fern_attnpool_tokens(fern_ctx* c, const float* x, const float* pos, float* T, float* T0, int b, int HW, int C, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_attnpool_tokens: ctx is NULL");
    if (b < 0 || HW <= 0 || C <= 0) return fail(FERN_ERR_ARG, "fern_attnpool_tokens: bad argument");
    if (b == 0) return FERN_OK;
    if (!x || !pos || !T || !T0) return fail(FERN_ERR_ARG, "fern_attnpool_tokens: NULL argument");
    if (C % 4 || HW == INT32_MAX || pixel_rows(b, HW + 1, 1) < 0) return fail(FERN_ERR_ARG, "fern_attnpool_tokens: need C % 4 == 0 and b * (HW + 1) < 2^31");
    if (misaligned16(x) || misaligned16(pos) || misaligned16(T) || misaligned16(T0)) return fail(FERN_ERR_ARG, "fern_attnpool_tokens: pointers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t st = (hipStream_t)stream;
    float* mean;      // [b, C], the tower's arena slot
    FERN_TRY(ws_begin(c, st));
    FERN_TRY(ws_get(c, (size_t)b * C, &mean));
    HIP_TRY(launch_attnpool_tokens(x, mean, pos, T, T0, b, HW, C, st));
    return FERN_OK;
}

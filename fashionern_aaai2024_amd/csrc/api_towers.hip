// C-ABI layer of libfern.so: the CLIP towers.  One block recipe in four operand forms, the ViT / text / pair walkers over it, the
// ModifiedResNet walker, and the three encoder entry points.
#include <cmath>
#include "ctx.h"

using namespace fern;
using namespace fern::api;

// A pre-LN residual block (modeling_clip.py:354-401) is two halves -- x += attn(ln_1(x)); x += mlp(ln_2(x)) -- and each half runs its two
// token-level GEMMs in one operand form.  Accumulation, the LayerNorm statistics and the attention softmax are fp32 in every form.
//   F32   fp32 operands (the parity mode; under f32x3 the GEMMs run split, run_gemm).
//   BF16  perf mode: LayerNorm / attention / GELU outputs are rounded to bf16 as they are written, weights are the bf16 copies.
//   FP8   (BASELINE config 5: "fp8 MFMA encoder path") e4m3fn operands with per-token activation scales and per-output-channel weight
//         scales, folded back in the fp32 epilogue.  LayerNorm quantises as it writes; the attention and GELU outputs are written as bf16
//         (a row's maximum is not known inside those kernels) and quantised by a row pass.  Attention itself runs on bf16 operands.
//   MX    FP8 with block-scaled operands -- one E8M0 scale per (token, 32 channels) and per (output channel, 32 inputs), applied inside
//         v_mfma_scale_f32_32x32x64_f8f6f4 (twice the MFMA rate of the plain fp8 form, and an outlier channel costs its own 32-block
//         precision, not the whole token row).  The attention kernel (head dim a multiple of 32) and c_fc quantise their outputs where
//         they are produced (fp32 values -> e4m3fn + block scales): no bf16 round trip, no extra pass.
enum Form { F32, BF16, FP8, MX };

// One tower's chunk: weights, shape, the form of each half and the workspace.  The reduced forms keep their operands inside the fp32-sized
// buffers; the accessors below are the only place those offsets are written.
struct Tower {
    const ClipBlockW* blocks;
    int batch, S, width, heads, mlp, causal;
    Form attn, mlpf;
    bool bf16_stream;      // the mode's residual stream is bf16: the walker allocates Xb where full blocks run
    float *X, *XN, *QKV, *ATT, *H;
    unsigned short* Xb;    // the bf16 residual stream (X is then not read by the blocks); null: the stream is the fp32 X

    long R() const { return (long)batch * S; }
    void* stream() const { return Xb ? (void*)Xb : (void*)X; }
    // XN / QKV / ATT / H double as the bf16 operand buffers (half filled)
    unsigned short* XNb() const { return reinterpret_cast<unsigned short*>(XN); }
    unsigned short* QKVb() const { return reinterpret_cast<unsigned short*>(QKV); }
    unsigned short* ATTb() const { return reinterpret_cast<unsigned short*>(ATT); }
    unsigned short* Hb() const { return reinterpret_cast<unsigned short*>(H); }
    // XN: fp8 rows, the scales of the operand in flight behind them (FP8: one float per row; MX: the same area holds E8M0 bytes)
    unsigned char* XN8() const { return reinterpret_cast<unsigned char*>(XN); }
    float* SA() const { return XN + ((size_t)R() * width / 4 + 63) / 64 * 64; }
    unsigned char* SM() const { return reinterpret_cast<unsigned char*>(SA()); }
    unsigned char* SH() const { return SM() + ((size_t)R() * (width / 32) + 255) / 256 * 256; }      // H's MX scales, behind the LayerNorm output's
    // ATT / H: bf16 output in the first half, its fp8 copy behind it; c_fc in the MX form writes fp8 directly, at H
    unsigned char* ATT8() const { return reinterpret_cast<unsigned char*>(ATT) + (size_t)R() * width * 2; }
    unsigned char* H8(Form f) const { return reinterpret_cast<unsigned char*>(H) + (f == MX ? 0 : (size_t)R() * mlp * 2); }
};

// precision mode -> the forms of a tower's halves and its residual stream.
//   mx8     (FERN_PREC_MX8) both halves MX over a BF16 residual stream (round 4): the two residual GEMMs of a block read and write it in
//           place (C = bf16(acc + bias + Xb): one rounding per residual add) and the LayerNorms read it -- out-proj / c_proj were HBM-bound
//           on their 2 x 39 MB of fp32 residual traffic per launch (M = 12608), the LayerNorm + quantise passes on their 39 MB reads.
//   mx8mlp  (FERN_PREC_MX8_MLP) the attention half BF16, the MLP half -- two thirds of a block's GEMM flops -- MX, over the fp32 stream:
//           half of the fp8 rounding points of mx8 (and its bf16 residual stream) are gone; bench.py's `reduced_modes` table has what
//           that buys.
//   mx8img  (FERN_PREC_MX8_IMG, round 6) the attention half MX too where the attention kernel can quantise its own output (head dim a
//           multiple of 32), still over the FP32 stream: all four GEMMs at the fp8 rate without mx8's bf16 stream, whose 24 extra
//           roundings per tower cost more Recall than the four GEMMs' operands do.
//   The TEXT tower runs BF16 throughout under mx8mlp / mx8img (round 6): its GEMMs (M = 77 B rows, K = 512) are the ones the block-scaled
//   kernels run worst (0.07-0.12 of their peak) and its rounding points sit directly on the query: e4m3 there cost 0.9 pp of Recall@50
//   (bench.py `reduced_modes`: mx8mlp -1.03 -> -0.15 pp) for ~0.1 ms of a 4 ms step.
static void tower_forms(const fern_ctx* c, bool text, Tower* T) {
    T->attn = T->mlpf = F32;
    T->bf16_stream = false;
    switch (c->precision) {
    case FERN_PREC_BF16: T->attn = T->mlpf = BF16; break;
    case FERN_PREC_FP8: T->attn = T->mlpf = FP8; break;
    case FERN_PREC_MX8: T->attn = T->mlpf = MX; T->bf16_stream = true; break;
    case FERN_PREC_MX8_MLP:
    case FERN_PREC_MX8_IMG:
        T->attn = !text && c->precision == FERN_PREC_MX8_IMG && (T->width / T->heads) % 32 == 0 ? MX : BF16;
        T->mlpf = text ? BF16 : MX;
        break;
    default: break;
    }
}

// Shape, weights and forms of one tower for a chunk of `batch` samples, and its five buffers (fp32-sized in every mode).
static int tower_open(fern_ctx* c, bool text, int batch, Tower* T) {
    const ClipW& W = c->clip;
    const fern_clip_config& cf = W.cfg;
    const int g = cf.image_size / cf.patch_size;
    if (text) *T = Tower{W.tblocks.data(), batch, cf.context_length, cf.t_width, cf.t_heads, cf.t_mlp, 1};
    else *T = Tower{W.vblocks.data(), batch, g * g + 1, cf.v_width, cf.v_heads, cf.v_mlp, 0};
    tower_forms(c, text, T);
    const size_t R = (size_t)T->R();
    FERN_TRY(ws_get(c, R * T->width, &T->X));
    FERN_TRY(ws_get(c, R * T->width, &T->XN));
    FERN_TRY(ws_get(c, R * 3 * T->width, &T->QKV));
    FERN_TRY(ws_get(c, R * T->width, &T->ATT));
    return ws_get(c, R * T->mlp, &T->H);
}

static int run_gemm_form(fern_ctx* c, Form f, const GemmParams& p, hipStream_t s) { return f == F32 ? run_gemm(c, p, s) : run_gemm_b(c, p, s); }

// LayerNorm of the residual stream into XN in operand form f, and the descriptor of the GEMM that reads it.
static int ln_gemm(const Tower& T, Form f, const LNW& ln, const LinearW& L, void* C, long ldc, int epi, bool out_bf16, hipStream_t s, GemmParams* p) {
    const long R = T.R();
    const int w = T.width;
    switch (f) {
    case F32:
        HIP_TRY(launch_layernorm(T.X, nullptr, ln.g, ln.b, T.XN, R, w, w, w, 1e-5f, s));
        *p = gemm_desc(T.XN, w, L, reinterpret_cast<float*>(C), ldc, (int)R, epi);
        break;
    case BF16:
        HIP_TRY(launch_layernorm_bf16(T.X, ln.g, ln.b, T.XNb(), R, w, w, w, 1e-5f, s));
        *p = gemm_desc_b(T.XNb(), w, L, C, ldc, (int)R, epi, out_bf16);
        break;
    case FP8:
        HIP_TRY(launch_layernorm_fp8(T.X, ln.g, ln.b, T.XN8(), T.SA(), R, w, w, w, 1e-5f, s));
        *p = gemm_desc_f8(T.XN8(), T.SA(), w, L, C, ldc, (int)R, epi, out_bf16);
        break;
    case MX:
        HIP_TRY(launch_layernorm_mx8(T.Xb ? nullptr : T.X, ln.g, ln.b, T.XN8(), T.SM(), R, R, w, w, w, 1e-5f, s, T.Xb));
        *p = gemm_desc_mx(T.XN8(), T.SM(), R, w, L, C, ldc, (int)R, epi, out_bf16);
        break;
    }
    return FERN_OK;
}
// out-proj / c_proj write the residual stream in place.  Only the MX form runs over the bf16 stream (tower_forms).
static void residual_in_place(const Tower& T, GemmParams* p) {
    if (T.Xb) p->Rb = T.Xb;
    else p->R = T.X;
}

// The four steps of a block: each launches what precedes its GEMM and fills the GEMM's descriptor.
static int prep_qkv(fern_ctx*, const Tower& T, const ClipBlockW& Bk, hipStream_t s, GemmParams* p) {
    return ln_gemm(T, T.attn, Bk.ln1, Bk.qkv, T.QKV, 3 * T.width, EPI_BIAS, true, s, p);
}
static int prep_out(fern_ctx* c, const Tower& T, const ClipBlockW& Bk, hipStream_t s, GemmParams* p) {
    const long R = T.R();
    const int w = T.width, hd = w / T.heads;
    const bool fused = T.attn == MX && hd % 32 == 0;      // the attention kernel quantises its fp32 output itself (the QKV GEMM is done with SM by now)
    if (T.attn == F32) {
        AttnParams a{T.QKV, T.QKV + w, T.QKV + 2 * w, T.ATT, 3L * w, 3L * w, 3L * w, (long)w,
                     T.batch, T.heads, hd, T.S, T.S, T.causal, 1.0f / std::sqrt((float)hd)};
        FERN_TRY(run_attention(c, a, s));
    } else {
        AttnParams a{nullptr, nullptr, nullptr, nullptr, 3L * w, 3L * w, 3L * w, (long)w,
                     T.batch, T.heads, hd, T.S, T.S, T.causal, 1.0f / std::sqrt((float)hd), T.ATTb(), T.QKVb(), T.QKVb() + w, T.QKVb() + 2 * w};
        if (fused) { a.out_b = nullptr; a.out_q8 = T.ATT8(); a.out_scales = T.SM(); a.out_srows = R; }
        FERN_TRY(run_attention(c, a, s));
    }
    switch (T.attn) {
    case F32: *p = gemm_desc(T.ATT, w, Bk.out, T.X, w, (int)R, EPI_BIAS_RESIDUAL); break;
    case BF16: *p = gemm_desc_b(T.ATTb(), w, Bk.out, T.X, w, (int)R, EPI_BIAS_RESIDUAL, false); break;
    case FP8:
        HIP_TRY(launch_quantize_rows_fp8(T.ATTb(), nullptr, w, T.ATT8(), w, T.SA(), R, w, s));
        *p = gemm_desc_f8(T.ATT8(), T.SA(), w, Bk.out, T.X, w, (int)R, EPI_BIAS_RESIDUAL, false);
        break;
    case MX:
        if (!fused) HIP_TRY(launch_quantize_mx8(T.ATTb(), nullptr, w, T.ATT8(), w, T.SM(), R, R, w, s));
        *p = gemm_desc_mx(T.ATT8(), T.SM(), R, w, Bk.out, T.stream(), w, (int)R, EPI_BIAS_RESIDUAL, T.Xb != nullptr);
        break;
    }
    residual_in_place(T, p);
    return FERN_OK;
}
static int prep_fc(fern_ctx* c, const Tower& T, const ClipBlockW& Bk, hipStream_t s, GemmParams* p) {
    FERN_TRY(ln_gemm(T, T.mlpf, Bk.ln2, Bk.fc, T.H, T.mlp, clip_mlp_epi(c), T.mlpf != MX, s, p));
    if (T.mlpf == MX) { p->out_mx8 = 1; p->mxc = T.SH(); p->mxc_rows = T.R(); }
    return FERN_OK;
}
static int prep_proj(fern_ctx*, const Tower& T, const ClipBlockW& Bk, hipStream_t s, GemmParams* p) {
    const long R = T.R();
    const int w = T.width, mlp = T.mlp;
    switch (T.mlpf) {
    case F32: *p = gemm_desc(T.H, mlp, Bk.proj, T.X, w, (int)R, EPI_BIAS_RESIDUAL); break;
    case BF16: *p = gemm_desc_b(T.Hb(), mlp, Bk.proj, T.X, w, (int)R, EPI_BIAS_RESIDUAL, false); break;
    case FP8:
        HIP_TRY(launch_quantize_rows_fp8(T.Hb(), nullptr, mlp, T.H8(FP8), mlp, T.SA(), R, mlp, s));
        *p = gemm_desc_f8(T.H8(FP8), T.SA(), mlp, Bk.proj, T.X, w, (int)R, EPI_BIAS_RESIDUAL, false);
        break;
    case MX:
        *p = gemm_desc_mx(T.H8(MX), T.SH(), R, mlp, Bk.proj, T.stream(), w, (int)R, EPI_BIAS_RESIDUAL, T.Xb != nullptr);
        break;
    }
    residual_in_place(T, p);
    return FERN_OK;
}

static int tower_block(fern_ctx* c, const Tower& T, int l, hipStream_t s) {
    const ClipBlockW& Bk = T.blocks[l];
    GemmParams p;
    FERN_TRY(prep_qkv(c, T, Bk, s, &p));
    FERN_TRY(run_gemm_form(c, T.attn, p, s));
    FERN_TRY(prep_out(c, T, Bk, s, &p));
    FERN_TRY(run_gemm_form(c, T.attn, p, s));
    FERN_TRY(prep_fc(c, T, Bk, s, &p));
    FERN_TRY(run_gemm_form(c, T.mlpf, p, s));
    FERN_TRY(prep_proj(c, T, Bk, s, &p));
    return run_gemm_form(c, T.mlpf, p, s);
}

// Last ViT block: only the class token is consumed afterwards (ln_post on token 0, modeling_clip.py:876-877), so
// Q, the attention output, out_proj and the MLP run for the class rows only.  The reduced forms project K/V for every token; the fp32
// forms do not project them at all: with one query per (image, head) both projections fold into the query and the output (attn.hip:
// pooled single-query attention -- exact algebra, the key bias cancels in the softmax).
// Equal to the full block on the rows that are read only to TOLERANCE since round 5, and still: the single-query attention (folded or
// not) and the 512-wide split-K c_proj add their products in another order than the full block's kernels (fp32 parity mode included).
// V.Xb (FERN_PREC_MX8 with its bf16 residual stream): the stream itself -- the token-level LayerNorm reads it as the full blocks do and
// only the class rows are widened to fp32 (X is then not read: round 5 dropped the 58 MB bf16 -> fp32 pass over the whole stream).
static int clip_block_cls_only(fern_ctx* c, const Tower& V, const ClipBlockW& Bk, float* CLS /*[b,width] out*/, float* T0 /*[b,width]*/,
                               float* T1 /*[b,width]*/, float* H /*[b,mlp]*/, hipStream_t s) {
    const int batch = V.batch, S = V.S, width = V.width, heads = V.heads, hd = width / heads;
    const float* X = V.X;
    const unsigned short* Xb = V.Xb;
    float* QKV = V.QKV;
    LinearW kv{Bk.qkv.w + (size_t)width * width, Bk.qkv.b + width, 2 * width, width, Bk.qkv.wb + (size_t)width * width,
               Bk.qkv.w8 ? Bk.qkv.w8 + (size_t)width * width : nullptr, Bk.qkv.sw ? Bk.qkv.sw + width : nullptr,
               Bk.qkv.wm ? Bk.qkv.wm + (size_t)width * width : nullptr, Bk.qkv.swm ? Bk.qkv.swm + (size_t)width * 4 : nullptr, Bk.qkv.swm_rows};
    // token-level ln_1 in the attention half's form; this block stays BF16 under FERN_PREC_MX8_IMG as under FERN_PREC_MX8_MLP
    const Form f = c->precision == FERN_PREC_MX8_IMG ? BF16 : V.attn;
    // The fp32 data flow (fp32, f32x3) attends over ln_1(x) itself and never projects K / V; the reduced forms (their oracles restate the
    // rounding points of the projected K / V) and shapes past the pooled kernels' limits project them for every token (fp32 output).
    const bool pooled = f == F32 && S <= POOLED_MAX_KEYS && width <= POOLED_MAX_E && hd <= 128;
    if (pooled) {
        HIP_TRY(launch_layernorm(X, nullptr, Bk.ln1.g, Bk.ln1.b, V.XN, V.R(), width, width, width, 1e-5f, s));
    } else {
        GemmParams pk;
        FERN_TRY(ln_gemm(V, f, Bk.ln1, kv, QKV + width, 3 * width, EPI_BIAS, false, s, &pk));
        FERN_TRY(run_gemm_form(c, f, pk, s));                                                          // K, V for all tokens
    }
    if (f == F32) {
        HIP_TRY(launch_gather_rows(V.XN, width, T0, width, batch, width, 1, S, 0, nullptr, s));        // ln_1(x)[:, 0]
    } else {      // the class-row chain below stays fp32 in every form
        if (Xb) HIP_TRY(launch_gather_rows_bf16(Xb, width, T1, width, batch, width, S, s));
        else HIP_TRY(launch_gather_rows(X, width, T1, width, batch, width, 1, S, 0, nullptr, s));      // x[:, 0]
        HIP_TRY(launch_layernorm(T1, nullptr, Bk.ln1.g, Bk.ln1.b, T0, batch, width, width, width, 1e-5f, s));   // ln_1(x)[:, 0]
    }
    LinearW qw{Bk.qkv.w, Bk.qkv.b, width, width};
    FERN_TRY(run_gemm(c, gemm_desc(T0, width, qw, T1, width, batch, EPI_BIAS), s));                    // Q for the class rows
    if (pooled) {
        // one query per (batch, head) over ln_1(x) itself: K / V of the tokens are never formed (attn.hip: the pooled single-query attention)
        PooledAttnParams a{T1, (long)width, V.XN, (long)width, (long)S * width, kv.w, kv.w + (size_t)width * width, (long)width, kv.b + width,
                           T0, (long)width, nullptr, nullptr, batch, heads, hd, S, 1.0f / std::sqrt((float)hd)};
        FERN_TRY(run_pooled_attention(c, a, s));
    } else {
        // one query per (batch, head): q rows are [batch, 1]; K/V are read in place from the packed buffer
        AttnParams a{T1, QKV + width, QKV + 2 * width, T0, (long)width, 3L * width, 3L * width, (long)width,
                     batch, heads, hd, 1, S, 0, 1.0f / std::sqrt((float)hd)};
        FERN_TRY(run_attention(c, a, s));
    }
    if (Xb) HIP_TRY(launch_gather_rows_bf16(Xb, width, CLS, width, batch, width, S, s));               // residual x[:, 0]
    else HIP_TRY(launch_gather_rows(X, width, CLS, width, batch, width, 1, S, 0, nullptr, s));
    GemmParams po = gemm_desc(T0, width, Bk.out, CLS, width, batch, EPI_BIAS_RESIDUAL);
    po.R = CLS;
    FERN_TRY(run_gemm(c, po, s));
    HIP_TRY(launch_layernorm(CLS, nullptr, Bk.ln2.g, Bk.ln2.b, T0, batch, width, width, width, 1e-5f, s));
    FERN_TRY(run_gemm(c, gemm_desc(T0, width, Bk.fc, H, Bk.fc.out, batch, clip_mlp_epi(c)), s));
    GemmParams p2 = gemm_desc(H, Bk.fc.out, Bk.proj, CLS, width, batch, EPI_BIAS_RESIDUAL);
    p2.R = CLS;
    // The class rows' c_proj is M = batch with an unsplit k chain of 3072 (ViT-B): 24 workgroups walking 48 k tiles each, 58 us.  Like
    // the query-side combiners' hidden layer (CombinerW.ksplit) K is cut into 512-wide slices at THIS call site, for every batch size
    // (kernels.h: GemmParams.ksplit): 144 workgroups, ~12 us + a 5 us reduce that adds the slices in ascending order.
    const int ks = (Bk.fc.out >= 2048 && Bk.fc.out % 512 == 0 && (width & 3) == 0) ? Bk.fc.out / 512 : 1;
    if (ks > 1) {
        float* kpart;
        FERN_TRY(ws_get(c, (size_t)ks * batch * width, &kpart));
        p2.ksplit = ks; p2.kpart = kpart; p2.epi = EPI_BIAS; p2.R = nullptr;      // slices store raw sums; bias + residual happen in the reduce
        FERN_TRY(run_gemm(c, p2, s));
        HIP_TRY(launch_splitk_bias_residual(kpart, ks, batch, width, Bk.proj.b, CLS, width, CLS, width, s));
        return FERN_OK;
    }
    return run_gemm(c, p2, s);
}

// Front of the ViT tower: conv1 over the patches (its epilogue adds the positional embedding and skips the class slot) and the class token.
// H is free until the first block: the reduced-precision modes stage their rounded patch rows there.
static int vit_front(fern_ctx* c, const float* images, float* X, float* H, int b, hipStream_t s) {
    const ClipW& W = c->clip;
    const fern_clip_config& cf = W.cfg;
    const int vw = cf.v_width, g = cf.image_size / cf.patch_size, g2 = g * g, S = g2 + 1;
    if (W.conv_kp) {
        // patch sides the 16-byte patch loaders do not take (14): fp32 patch rows zero-padded to conv_kp columns, then the plain-loader fp32
        // GEMM against the padded weight; same epilogue.  Every precision mode: the reduced modes define no patch embedding for these shapes
        const long rows = (long)b * g2;
        float* P = H;
        // H is [b * S, v_mlp] FLOATS in both walkers (vit_chunk, pair_chunk: tower_open): element counts are compared
        if ((size_t)rows * W.conv_kp > (size_t)b * S * cf.v_mlp) FERN_TRY(ws_get(c, (size_t)rows * W.conv_kp, &P));      // narrow MLPs (test towers)
        HIP_TRY(launch_patch_rows_f32(images, P, b, cf.image_size, cf.patch_size, g, W.conv_kp, s));
        LinearW conv{W.conv_wp, nullptr, vw, W.conv_kp};
        GemmParams pp = gemm_desc(P, W.conv_kp, conv, X, vw, (int)rows, EPI_PATCH_EMBED);
        pp.aux0 = W.vpos; pp.grid = g;
        FERN_TRY(run_gemm(c, pp, s));
    } else if (c->precision == FERN_PREC_MX8 && W.conv_mx.wm && (3 * cf.patch_size * cf.patch_size) <= 1280) {
        // block-scaled mode: patch rows are quantised once (H is free until the first block) and conv1 runs on the scaled MFMA;
        // same epilogue (positional embedding added, class slot skipped)
        const int kd = 3 * cf.patch_size * cf.patch_size;
        const long rows = (long)b * g2;
        unsigned char* A8 = reinterpret_cast<unsigned char*>(H);
        unsigned char* SA = A8 + ((size_t)rows * kd + 255) / 256 * 256;
        HIP_TRY(launch_im2col_mx8(images, A8, SA, rows, b, cf.image_size, cf.patch_size, g, s));
        GemmParams pm = gemm_desc_mx(A8, SA, rows, kd, W.conv_mx, X, vw, (int)rows, EPI_PATCH_EMBED, false);
        pm.aux0 = W.vpos; pm.grid = g;
        FERN_TRY(run_gemm_b(c, pm, s));
    } else if ((c->precision == FERN_PREC_BF16 || c->precision == FERN_PREC_MX8_MLP || c->precision == FERN_PREC_MX8_IMG) && W.conv_mx.wb &&
               (3 * cf.patch_size * cf.patch_size) <= 1280) {
        // bf16-operand modes (round 6): patch rows rounded to bf16 once (H is free until the first block), conv1 on the bf16 MFMA; same epilogue
        const int kd = 3 * cf.patch_size * cf.patch_size;
        const long rows = (long)b * g2;
        unsigned short* Ab = reinterpret_cast<unsigned short*>(H);
        HIP_TRY(launch_im2col_bf16(images, Ab, b, cf.image_size, cf.patch_size, g, s));
        GemmParams pb = gemm_desc_b(Ab, kd, W.conv_mx, X, vw, (int)rows, EPI_PATCH_EMBED, false);
        pb.aux0 = W.vpos; pb.grid = g;
        FERN_TRY(run_gemm_b(c, pb, s));
    } else {
    // conv1 as an im2col-free GEMM; epilogue adds the positional embedding and skips the class slot
    GemmParams pe{};
    pe.A = images; pe.W = W.conv_w; pe.ldw = 3L * cf.patch_size * cf.patch_size; pe.C = X; pe.ldc = vw;
    pe.M = b * g2; pe.N = vw; pe.K = 3 * cf.patch_size * cf.patch_size;
    pe.epi = EPI_PATCH_EMBED; pe.aload = ALOAD_IM2COL; pe.aux0 = W.vpos;
    pe.img = cf.image_size; pe.patch = cf.patch_size; pe.grid = g;
    FERN_TRY(run_gemm(c, pe, s));
    }
    HIP_TRY(launch_vit_cls(W.cls, W.vpos, X, b, S, vw, s));
    return FERN_OK;
}

// Tail of the ViT tower: the last block for the class rows only, ln_post, the visual projection (modeling_clip.py:876-887).  ATT / H are
// free after the last full block: their heads are the [b, width] / [b, mlp] temporaries.
static int vit_tail(fern_ctx* c, const Tower& V, float* CLS, float* out, hipStream_t s) {
    const ClipW& W = c->clip;
    const fern_clip_config& cf = W.cfg;
    const int vw = V.width, b = V.batch;
    FERN_TRY(clip_block_cls_only(c, V, W.vblocks[cf.v_layers - 1], CLS, V.ATT, V.ATT + (size_t)b * vw, V.H, s));
    HIP_TRY(launch_layernorm(CLS, nullptr, W.ln_post.g, W.ln_post.b, CLS, b, vw, vw, vw, 1e-5f, s));
    LinearW proj{W.vproj_t, nullptr, cf.embed_dim, vw};
    return run_gemm(c, gemm_desc(CLS, vw, proj, out, cf.embed_dim, b, EPI_BIAS), s);
}
// Tail of the text tower: ln_final over every token, the text projection of all rows (out_seq; global == seq[EOT]) or of the EOT rows only
// (modeling_clip.py:760-768, models/clip_model.py:23-31).
static int text_tail(fern_ctx* c, const float* X, float* XN, const int* eot, float* out_global, float* out_seq, int B, hipStream_t s) {
    const ClipW& W = c->clip;
    const fern_clip_config& cf = W.cfg;
    const int tw = cf.t_width, T = cf.context_length, E = cf.embed_dim;
    const long R = (long)B * T;
    HIP_TRY(launch_layernorm(X, nullptr, W.ln_final.g, W.ln_final.b, XN, R, tw, tw, tw, 1e-5f, s));
    LinearW proj{W.tproj_t, nullptr, E, tw};
    if (out_seq) {
        FERN_TRY(run_gemm(c, gemm_desc(XN, tw, proj, out_seq, E, (int)R, EPI_BIAS), s));
        if (out_global) HIP_TRY(launch_gather_rows(out_seq, E, out_global, E, B, E, 1, T, 0, eot, s));   // global == seq[EOT]
    } else if (out_global) {
        float* pooled;
        FERN_TRY(ws_get(c, (size_t)B * tw, &pooled));
        HIP_TRY(launch_gather_rows(XN, tw, pooled, tw, B, tw, 1, T, 0, eot, s));
        FERN_TRY(run_gemm(c, gemm_desc(pooled, tw, proj, out_global, E, B, EPI_BIAS), s));
    }
    return FERN_OK;
}

// Images per chunk of the ViT walkers (vit_chunk, pair_chunk): 64 up to 197 tokens -- what every tower before ViT-L/14 ran
// with -- and beyond that as many as keep a chunk at those 64 x 197 = 12 608 token rows (257 tokens: 49 images, 577: 21), so the workspace
// grows with the tower's width only.  Rows are batch-invariant: where a chunk ends changes no result.
static int vit_chunk_images(const fern_clip_config& cf) {
    const int g = cf.image_size / cf.patch_size, S = g * g + 1;
    return std::max(1, std::min(64, 64 * 197 / S));
}

static int vit_chunk(fern_ctx* c, const float* images, float* out, int b, hipStream_t s) {
    const ClipW& W = c->clip;
    Tower V;
    float* CLS;
    FERN_TRY(tower_open(c, false, b, &V));
    FERN_TRY(ws_get(c, (size_t)b * V.width, &CLS));
    FERN_TRY(vit_front(c, images, V.X, V.H, b, s));
    const long R = V.R();
    const int vw = V.width;
    if (V.bf16_stream && W.cfg.v_layers > 1) {
        FERN_TRY(ws_get(c, (size_t)R * vw, &V.Xb));
        HIP_TRY(launch_layernorm_bf16(V.X, W.ln_pre.g, W.ln_pre.b, V.Xb, R, vw, vw, vw, 1e-5f, s));      // ln_pre writes the stream (rounded once)
    } else {
        HIP_TRY(launch_layernorm(V.X, nullptr, W.ln_pre.g, W.ln_pre.b, V.X, R, vw, vw, vw, 1e-5f, s));
    }
    for (int l = 0; l + 1 < W.cfg.v_layers; ++l) FERN_TRY(tower_block(c, V, l, s));
    // the class-row chain of the last block is fp32; with the bf16 stream only the class rows are widened (exactly), inside the block
    return vit_tail(c, V, CLS, out, s);
}

// ---- open_clip ModifiedResNet (RN50x4).  Activations are NHWC, so every 1x1 convolution is a plain GEMM over the pixel
// rows, every 3x3 convolution the same GEMM with the 3x3-window A loader, BatchNorm is folded into the weights and the
// ReLU / residual add live in the GEMM epilogue.
GemmParams fern::api::conv_desc(const float* A, const ConvW& W, float* C, int M, int epi) {
    GemmParams p{};
    p.A = A; p.lda = W.k; p.W = W.w; p.ldw = W.k; p.bias = W.b; p.C = C; p.ldc = W.cout;
    p.M = M; p.N = W.cout; p.K = W.k; p.epi = epi; p.aload = ALOAD_PLAIN;
    return p;
}
GemmParams fern::api::conv3x3_desc(const float* A, const ConvW& W, float* C, int b, int H, int Wd, int cin, const float* zeros) {
    GemmParams p = conv_desc(A, W, C, b * H * Wd, EPI_BIAS_RELU);
    p.aload = ALOAD_CONV3; p.conv_h = H; p.conv_w = Wd; p.conv_c = cin; p.zeros = zeros;
    return p;
}
static int conv3x3(fern_ctx* c, const float* A, const ConvW& W, float* C, int b, int H, int Wd, int cin, hipStream_t s) {
    return run_gemm(c, conv3x3_desc(A, W, C, b, H, Wd, cin, c->clip.res.zeros), s);
}

static int resnet_chunk(fern_ctx* c, const float* images, float* out, int b, hipStream_t s) {
    const ClipW& W = c->clip;
    const ResNetW& R = W.res;
    const fern_clip_config& cf = W.cfg;
    const int S = cf.image_size, s1 = S / 2, w = cf.r_width;
    // one arena slot sized for the largest activation of the tower, six of them reused round-robin
    size_t max_act = (size_t)b * s1 * s1 * std::max(R.stem_c, w);
    {
        int H = S / 4;
        for (const auto& B : R.blocks) {
            max_act = std::max(max_act, (size_t)b * H * H * std::max(B.cin, B.planes * 4));
            if (B.stride > 1) H /= 2;
        }
    }
    {
        const int hf = S / 32;
        max_act = std::max(max_act, (size_t)b * (hf * hf + 1) * (size_t)(w * 32));      // attention-pool token rows (their K/V are never formed)
    }
    float* buf[6];
    for (auto& p : buf) FERN_TRY(ws_get(c, max_act, &p));
    // stem
    HIP_TRY(launch_stem_conv(images, R.stem1.w, R.stem1.b, buf[0], b, S, R.stem_c, s));
    FERN_TRY(conv3x3(c, buf[0], R.stem2, buf[1], b, s1, s1, R.stem_c, s));
    FERN_TRY(conv3x3(c, buf[1], R.stem3, buf[0], b, s1, s1, R.stem_c, s));
    HIP_TRY(launch_avgpool_nhwc(buf[0], buf[1], b, s1, s1, w, 2, s));
    float* X = buf[1];
    float* OUT = buf[0];
    int H = S / 4;
    for (const auto& B : R.blocks) {
        const int rows = b * H * H, Ho = H / B.stride, rows_o = b * Ho * Ho;
        float *T1 = buf[2], *T2 = buf[3], *TP = buf[4], *ID = buf[5];
        FERN_TRY(run_gemm(c, conv_desc(X, B.c1, T1, rows, EPI_BIAS_RELU), s));                    // 1x1 + BN + ReLU
        FERN_TRY(conv3x3(c, T1, B.c2, T2, b, H, H, B.planes, s));                                  // 3x3 + BN + ReLU
        const float* t2 = T2;
        const float* xin = X;
        if (B.stride > 1) {
            HIP_TRY(launch_avgpool_nhwc(T2, T1, b, H, H, B.planes, B.stride, s));                  // anti-aliasing avg-pool
            t2 = T1;
            HIP_TRY(launch_avgpool_nhwc(X, TP, b, H, H, B.cin, B.stride, s));
            xin = TP;
        }
        const float* identity = X;
        if (B.has_down) {
            FERN_TRY(run_gemm(c, conv_desc(xin, B.down, ID, rows_o, EPI_BIAS), s));                // shortcut: [avg-pool] + 1x1 + BN
            identity = ID;
        }
        GemmParams p3 = conv_desc(t2, B.c3, OUT, rows_o, EPI_BIAS_RESIDUAL_RELU);                  // 1x1 + BN + identity + ReLU
        p3.R = identity;
        FERN_TRY(run_gemm(c, p3, s));
        std::swap(X, OUT);
        H = Ho;
    }
    // AttentionPool2d: NHWC rows of one image are already its HW tokens
    const int HW = H * H, E = w * 32, heads = cf.r_heads, hd = E / heads;
    float *T = buf[2], *T0 = buf[3], *MEAN = buf[3] + (size_t)b * E, *Q = buf[5], *ATT = buf[5] + (size_t)b * E;
    HIP_TRY(launch_attnpool_tokens(X, MEAN, R.pos, T, T0, b, HW, E, s));
    FERN_TRY(run_gemm(c, gemm_desc(T0, E, R.q, Q, E, b, EPI_BIAS), s));
    // one query per (image, head) over the token rows themselves (attn.hip: the pooled single-query attention)
    PooledAttnParams a{Q, (long)E, T, (long)E, (long)(HW + 1) * E, R.kv.w, R.kv.w + (size_t)E * E, (long)E, R.kv.b + E,
                       ATT, (long)E, nullptr, nullptr, b, heads, hd, HW + 1, 1.0f / std::sqrt((float)hd)};
    FERN_TRY(run_pooled_attention(c, a, s));
    return run_gemm(c, gemm_desc(ATT, E, R.cproj, out, cf.embed_dim, b, EPI_BIAS), s);
}

extern "C" int fern_vit_encode_image(fern_ctx* c, const float* images, float* out, int b, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_vit_encode_image: ctx is NULL");
    if (!c->clip.ready || (c->clip.cfg.v_arch == 0 && c->clip.cfg.v_layers <= 0))
        return fail(FERN_ERR_STATE, "fern_vit_encode_image: image tower not finalised (fern_finalize_clip)");
    FERN_TRY(check_fresh(c, "fern_vit_encode_image"));
    if (b < 0 || (b && (!images || !out))) return fail(FERN_ERR_ARG, "fern_vit_encode_image: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const fern_clip_config& cf = c->clip.cfg;
    const long img_sz = 3L * cf.image_size * cf.image_size;
    const bool resnet = cf.v_arch == 1;
    const int CH = resnet ? 128 : vit_chunk_images(cf);      // the ResNet's late stages have few pixels per image: larger chunks fill the chip (M = 128 x 81 rows)
    return for_query_chunks(c, s, b, CH, [&](long o, int m) -> int {
        return resnet ? resnet_chunk(c, images + o * img_sz, out + o * cf.embed_dim, m, s) : vit_chunk(c, images + o * img_sz, out + o * cf.embed_dim, m, s);
    });
}

static int text_chunk(fern_ctx* c, const int64_t* tokens, float* out_global, float* out_seq, int B, hipStream_t s) {
    const ClipW& W = c->clip;
    const fern_clip_config& cf = W.cfg;
    Tower T;
    int* eot;
    FERN_TRY(tower_open(c, true, B, &T));
    FERN_TRY(ws_get(c, (size_t)B, &eot));
    HIP_TRY(launch_text_embed(tokens, W.tok_emb, W.tpos, T.X, eot, B, T.S, T.width, cf.vocab_size, c->tok_flag, s));
    if (T.bf16_stream) {
        FERN_TRY(ws_get(c, (size_t)T.R() * T.width, &T.Xb));
        HIP_TRY(launch_f32_to_bf16(T.X, T.Xb, T.R() * T.width, s));
    }
    for (int l = 0; l < cf.t_layers; ++l) FERN_TRY(tower_block(c, T, l, s));
    if (T.Xb) HIP_TRY(launch_bf16_to_f32(T.Xb, T.X, T.R() * T.width, s));
    return text_tail(c, T.X, T.XN, eot, out_global, out_seq, B, s);
}

// Both towers of a composed query in one pass (round 6): the image tower's full blocks and the text tower's blocks are
// walked LAYER BY LAYER and the four GEMMs of a layer -- QKV, out-proj, c_fc, c_proj -- are issued as image + text PAIRS: the text layer's
// few hundred tiles ride in the image layer's launch and back-fill its tail instead of running as under-filled launches of their own.
// Two data flows pair (fern_encode_pair): fp32 (FERN_PREC_FP32, also under f32x3: run_gemm_pair) and FERN_PREC_MX8_IMG (the c5 default)
// with both image halves MX and the text tower BF16 (run_gemm_b_pair).  Everything else (LayerNorms, attention, the class-row block, the
// projections) is issued exactly as vit_chunk / text_chunk issue it, and every GEMM computes the same tiles in the same k order: the
// features are bit-identical to fern_vit_encode_image + fern_text_encode.
static int pair_chunk(fern_ctx* c, const float* images, float* out_img, const int64_t* tokens, float* out_global, float* out_seq, int b, hipStream_t s) {
    const ClipW& W = c->clip;
    const fern_clip_config& cf = W.cfg;
    Tower V, T;
    float* CLS;
    int* eot;
    FERN_TRY(tower_open(c, false, b, &V));
    FERN_TRY(ws_get(c, (size_t)b * V.width, &CLS));
    FERN_TRY(tower_open(c, true, b, &T));
    FERN_TRY(ws_get(c, (size_t)b, &eot));
    // image tower front: conv1 (epilogue adds the positional embedding), class token, ln_pre -- as vit_chunk
    FERN_TRY(vit_front(c, images, V.X, V.H, b, s));
    HIP_TRY(launch_layernorm(V.X, nullptr, W.ln_pre.g, W.ln_pre.b, V.X, V.R(), V.width, V.width, V.width, 1e-5f, s));
    // text tower front -- as text_chunk
    HIP_TRY(launch_text_embed(tokens, W.tok_emb, W.tpos, T.X, eot, b, T.S, T.width, cf.vocab_size, c->tok_flag, s));
    const int vfull = cf.v_layers - 1;                     // the image tower's last block runs for the class rows only
    const int paired = vfull < cf.t_layers ? vfull : cf.t_layers;
    const bool mx = V.attn == MX;
    auto run_pair = [&](const GemmParams& pv, const GemmParams& pt) { return mx ? run_gemm_b_pair(c, pv, pt, s) : run_gemm_pair(c, pv, pt, s); };
    for (int l = 0; l < paired; ++l) {
        const ClipBlockW &Bv = V.blocks[l], &Bt = T.blocks[l];
        GemmParams pv, pt;
        FERN_TRY(prep_qkv(c, V, Bv, s, &pv));
        FERN_TRY(prep_qkv(c, T, Bt, s, &pt));
        FERN_TRY(run_pair(pv, pt));
        FERN_TRY(prep_out(c, V, Bv, s, &pv));
        FERN_TRY(prep_out(c, T, Bt, s, &pt));
        FERN_TRY(run_pair(pv, pt));
        FERN_TRY(prep_fc(c, V, Bv, s, &pv));
        FERN_TRY(prep_fc(c, T, Bt, s, &pt));
        FERN_TRY(run_pair(pv, pt));
        FERN_TRY(prep_proj(c, V, Bv, s, &pv));
        FERN_TRY(prep_proj(c, T, Bt, s, &pt));
        FERN_TRY(run_pair(pv, pt));
    }
    for (int l = paired; l < vfull; ++l) FERN_TRY(tower_block(c, V, l, s));
    for (int l = paired; l < cf.t_layers; ++l) FERN_TRY(tower_block(c, T, l, s));
    FERN_TRY(vit_tail(c, V, CLS, out_img, s));
    return text_tail(c, T.X, T.XN, eot, out_global, out_seq, b, s);
}

// A token id outside the vocabulary cannot raise from inside a kernel (nn.Embedding does, in the reference): the embedding
// kernel poisons the row with NaN and sets a host-mapped flag; it is turned into FERN_ERR_ARG here, at fern_sync and at the
// next fern_text_encode -- without a synchronisation on the launch path.
int fern::api::check_token_flag(fern_ctx* c, const char* fn) {
    if (!c->tok_flag) return FERN_OK;
    const int v = __atomic_load_n(c->tok_flag, __ATOMIC_RELAXED);
    if (v == 0) return FERN_OK;
    __atomic_store_n(c->tok_flag, 0, __ATOMIC_RELAXED);
    return fail(FERN_ERR_ARG, std::string(fn) + ": an earlier fern_text_encode on this context read a token id outside [0, vocab_size) at flat "
                                                 "position " + std::to_string(v - 1) + " of its chunk (its features are NaN): tokenizer / vocabulary mismatch?");
}

// Common head of the entries that embed tokens: device, the flag (allocated on first use), the error an earlier call left behind.
static int token_begin(fern_ctx* c, const char* fn) {
    HIP_TRY(hipSetDevice(c->device));
    if (!c->tok_flag) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->tok_flag), sizeof(int), hipHostMallocMapped));
        *c->tok_flag = 0;
    }
    return check_token_flag(c, fn);
}

extern "C" int fern_text_encode(fern_ctx* c, const int64_t* tokens, const float* visual_emb, const int64_t* visual_emb_shape, float* out_global,
                                float* out_seq, int B, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_text_encode: ctx is NULL");
    if (!c->clip.ready || c->clip.cfg.t_layers <= 0) return fail(FERN_ERR_STATE, "fern_text_encode: text tower not finalised (fern_finalize_clip)");
    FERN_TRY(check_fresh(c, "fern_text_encode"));
    if (B < 0 || (B && (!tokens || (!out_global && !out_seq)))) return fail(FERN_ERR_ARG, "fern_text_encode: bad argument");
    const fern_clip_config& cf = c->clip.cfg;
    if (visual_emb) {      // clip_model.py:23-31: visual_emb = ref_patch_feats.transpose(0, 1), [13, B, D]; checked, then unused (vanilla CLIP branch)
        if (!visual_emb_shape || visual_emb_shape[0] != 13 || visual_emb_shape[1] != B || visual_emb_shape[2] != cf.embed_dim)
            return fail(FERN_ERR_ARG, "fern_text_encode: visual_emb must be [13, B, embed_dim]");
    }
    FERN_TRY(token_begin(c, "fern_text_encode"));
    hipStream_t s = (hipStream_t)stream;
    return for_query_chunks(c, s, B, 256, [&](long o, int m) -> int {
        return text_chunk(c, tokens + o * cf.context_length, out_global ? out_global + o * cf.embed_dim : nullptr,
                          out_seq ? out_seq + o * cf.context_length * cf.embed_dim : nullptr, m, s);
    });
}

extern "C" int fern_encode_pair(fern_ctx* c, const float* images, const int64_t* tokens, float* out_image, float* out_global, float* out_seq, int B,
                                void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_encode_pair: ctx is NULL");
    if (!c->clip.ready) return fail(FERN_ERR_STATE, "fern_encode_pair: CLIP weights not finalised (fern_finalize_clip)");
    FERN_TRY(check_fresh(c, "fern_encode_pair"));
    if (B < 0 || (B && (!images || !tokens || !out_image || (!out_global && !out_seq)))) return fail(FERN_ERR_ARG, "fern_encode_pair: bad argument");
    const fern_clip_config& cf = c->clip.cfg;
    const bool towers = cf.v_arch == 0 && cf.v_layers > 1 && cf.t_layers > 0;
    // the mixed mode pairs when every image GEMM of a block is block-scaled (head dim a multiple of 32: tower_forms) and the text GEMMs
    // meet the bf16 family's k tiling
    const bool pair_mx = towers && c->precision == FERN_PREC_MX8_IMG && (cf.v_width / cf.v_heads) % 32 == 0 && cf.v_width % 128 == 0 &&
                         cf.v_mlp % 128 == 0 && cf.t_width % 32 == 0 && cf.t_mlp % 32 == 0;
    const bool pairable = towers && (c->precision == FERN_PREC_FP32 || pair_mx);
    if (!pairable) {      // every other mode / tower: the two entry points, one after the other (same results by definition)
        FERN_TRY(fern_vit_encode_image(c, images, out_image, B, stream));
        return fern_text_encode(c, tokens, nullptr, nullptr, out_global, out_seq, B, stream);
    }
    FERN_TRY(token_begin(c, "fern_encode_pair"));
    hipStream_t s = (hipStream_t)stream;
    const long img_sz = 3L * cf.image_size * cf.image_size;
    const int CH = vit_chunk_images(cf);                    // vit_chunk's chunk: the pairing keeps the image tower's launch shapes
    return for_query_chunks(c, s, B, CH, [&](long o, int m) -> int {
        return pair_chunk(c, images + o * img_sz, out_image + o * cf.embed_dim, tokens + o * cf.context_length,
                          out_global ? out_global + o * cf.embed_dim : nullptr, out_seq ? out_seq + o * cf.context_length * cf.embed_dim : nullptr, m, s);
    });
}

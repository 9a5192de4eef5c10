// C-ABI layer of libfern.so: the launch sequences of the fusion head (VisualSR, the combiners, the DVR query module and the gallery's
// index fusion) and the small feature utilities beside them.  Weights come from api_weights.hip, the workspace from the caller's arena.
#include <cmath>
#include "ctx.h"

using namespace fern;
using namespace fern::api;

// ---- fusion building blocks (internal; workspace comes from the caller's arena) -------------------------------------------------
// VisualSR.forward (fusion_model.py:141-154): the [13n, D] local embedding is never materialised --
// the GEMM epilogue applies BN13+tanh, multiplies by the global embedding and reduces against w_common.
static int run_visual_sr(fern_ctx* c, const SRW& W, const float* local, float* out, long n, int D, hipStream_t s) {
    float *raw, *g, *partial;
    FERN_TRY(ws_get(c, (size_t)n * D, &raw));
    FERN_TRY(ws_get(c, (size_t)n * D, &g));
    HIP_TRY(launch_mean_rows(local, D, raw, D, n, 13, D, 13, 0, s));
    GemmParams pg = gemm_desc(raw, D, W.global, g, D, (int)n, EPI_COLAFFINE_TANH);
    pg.aux0 = W.bnd_scale; pg.aux1 = W.bnd_shift;
    FERN_TRY(run_gemm(c, pg, s));
    const int M = (int)(n * 13);
    const int nb = gemm_num_col_blocks(M, D, D);
    FERN_TRY(ws_get(c, (size_t)M * nb, &partial));
    GemmParams pl = gemm_desc(local, D, W.local, nullptr, D, M, EPI_SR_LOCAL);
    pl.aux0 = W.wc; pl.aux1 = W.bn13_mean; pl.aux2 = W.bn13_inv; pl.aux3 = W.bn13_beta;
    pl.G = g; pl.ldg = D; pl.partial = partial;
    FERN_TRY(run_gemm(c, pl, s));
    HIP_TRY(launch_sr_finalize(partial, nb, W.bc, local, out, n, D, s));
    return FERN_OK;
}

// CombinerSimple.forward (fusion_model.py:86-94): the 8D hidden layer only exists inside the GEMM
// epilogue, which reduces it against dynamic_scalar.3.weight on the fly.
static int run_combiner(fern_ctx* c, const CombinerW& W, const float* image, const float* text, float* out, long n, int D, hipStream_t s) {
    float *cat, *partial;
    const int Pj = W.text.out, H = 2 * Pj;      // cat(text_proj, image_proj) width; ERN: 8D
    FERN_TRY(ws_get(c, (size_t)n * H, &cat));
    FERN_TRY(run_gemm(c, gemm_desc(text, D, W.text, cat, H, (int)n, EPI_BIAS_RELU), s));          // :87,:90 text first
    FERN_TRY(run_gemm(c, gemm_desc(image, D, W.image, cat + Pj, H, (int)n, EPI_BIAS_RELU), s));   // :88
    const int nb = gemm_num_col_blocks((int)n, W.hidden.out, H);
    FERN_TRY(ws_get(c, (size_t)n * nb, &partial));
    GemmParams ph = gemm_desc(cat, H, W.hidden, nullptr, H, (int)n, EPI_RELU_DOT);
    ph.aux0 = W.w2; ph.partial = partial;
    if (W.ksplit > 1) {
        float* kpart;
        FERN_TRY(ws_get(c, (size_t)W.ksplit * n * W.hidden.out, &kpart));
        ph.ksplit = W.ksplit; ph.kpart = kpart; ph.epi = EPI_BIAS;      // slices store raw sums; bias + ReLU + dot happen in the reduce
        FERN_TRY(run_gemm(c, ph, s));
        HIP_TRY(launch_splitk_relu_dot(kpart, W.ksplit, n, W.hidden.out, W.hidden.b, W.w2, partial, s));
    } else {
        FERN_TRY(run_gemm(c, ph, s));
    }
    HIP_TRY(launch_combiner_finalize(partial, nb, W.b2, image, text, out, n, D, s));
    return FERN_OK;
}

static int check_fusion(fern_ctx* c, const char* fn, int parts) {
    if (!c) return fail(FERN_ERR_ARG, std::string(fn) + ": ctx is NULL");
    if ((c->fusion.parts & parts) != parts) return fail(FERN_ERR_STATE, std::string(fn) + ": fusion weights not finalised (fern_finalize_fusion)");
    FERN_TRY(check_fresh(c, fn));
    HIP_TRY(hipSetDevice(c->device));
    return FERN_OK;
}

extern "C" int fern_combiner(fern_ctx* c, int which, const float* image, const float* text, float* out, int64_t n, void* stream) {
    if (which < 0 || which > 3) return fail(FERN_ERR_ARG, "fern_combiner: bad combiner id");
    FERN_TRY(check_fusion(c, "fern_combiner", which == FERN_COMBINER_TARGET ? FERN_PART_TARGET_COMBINER : FERN_PART_DVR));
    if ( n < 0 || (n && (!image || !text || !out))) return fail(FERN_ERR_ARG, "fern_combiner: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int D = c->fusion.D;
    return for_query_chunks(c, s, n, 8192, [&](long o, int m) -> int {
        return run_combiner(c, c->fusion.comb[which], image + o * D, text + o * D, out + o * D, m, D, s);
    });
}

extern "C" int fern_visual_sr(fern_ctx* c, int which, const float* local, float* out, int64_t n, void* stream) {
    if (which < 0 || which > 1) return fail(FERN_ERR_ARG, "fern_visual_sr: bad VisualSR id");
    FERN_TRY(check_fusion(c, "fern_visual_sr", which == FERN_SR_TARGET ? FERN_PART_TARGET_SR : FERN_PART_DVR));
    if ( n < 0 || (n && (!local || !out))) return fail(FERN_ERR_ARG, "fern_visual_sr: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int D = c->fusion.D;
    return for_query_chunks(c, s, n, 8192, [&](long o, int m) -> int {
        return run_visual_sr(c, c->fusion.sr[which], local + o * 13 * D, out + o * D, m, D, s);
    });
}

// models/others/Combiner_Model.py (CLIP4Cir Combiner, CVPR'22): the variant of CombinerSimple with a residual
// output_layer(relu(combiner_layer(cat))) branch; its Linear layers take inputs of width 2 * clip_feature_dim (fern_finalize_clip4cir).
extern "C" int fern_combiner_clip4cir(fern_ctx* c, const float* image, const float* text, float* out, int64_t n, void* stream) {
    if (!c) return fail(FERN_ERR_ARG, "fern_combiner_clip4cir: ctx is NULL");
    if (!c->c4c.ready) return fail(FERN_ERR_STATE, "fern_combiner_clip4cir: weights not finalised (fern_finalize_clip4cir)");
    FERN_TRY(check_fresh(c, "fern_combiner_clip4cir"));
    if (n < 0 || (n && (!image || !text || !out))) return fail(FERN_ERR_ARG, "fern_combiner_clip4cir: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const Clip4CirW& W = c->c4c;
    const int Wd = W.width, Pj = W.text.out, H2 = 2 * Pj, Hd = W.comb.out;
    return for_query_chunks(c, s, n, 8192, [&](long o, int m) -> int {
        float *cat, *comb, *O, *partial;
        FERN_TRY(ws_get(c, (size_t)m * H2, &cat));
        FERN_TRY(ws_get(c, (size_t)m * Hd, &comb));
        FERN_TRY(ws_get(c, (size_t)m * Wd, &O));
        const float *im = image + o * Wd, *tx = text + o * Wd;
        FERN_TRY(run_gemm(c, gemm_desc(tx, Wd, W.text, cat, H2, m, EPI_BIAS_RELU), s));              // :49-51
        FERN_TRY(run_gemm(c, gemm_desc(im, Wd, W.image, cat + Pj, H2, m, EPI_BIAS_RELU), s));        // :52-54
        FERN_TRY(run_gemm(c, gemm_desc(cat, H2, W.comb, comb, Hd, m, EPI_BIAS_RELU), s));            // :59-61
        FERN_TRY(run_gemm(c, gemm_desc(comb, Hd, W.outl, O, Wd, m, EPI_BIAS), s));                   // output_layer
        const int nb = gemm_num_col_blocks(m, Hd, H2);
        FERN_TRY(ws_get(c, (size_t)m * nb, &partial));
        GemmParams ph = gemm_desc(cat, H2, W.hidden, nullptr, H2, m, EPI_RELU_DOT);                  // dynamic_scalar
        ph.aux0 = W.w2; ph.partial = partial;
        FERN_TRY(run_gemm(c, ph, s));
        HIP_TRY(launch_combiner_finalize(partial, nb, W.b2, im, tx, out + o * Wd, m, Wd, s, O));     // :63-70
        return FERN_OK;
    });
}

// utils.element_wise_sum (utils/utils.py:133-140): F.normalize(image_features + text_features)
extern "C" int fern_element_wise_sum(fern_ctx* c, const float* image, const float* text, float* out, int64_t n, int d, void* stream) {
    if (!c || n < 0 || (n && (!image || !text || !out))) return fail(FERN_ERR_ARG, "fern_element_wise_sum: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_l2norm(image, d, out, d, n, d, 1e-12f, 0, (hipStream_t)stream, text));
    return FERN_OK;
}

// losses/loss.py:10-14 BatchBasedClassificationLoss.forward: cross_entropy(100 * predicted @ target.T, arange(B)), forward value
extern "C" int fern_batch_classification_loss(fern_ctx* c, const float* predicted, const float* target, int B, int D, float* out_loss,
                                              void* stream) {
    if (!c || B < 1 || D < 1 || !predicted || !target || !out_loss) return fail(FERN_ERR_ARG, "fern_batch_classification_loss: bad argument");
    if (D % 16) return fail(FERN_ERR_ARG, "fern_batch_classification_loss: D must be a multiple of 16");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    FERN_TRY(ws_begin(c, s));
    const long ld = (B + 3) & ~3L;
    float *logits, *rows;
    FERN_TRY(ws_get(c, (size_t)B * ld, &logits));
    FERN_TRY(ws_get(c, (size_t)B, &rows));
    GemmParams p{};
    p.A = predicted; p.lda = D; p.W = target; p.ldw = D; p.C = logits; p.ldc = ld; p.M = B; p.N = B; p.K = D; p.epi = EPI_BIAS; p.aload = ALOAD_PLAIN;
    FERN_TRY(run_gemm(c, p, s));
    HIP_TRY(launch_ce_diag_mean(logits, ld, B, 100.0f, rows, out_loss, s));
    return FERN_OK;
}

extern "C" int fern_l2_normalize(fern_ctx* c, const float* x, float* out, int64_t n, int d, void* stream) {
    if (!c || n < 0 || (n && (!x || !out))) return fail(FERN_ERR_ARG, "fern_l2_normalize: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_l2norm(x, d, out, d, n, d, 1e-12f, 0, (hipStream_t)stream));
    return FERN_OK;
}

extern "C" int fern_index_fuse(fern_ctx* c, const float* tar_feats, const float* tar_local, float* out, int64_t n, int normalize_input,
                               void* stream) {
    FERN_TRY(check_fusion(c, "fern_index_fuse", FERN_PART_TARGET_SR | FERN_PART_TARGET_COMBINER));
    if (n < 0 || (n && (!tar_feats || !tar_local || !out))) return fail(FERN_ERR_ARG, "fern_index_fuse: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int D = c->fusion.D;
    // 8192 gallery rows per tile: bounds the [rows, 8D] Combiner buffer (the reference runs the whole gallery as ONE batch)
    return for_query_chunks(c, s, n, 8192, [&](long o, int m) -> int {
        const float* img = tar_feats + o * D;
        if (normalize_input) {
            float* tn;
            FERN_TRY(ws_get(c, (size_t)m * D, &tn));
            HIP_TRY(launch_l2norm(img, D, tn, D, m, D, 1e-12f, 0, s));      // F.normalize, test_fiq.py:45
            img = tn;
        }
        float* sr;
        FERN_TRY(ws_get(c, (size_t)m * D, &sr));
        FERN_TRY(run_visual_sr(c, c->fusion.sr[FERN_SR_TARGET], tar_local + o * 13 * D, sr, m, D, s));      // model.py:65
        return run_combiner(c, c->fusion.comb[FERN_COMBINER_TARGET], img, sr, out + o * D, m, D, s);        // model.py:66
    });
}

// ERN mode="test" (model.py:68-69 -> DVR_module.forward, fusion_model.py:26-55)
static int dvr_chunk(fern_ctx* c, const float* ref_global, const float* ref_local, const float* text_global, const float* text_seq,
                     float* out, int B, int T, hipStream_t s) {
    const FusionW& F = c->fusion;
    const int D = F.D, P = 13, S = 1 + P + T, heads = 8, hd = D / heads;
    const long R = (long)B * S;
    const int inter = F.layer[0].inter.out;
    float *X, *X1, *QKV, *ATT, *H;
    FERN_TRY(ws_get(c, (size_t)R * D, &X));
    FERN_TRY(ws_get(c, (size_t)R * D, &X1));
    FERN_TRY(ws_get(c, (size_t)R * 3 * D, &QKV));
    FERN_TRY(ws_get(c, (size_t)R * D, &ATT));
    FERN_TRY(ws_get(c, (size_t)R * inter, &H));
    // PlusModel / BertEmbeddings (fusion_model.py:199-212)
    HIP_TRY(launch_bert_embed(F.cls, ref_local, text_seq, F.type, F.pos, F.emb_ln.g, F.emb_ln.b, X, B, P, T, D, 1e-12f, s));
    const bool reduced = c->precision != FERN_PREC_FP32;
    unsigned short* Xb = nullptr;
    if (reduced) FERN_TRY(ws_get(c, (size_t)R * D, &Xb));
    for (int l = 0; l < 2; ++l) {
        const BertLayerW& L = F.layer[l];
        if (reduced) {
            // Reduced-precision modes (bf16 and fp8 alike): the two BERT blocks follow the towers' bf16 recipe -- bf16 operands
            // on the four token-level GEMMs and the attention, fp32 accumulation, fp32 residual stream and LayerNorm.
            unsigned short* QKVb = reinterpret_cast<unsigned short*>(QKV);
            unsigned short* ATTb = reinterpret_cast<unsigned short*>(ATT);
            unsigned short* Hb = reinterpret_cast<unsigned short*>(H);
            HIP_TRY(launch_f32_to_bf16(X, Xb, R * D, s));
            FERN_TRY(run_gemm_b(c, gemm_desc_b(Xb, D, L.qkv, QKVb, 3 * D, (int)R, EPI_BIAS, true), s));
            AttnParams ab{nullptr, nullptr, nullptr, nullptr, 3L * D, 3L * D, 3L * D, (long)D, B, heads, hd, S, S, 0,
                          1.0f / std::sqrt((float)hd), ATTb, QKVb, QKVb + D, QKVb + 2 * D};
            FERN_TRY(run_attention(c, ab, s));
            GemmParams qo = gemm_desc_b(ATTb, D, L.attn_out, X1, D, (int)R, EPI_BIAS_RESIDUAL, false);
            qo.R = X;
            FERN_TRY(run_gemm_b(c, qo, s));
            HIP_TRY(launch_layernorm(X1, nullptr, L.ln1.g, L.ln1.b, X1, R, D, D, D, 1e-12f, s));
            HIP_TRY(launch_f32_to_bf16(X1, Xb, R * D, s));
            FERN_TRY(run_gemm_b(c, gemm_desc_b(Xb, D, L.inter, Hb, inter, (int)R, EPI_BIAS_GELU, true), s));
            GemmParams q2 = gemm_desc_b(Hb, inter, L.out, X, D, (int)R, EPI_BIAS_RESIDUAL, false);
            q2.R = X1;
            FERN_TRY(run_gemm_b(c, q2, s));
            HIP_TRY(launch_layernorm(X, nullptr, L.ln2.g, L.ln2.b, X, R, D, D, D, 1e-12f, s));
            continue;
        }
        FERN_TRY(run_gemm(c, gemm_desc(X, D, L.qkv, QKV, 3 * D, (int)R, EPI_BIAS), s));
        AttnParams a{QKV, QKV + D, QKV + 2 * D, ATT, 3L * D, 3L * D, 3L * D, (long)D, B, heads, hd, S, S, 0, 1.0f / std::sqrt((float)hd)};
        FERN_TRY(run_attention(c, a, s));
        GemmParams po = gemm_desc(ATT, D, L.attn_out, X1, D, (int)R, EPI_BIAS_RESIDUAL);
        po.R = X;
        FERN_TRY(run_gemm(c, po, s));
        HIP_TRY(launch_layernorm(X1, nullptr, L.ln1.g, L.ln1.b, X1, R, D, D, D, 1e-12f, s));
        FERN_TRY(run_gemm(c, gemm_desc(X1, D, L.inter, H, inter, (int)R, EPI_BIAS_GELU), s));
        GemmParams p2 = gemm_desc(H, inter, L.out, X, D, (int)R, EPI_BIAS_RESIDUAL);
        p2.R = X1;
        FERN_TRY(run_gemm(c, p2, s));
        HIP_TRY(launch_layernorm(X, nullptr, L.ln2.g, L.ln2.b, X, R, D, D, D, 1e-12f, s));
    }
    // F.normalize every row of last_hidden_state (rows 1..13 image, 14.. text; row 0 is never read) -- :38-41
    float* XN = X1;
    HIP_TRY(launch_l2norm(X, D, XN, D, R, D, 1e-12f, 0, s));
    // MR_component: only output rows 0..12 survive (:47), so Q is projected for the first 13 text rows only
    const long Rp = (long)B * P;
    float *IMG, *TXT, *Q13, *KV, *CA, *CROSS, *PV, *TM, *G, *Lf;
    FERN_TRY(ws_get(c, (size_t)Rp * D, &IMG));
    FERN_TRY(ws_get(c, (size_t)Rp * D, &TXT));
    FERN_TRY(ws_get(c, (size_t)Rp * D, &Q13));
    FERN_TRY(ws_get(c, (size_t)Rp * 2 * D, &KV));
    FERN_TRY(ws_get(c, (size_t)Rp * D, &CA));
    FERN_TRY(ws_get(c, (size_t)Rp * D, &CROSS));
    FERN_TRY(ws_get(c, (size_t)B * D, &PV));
    FERN_TRY(ws_get(c, (size_t)B * D, &TM));
    FERN_TRY(ws_get(c, (size_t)B * D, &G));
    FERN_TRY(ws_get(c, (size_t)B * D, &Lf));
    HIP_TRY(launch_gather_rows(XN, D, IMG, D, Rp, D, P, S, 1, nullptr, s));
    HIP_TRY(launch_gather_rows(XN, D, TXT, D, Rp, D, P, S, 1 + P, nullptr, s));
    FERN_TRY(run_gemm(c, gemm_desc(TXT, D, F.mha_q, Q13, D, (int)Rp, EPI_BIAS), s));
    FERN_TRY(run_gemm(c, gemm_desc(IMG, D, F.mha_kv, KV, 2 * D, (int)Rp, EPI_BIAS), s));
    AttnParams ca{Q13, KV, KV + D, CA, (long)D, 2L * D, 2L * D, (long)D, B, heads, hd, P, P, 0, 1.0f / std::sqrt((float)hd)};
    FERN_TRY(run_attention(c, ca, s));
    FERN_TRY(run_gemm(c, gemm_desc(CA, D, F.mha_out, CROSS, D, (int)Rp, EPI_BIAS), s));
    FERN_TRY(run_visual_sr(c, F.sr[FERN_SR_DVR], CROSS, PV, B, D, s));                                   // :48
    HIP_TRY(launch_mean_rows(XN, D, TM, D, B, T, D, S, 1 + P, s));                                       // :49
    FERN_TRY(run_combiner(c, F.comb[FERN_COMBINER_DVR_GLOBAL], ref_global, text_global, G, B, D, s));    // :52
    FERN_TRY(run_combiner(c, F.comb[FERN_COMBINER_DVR_LOCAL], PV, TM, Lf, B, D, s));                     // :53
    return run_combiner(c, F.comb[FERN_COMBINER_DVR_FINAL], G, Lf, out, B, D, s);                        // :54
}

extern "C" int fern_dvr_fuse(fern_ctx* c, const float* ref_global, const float* ref_local, const float* text_global, const float* text_seq,
                             float* out, int B, int seq_len, void* stream) {
    FERN_TRY(check_fusion(c, "fern_dvr_fuse", FERN_PART_DVR));
    if (B < 0 || (B && (!ref_global || !ref_local || !text_global || !text_seq || !out))) return fail(FERN_ERR_ARG, "fern_dvr_fuse: bad argument");
    // the MR cross-attention keeps output rows [:13] of the text queries (fusion_model.py:47) and feeds them to BatchNorm1d(13):
    // fewer than 13 text rows fail there in the reference; here they would read the next sample's rows
    if (seq_len < 13 || 1 + 13 + seq_len > 96) return fail(FERN_ERR_ARG, "fern_dvr_fuse: need 13 <= seq_len and 1 + 13 + seq_len <= 96");
    hipStream_t s = (hipStream_t)stream;
    const int D = c->fusion.D;
    return for_query_chunks(c, s, B, 256, [&](long o, int m) -> int {
        return dvr_chunk(c, ref_global + o * D, ref_local + o * 13 * D, text_global + o * D, text_seq + o * seq_len * D, out + o * D, m, seq_len, s);
    });
}

/*
 * fern.h -- C ABI of libfern.so: the MI355X (gfx950) implementation of FashionERN's
 * encode -> fuse -> rank inference path.
 *
 * The reference has no FFI: the path sits behind a Python object protocol
 * (SURVEY.md section 8b).  Each entry point below names the reference interface it replaces
 * (paths relative to the reference repository root).  All pointers are raw device pointers
 * unless a parameter is called `host_*`; matrices are row-major, contiguous unless an ld* is
 * given; fp32 throughout (the reference evaluates in fp32: run/test/test_fiq.py:145,169).
 *
 * Conventions
 *   - every function returns 0 on success, a negative fern_status otherwise;
 *     fern_last_error() returns a message for the calling thread's last failure;
 *   - launch functions are asynchronous on `stream` (a hipStream_t passed as void*) and never
 *     synchronise; workspaces grow on first use (hipMalloc), so run one warm-up call per shape
 *     before capturing into a hipGraph;
 *   - a context is bound to one device and is not thread-safe (one per device per process);
 *   - re-finalising a weight group (fern_finalize_*) frees its previous device copy and invalidates forks made earlier;
 *   - NO collectives are exported.  SURVEY.md 8b listed fern_comm_init / fern_all_gather; they are deliberately left to
 *     torch.distributed (backend "nccl" = RCCL over xGMI, "gloo" in the CPU tests): the path has exactly one exchange
 *     step -- the all-gather of fused gallery shards -- and the reference side already owns a process group, so a second
 *     communicator inside this library would only duplicate its bootstrap.  The gallery-sharded alternative needs
 *     fern_sim_topk(idx_offset=) + fern_topk_merge from this library and two all-gathers from the caller.
 */
#ifndef FERN_H
#define FERN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FERN_ABI_VERSION 3

#if defined(__GNUC__)
#define FERN_API __attribute__((visibility("default")))
#else
#define FERN_API
#endif

typedef struct fern_ctx fern_ctx;

typedef enum {
    FERN_OK = 0,
    FERN_ERR_ARG = -1,      /* bad argument / unsupported shape */
    FERN_ERR_HIP = -2,      /* HIP runtime error */
    FERN_ERR_STATE = -3,    /* weights missing / not finalised */
    FERN_ERR_NOMEM = -4
} fern_status;

typedef enum { FERN_F32 = 0, FERN_I64 = 1 } fern_dtype;

/* which CombinerSimple / VisualSR instance of ERN (models/model.py:16-20, fusion_model.py:17-24) */
typedef enum {
    FERN_COMBINER_TARGET = 0,      /* ERN.Combiner_module      (model.py:20)  */
    FERN_COMBINER_DVR_GLOBAL = 1,  /* DVR.combiner_global      (fusion_model.py:22) */
    FERN_COMBINER_DVR_LOCAL = 2,   /* DVR.combiner_local       (fusion_model.py:23) */
    FERN_COMBINER_DVR_FINAL = 3    /* DVR.combiner             (fusion_model.py:24) */
} fern_combiner_id;

/* groups of fusion weights that can be finalised independently (a stand-alone CombinerSimple / VisualSR /
 * DVR_module loads its weights under the ERN prefix of the slot it occupies) */
typedef enum {
    FERN_PART_DVR = 1,              /* "DVR.*"              -> fern_dvr_fuse, DVR combiners / SR */
    FERN_PART_TARGET_SR = 2,        /* "SR_module.*"        -> fern_visual_sr(FERN_SR_TARGET) */
    FERN_PART_TARGET_COMBINER = 4,  /* "Combiner_module.*"  -> fern_combiner(FERN_COMBINER_TARGET) */
    FERN_PART_ALL = 7               /* everything ERN owns  -> + fern_index_fuse */
} fern_fusion_part;

/* Operand precision of the CLIP towers' token-level GEMMs (BASELINE.json config 5 names a reduced-precision encoder;
 * SURVEY.md 7 step 6 "perf mode").  FP32 is the parity mode (exact fp32 FMA chains on the fp32 MFMA) and the default.
 * BF16: in every full transformer block of both towers the QKV / out-proj / c_fc / c_proj contractions (and the last ViT
 * block's K/V projection) read activations and weights rounded to bf16 (RNE) and accumulate in fp32, and the attention
 * of those blocks runs in the bf16 operand form (fern_attention_bf16: q/k/v and the un-normalised softmax weights
 * rounded to bf16, fp32 accumulation); the two BERT blocks of the fusion stage (fern_dvr_fuse) follow the same recipe.
 * The residual streams, LayerNorm / softmax statistics, GELU, patch embedding, class-token chain of the last ViT block,
 * final projections, cross attention, VisualSR, the combiners and the ranking path stay fp32.  Rounding points are fixed by the layer structure, not by
 * the batch size, so results remain batch-invariant. */
typedef enum {
    FERN_PREC_FP32 = 0,
    FERN_PREC_BF16 = 1,
    /* BASELINE.json config 5 ("fp8 MFMA encoder path"): as BF16, but the four token-level GEMMs of a block (and the last ViT
     * block's K/V projection) take OCP e4m3fn operands on v_mfma_f32_32x32x16_fp8_fp8: one dynamic scale per token row
     * (max|row| / 448, computed where the row is produced) and one static scale per output channel of the weight, both
     * folded back in the fp32 epilogue; attention, and the fusion stage's BERT blocks, stay in the bf16 operand form (fp8 is
     * for the encoder GEMMs only).  Needs tower / MLP widths % 64 == 0. */
    FERN_PREC_FP8 = 2,
    /* The same block structure with BLOCK-SCALED (MX) fp8 operands on v_mfma_scale_f32_32x32x64_f8f6f4, gfx950's scaled MFMA at
     * twice the bf16 / plain-fp8 matrix rate: one E8M0 (power-of-two) scale per (token, 32 consecutive channels) of the
     * activations and per (output channel, 32 consecutive inputs) of the weights (fern_quantize_mx8), applied inside the MFMA --
     * an outlier channel costs the precision of its own 32-block, not of the whole token row.  The ViT patch embedding runs the same way
     * (patch rows quantised once, conv1 as a block-scaled GEMM) when 3 * patch^2 is a multiple of 128.  Needs tower / MLP widths % 128 == 0. */
    FERN_PREC_MX8 = 3,
    /* fp32 data everywhere (the FP32 mode's buffers, statistics, attention, epilogues), but every plain-epilogue GEMM of 256 rows or
     * more computes its fp32 dot products as "f32x3": both operands split in registers into three bf16 planes (8 + 8 + 8 mantissa bits,
     * by truncation) and the six partial products of total order <= 4 run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  The
     * error against exact arithmetic is the fp32 MFMA kernel's own (~2e-6 of the output rms), at ~1.4-1.5x its speed; it is not the
     * sequential fp32 fma chain, so results are fp32-accurate but not bit-identical to FERN_PREC_FP32 (they are bit-identical across
     * tile shapes and batch sizes).  The ranking stage never uses it: fern_sim_topk* scores stay the exact chain.  No reference
     * counterpart (cuBLAS's own TF32x3-style modes are the closest relative). */
    FERN_PREC_F32X3 = 4,
    /* MX8 for the MLP pair (c_fc + c_proj: two thirds of a block's GEMM flops) of the IMAGE tower, BF16 for LayerNorm-1 / QKV /
     * attention / out-proj and (round 6) for the whole text tower, fp32 residual stream: the fp8 rounding points that remain sit where
     * the flops are (the ViT's 12608-row MLP GEMMs), none on the query's text side; between the two modes in speed and the fastest
     * mode that keeps Recall@50 within 1 pp of the fp32 encoder on bench.py's `reduced_modes` table -- the c5 default since round 6. */
    FERN_PREC_MX8_MLP = 5,
    /* Round 6, the c5 default: block-scaled fp8 (MX8) operands for ALL FOUR token-level GEMMs of the IMAGE tower -- LayerNorm-1 / -2 and
     * the attention kernel write e4m3fn + E8M0 scales, c_fc quantises its GELU output -- over the FP32 residual stream (not MX8's bf16
     * stream), and the bf16 block for the text tower and the fusion BERT.  All of the ViT's GEMM flops at the fp8 MFMA rate; on bench.py's
     * `reduced_modes` table (2 048 queries x 8 192 images) Recall@50 moves by 0.0 pp and the top-50 overlap is 0.942, against -2.7 pp /
     * 0.893 for FERN_PREC_MX8: what costs MX8 its Recall is the text tower's operands (-1.5 pp) and the bf16 residual stream (-1 pp),
     * not the image tower's fp8 GEMMs. */
    FERN_PREC_MX8_IMG = 6
} fern_precision;

typedef enum {
    FERN_SR_TARGET = 0,            /* ERN.SR_module            (model.py:19) */
    FERN_SR_DVR = 1                /* DVR.SR_module            (fusion_model.py:17) */
} fern_sr_id;

/* CLIP tower shapes (open_clip model config) */
typedef struct {
    int embed_dim;
    int image_size, patch_size, v_width, v_layers, v_heads, v_mlp;   /* ViT tower; v_layers == 0: none */
    int context_length, vocab_size, t_width, t_heads, t_layers, t_mlp;
    int v_arch;          /* 0 = ViT (fields above), 1 = open_clip ModifiedResNet (fields below; e.g. RN50x4) */
    int r_layers[4];     /* bottleneck blocks per stage, RN50x4: 4,6,10,6 */
    int r_width;         /* stem / stage-1 width, RN50x4: 80 */
    int r_heads;         /* attention-pool heads, RN50x4: 40 */
} fern_clip_config;

/* GEMM epilogues exposed for tests and for reference-side composition */
typedef enum {
    FERN_EPI_BIAS = 0,          /* C = A W^T + bias (bias may be NULL)            */
    FERN_EPI_BIAS_GELU = 1,     /* exact erf GELU                                 */
    FERN_EPI_BIAS_RELU = 2,
    FERN_EPI_BIAS_RESIDUAL = 3, /* C = A W^T + bias + R  (R has leading dim ldc)  */
    FERN_EPI_BIAS_QUICKGELU = 4 /* v * sigmoid(1.702 v), v = A W^T + bias: accepted wherever FERN_EPI_BIAS_GELU is, the quantising
                                   fern_gemm_mx8_quant included.  One arithmetic for every operand family (each GELU family has its own form) */
} fern_epilogue;

/* MLP activation of the CLIP towers (fern_clip_set_activation) */
typedef enum {
    FERN_ACT_GELU = 0,          /* exact-erf GELU: open_clip's configs built without pretrained weights (the default)                 */
    FERN_ACT_QUICK_GELU = 1     /* x * sigmoid(1.702 x): OpenAI's checkpoints -- open_clip's pretrained="openai", force_quick_gelu and
                                   "*-quickgelu" configs, HF CLIPConfig's default hidden_act="quick_gelu"                              */
} fern_clip_activation;

/* Operand forms the towers' producers write (fern_layernorm_q, fern_im2col_q) */
typedef enum {
    FERN_QFORM_BF16 = 0,        /* bf16, round to nearest even                                          */
    FERN_QFORM_FP8 = 1,         /* e4m3fn with one fp32 scale per row (fern_quantize_rows_fp8's form)   */
    FERN_QFORM_MX8 = 2          /* e4m3fn with one E8M0 byte per 32-element block (fern_quantize_mx8's) */
} fern_qform;

/* kernel-time accounting for bench.py's roofline block */
typedef struct {
    double gemm_ms;        /* every fp32-MFMA GEMM launch: sum over its kernel dispatches of the dispatch's own begin -> end timestamps
                              (hipExtLaunchKernelGGL event pairs = what rocprofv3 --kernel-trace reports per kernel), not stream-marker intervals */
    double gemm_flops;     /* sum of 2*M*N*K of those launches */
    int64_t gemm_launches;
    double attn_ms;        /* attention launches, per-dispatch begin -> end timestamps like gemm_ms */
    double attn_flops;
    int64_t attn_launches;
    double topk_ms;        /* the rest of the ranking stage: sample pass, bound, candidate selection / rescoring, gated exact pass and every
                              launch boundary between them = (the stage's interval) - sweep_ms.  The interval is the stage's first dispatch
                              begin -> last dispatch end (dispatch timestamps, like gemm_ms) for fern_sim_topk_prefiltered and
                              fern_sim_topk_bf16, one stream-marker interval for the plain fern_sim_topk */
    int64_t topk_launches;
    double sweep_ms;       /* the full-gallery similarity sweep inside fern_sim_topk / _bf16 / _prefiltered: the kernel's own duration */
    double sweep_bytes;    /* algorithmic bytes of those sweeps: N*D*s_g + B*D*4 + B*K*8 */
    int64_t sweep_launches;
    double gemm_fp8_ms;    /* fp8-operand GEMM launches (FERN_PREC_FP8, fern_gemm_fp8): not included in gemm_* / gemm_bf16_* */
    double gemm_fp8_flops;
    int64_t gemm_fp8_launches;
    double gemm_bf16_ms;   /* bf16-operand GEMM launches (FERN_PREC_BF16 encoder blocks, fern_gemm_bf16): NOT included in gemm_* */
    double gemm_bf16_flops;
    int64_t gemm_bf16_launches;
    double gemm_alg_bytes; /* algorithmic bytes of the fp32 GEMM launches counted in gemm_*: 4 (M K + N K + M N) each */
    int64_t gemm_dispatches; /* kernel dispatches behind gemm_launches (a bulk + remainder plan is two dispatches per launch) */
    double gemm_mx8_ms;    /* block-scaled fp8 GEMM launches (FERN_PREC_MX8, fern_gemm_mx8): not included in any of the above */
    double gemm_mx8_flops;
    int64_t gemm_mx8_launches;
    double gemm_mx8_bf16_flops; /* the part of gemm_mx8_flops done on the BF16 MFMA: the text tower's GEMMs that ride in the image tower's
                                   block-scaled launches under FERN_PREC_MX8_IMG (fern_encode_pair) -- a roofline of those launches prices
                                   the two parts against their own peaks (ABI 3) */
} fern_prof_stats;

FERN_API int fern_abi_version(void);
FERN_API const char* fern_last_error(void);

/* lifetime ------------------------------------------------------------------------------ */
FERN_API int fern_ctx_create(int device, fern_ctx** out);
/* a second context on the same device that SHARES the parent's finalised weights (no copy) and owns its own workspace:
 * one per extra HIP stream when several batches are kept in flight.  Destroy forks before the parent; re-finalising the
 * parent invalidates them. */
FERN_API int fern_ctx_fork(fern_ctx* parent, fern_ctx** out);
FERN_API int fern_ctx_destroy(fern_ctx* ctx);
FERN_API int fern_sync(fern_ctx* ctx, void* stream);

/* weights: replaces nn.Module.load_state_dict (run/test/test_fiq.py:143,149) ----------------
 * `key` is the reference state-dict key (open_clip names for the CLIP
 * towers).  Data is copied; unknown keys are kept but unused (e.g. pooler, position_ids,
 * num_batches_tracked, logit_scale).  host_ptr is HOST memory. */
FERN_API int fern_load_tensor(fern_ctx* ctx, const char* key, const void* host_ptr, int dtype, int ndim,
                     const int64_t* shape);
/* repack for the kernels (packed QKV, folded BatchNorm, transposed projections) and upload */
FERN_API int fern_finalize_fusion(fern_ctx* ctx, int feature_dim, int parts); /* ERN(clip, feature_dim, device) model.py:8; parts = FERN_PART_* mask */
FERN_API int fern_finalize_clip(fern_ctx* ctx, const fern_clip_config* cfg); /* open_clip.create_model_and_transforms test_fiq.py:141 */
/* The activation of BOTH towers' MLPs, in every precision mode and every encoder entry point (the fusion BERT keeps exact-erf GELU).
 * It belongs to the CLIP weights: fern_finalize_clip returns it to FERN_ACT_GELU, so call this after finalising; contexts forked from
 * `ctx` follow it (call it on the root context, FERN_ERR_ARG on a fork).  FERN_ERR_ARG for any other value and for a NULL ctx.
 * Additive: no field of fern_clip_config changes and FERN_ABI_VERSION stays 3. */
FERN_API int fern_clip_set_activation(fern_ctx* ctx, int act /* fern_clip_activation */);

/* encoders ------------------------------------------------------------------------------ */
/* clip_model.encode_image(images) -- call site utils/utils.py:64, models/clip_model.py:13-15.
 * images [b,3,S,S] f32 NCHW -> out [b,embed_dim], un-normalised. */
FERN_API int fern_vit_encode_image(fern_ctx* ctx, const float* images, float* out, int b, void* stream);
/* clip_model.encode_text(text, mode=, visual_emb=) -- call sites run/test/test_fiq.py:102-103,
 * models/clip_model.py:23-31.  tokens [B,ctx] int64 -> out_global [B,D] (may be NULL) and
 * out_seq [B,ctx,D] (may be NULL); one tower pass serves both (SURVEY.md 8c definition).
 * visual_emb (may be NULL) is the reference's `visual_emb=ref_patch_feats.transpose(0, 1)` argument: a device pointer with
 * visual_emb_shape = HOST int64[3], which must equal {13, B, embed_dim} (FERN_ERR_ARG otherwise); its values are not read
 * (the text encoder that consumes them is unreleased, README.md:41 -- "vanilla CLIP single branch").
 * A token id outside [0, vocab_size) makes the caption's features NaN and is reported as FERN_ERR_ARG by fern_sync or by the
 * next fern_text_encode on the context (nn.Embedding raises in the reference; the launch path here never synchronises). */
FERN_API int fern_text_encode(fern_ctx* ctx, const int64_t* tokens, const float* visual_emb, const int64_t* visual_emb_shape,
                              float* out_global, float* out_seq, int B, void* stream);
/* Both towers of B composed queries in one pass (round 6): `clip_model.encode_image(images)` + `clip_model.encode_text(text)` of the same
 * batch -- the two calls every query batch of the reference's harness and of ERN makes (utils/utils.py:64, run/test/test_fiq.py:102-103,
 * models/clip_model.py:10-31) -- with the towers walked layer by layer so that the text layer's GEMMs ride in the image layer's launches
 * (models/others/modeling_clip.py:694-768 and :832-887 are independent until the fusion).  images [B,3,S,S], tokens [B,ctx] ->
 * out_image [B,D], out_global [B,D] (may be NULL), out_seq [B,ctx,D] (may be NULL).  Results are BIT-IDENTICAL to fern_vit_encode_image +
 * fern_text_encode.  With the ViT tower the launches are paired under FERN_PREC_FP32 (also under F32X3: two fp32-data-flow GEMMs per launch)
 * and under FERN_PREC_MX8_IMG (the image layer's block-scaled GEMM carries the text layer's bf16 GEMM); every other mode / tower simply
 * makes the two calls.  Token-id errors as fern_text_encode. */
FERN_API int fern_encode_pair(fern_ctx* ctx, const float* images, const int64_t* tokens, float* out_image, float* out_global, float* out_seq,
                              int B, void* stream);

/* fusion -------------------------------------------------------------------------------- */
/* ERN.forward(mode="test") = DVR_module.forward -- models/model.py:68-69, fusion_model.py:26-55 */
FERN_API int fern_dvr_fuse(fern_ctx* ctx, const float* ref_global /*[B,D]*/, const float* ref_local /*[B,13,D]*/,
                  const float* text_global /*[B,D]*/, const float* text_seq /*[B,77,D]*/,
                  float* out /*[B,D]*/, int B, int seq_len, void* stream);
/* ERN.forward(mode="index") -- models/model.py:64-66; normalize_input folds the caller's
 * F.normalize(index_features) (run/test/test_fiq.py:45).  Tiles over n internally. */
FERN_API int fern_index_fuse(fern_ctx* ctx, const float* tar_feats /*[n,D]*/, const float* tar_local /*[n,13,D]*/,
                    float* out /*[n,D]*/, int64_t n, int normalize_input, void* stream);
/* CombinerSimple.forward(image_features, text_features) -- fusion_model.py:86-94 */
FERN_API int fern_combiner(fern_ctx* ctx, int which, const float* image /*[n,D]*/, const float* text /*[n,D]*/,
                  float* out /*[n,D]*/, int64_t n, void* stream);
/* VisualSR.forward(local_feature) -- fusion_model.py:141-154 */
FERN_API int fern_visual_sr(fern_ctx* ctx, int which, const float* local /*[n,13,D]*/, float* out /*[n,D]*/,
                   int64_t n, void* stream);
/* Select the encoder precision for the calls that follow on this context (forks inherit the value at fork time).
 * No reference counterpart: the reference evaluates in fp32 only (run/test/test_fiq.py:141-149). */
FERN_API int fern_set_precision(fern_ctx* ctx, int precision /* fern_precision */);
FERN_API int fern_get_precision(fern_ctx* ctx);
/* models/others/Combiner_Model.py:6-70 (CLIP4Cir `Combiner`, not called by the reference's own scripts): weights are loaded
 * under the prefix "clip4cir." with that class's key names; image / text / out are [n, 2*clip_feature_dim]. */
FERN_API int fern_finalize_clip4cir(fern_ctx* ctx);
FERN_API int fern_combiner_clip4cir(fern_ctx* ctx, const float* image, const float* text, float* out, int64_t n, void* stream);
/* losses/loss.py:10-14 BatchBasedClassificationLoss.forward(predicted [B,D], target [B,D]) =
 * cross_entropy(100 * predicted @ target.T, labels = arange(B)), mean over the batch: forward VALUE only (the training
 * loop and its backward are outside this path; ERN's default mode, models/model.py:71-75, produces the two inputs).
 * out_loss: one float on the device.  D % 16 == 0. */
FERN_API int fern_batch_classification_loss(fern_ctx* ctx, const float* predicted, const float* target, int B, int D, float* out_loss,
                                   void* stream);
/* utils.element_wise_sum(image_features, text_features) = F.normalize(image + text) -- utils/utils.py:133-140 */
FERN_API int fern_element_wise_sum(fern_ctx* ctx, const float* image, const float* text, float* out, int64_t n, int d, void* stream);
/* F.normalize(x, dim=-1) -- run/test/test_fiq.py:45 */
FERN_API int fern_l2_normalize(fern_ctx* ctx, const float* x, float* out, int64_t n, int d, void* stream);

/* image side (data formats either side of the path) ----------------------------------------------
 * PIL `Image.resize` on 8-bit RGB, as called by utils/extract_fashioniq_patch.py:142-149 (`resize((360,360), ANTIALIAS)`)
 * and by torchvision `Resize(dim, BICUBIC)` in dataloader/dataset.py:73-87.  One separable pass each; `bounds` [out,2] =
 * (first tap, tap count) and `coeffs` [out,ksize] = fixed-point (2^-22) weights are DEVICE arrays computed by the host
 * exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do.  src is HWC u8 with `src_ld` pixels per row; (x0, y0)
 * is the origin of the region being resampled (`Image.crop`).  Bit-identical to PIL.
 * THREAD SAFETY (the one exception to "a context is not thread-safe"): these three entry points read only `ctx->device`, touch no
 * workspace, tuner or error state of the context beyond the calling thread's last-error slot, and launch on the stream they are
 * given -- dataset transforms may call them from loader worker threads (utils.ThreadedLoader) while another thread encodes. */
FERN_API int fern_resample_u8_horizontal(fern_ctx* ctx, const uint8_t* src, int64_t src_ld, int x0, int y0, int rows, uint8_t* dst /*[rows,ow,3]*/,
                                         int ow, const int32_t* bounds, const int32_t* coeffs, int ksize, void* stream);
FERN_API int fern_resample_u8_vertical(fern_ctx* ctx, const uint8_t* src, int64_t src_ld, int x0, int y0, int cols, uint8_t* dst /*[oh,cols,3]*/,
                                       int oh, const int32_t* bounds, const int32_t* coeffs, int ksize, void* stream);
/* torchvision ToTensor + Normalize (dataloader/dataset.py:84-86) with a crop window: n images [.,src_ld,3] u8, `src_image_stride`
 * bytes apart -> dst [n,3,oh,ow] f32 = (v/255 - mean[c]) / std[c]; mean / std are HOST arrays of 3 floats. */
FERN_API int fern_u8_to_normalized_chw(fern_ctx* ctx, const uint8_t* src, int64_t src_ld, int x0, int y0, int64_t src_image_stride, float* dst,
                                       int n, int oh, int ow, const float* host_mean, const float* host_std, void* stream);

/* rank ---------------------------------------------------------------------------------- */
/* distances = 1 - q @ g.T ; argsort(distances)[:, :K] -- run/test/test_fiq.py:49-50.
 * Scores are cosines (q.g), sorted descending, ties -> lower gallery index.  out_idx holds
 * local row + idx_offset; exclude_idx (may be NULL) [B] removes one global index per query
 * (CIRR reference removal, run/test/test_cirr.py:55-58).  Unfilled slots: score -inf, idx -1.
 * 1 <= K <= 64.  Exact for every gallery: the [B, N] scores are never stored -- a sampled bound filters the sweep into candidate
 * lists -- and a query whose lists overflow is ranked by a capacity-free exact pass inside the same call. */
FERN_API int fern_sim_topk(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D]*/, int B,
                  int64_t N, int D, int K, float* out_scores /*[B,K]*/, int32_t* out_idx /*[B,K]*/,
                  int64_t idx_offset, const int32_t* exclude_idx, void* stream);
/* bf16-gallery variant (BASELINE.json config 5, "bf16 similarity"): `gallery` is [N,D] bf16 produced by fern_gallery_to_bf16
 * (round to nearest even); queries are rounded to bf16 inside the kernel; fp32 accumulation.  HBM-bound stream over the gallery.
 * Cosine scores differ from the fp32 path by <= ~5e-4 (inside north_star's 1e-3); ordering is exact for the rounded operands. */
FERN_API int fern_gallery_to_bf16(fern_ctx* ctx, const float* src, uint16_t* dst, int64_t n, int d, void* stream);
FERN_API int fern_sim_topk_bf16(fern_ctx* ctx, const float* q /*[B,D] f32*/, const uint16_t* gallery /*[N,D] bf16*/, int B, int64_t N, int D,
                                int K, float* out_scores, int32_t* out_idx, int64_t idx_offset, const int32_t* exclude_idx, void* stream);
/* The fp32-gallery ranking stage made HBM-bound: a CERTIFIED bf16 pre-filter + exact fp32 rescoring.  Same contract as fern_sim_topk --
 * `distances = 1 - q @ g.T; argsort` of run/test/test_fiq.py:49-50 on the fp32 gallery: the scores returned are the exact fp32 fma-chain
 * scores fern_sim_topk returns, the ordering is bit-identical to it -- but the pass over the gallery reads a bf16 copy (half the bytes,
 * bf16 MFMA rate), and only the few rows that can still be in the top-K are scored in fp32.
 *   fern_gallery_prepare: once per gallery (the reference builds its index once per evaluation, run/test/test_fiq.py:45-46):
 *       out_bf16 [N, D] = bf16(gallery) (round to nearest even = fern_gallery_to_bf16) and out_meta (DEVICE, 4 floats) =
 *       {max_n ||g_n - bf16(g_n)||, max_n ||bf16(g_n)||, max_n ||g_n||, 0}.  D % 4 == 0.  Re-run after the gallery changes -- or change
 *       its rows in place with fern_gallery_upsert, which keeps out_bf16 and out_meta valid.
 *   fern_sim_topk_prefiltered: per query b, |exact score - bf16 score| <= eps_b = ||q_b|| meta[0] + ||q_b - bf16(q_b)|| meta[1] + slack
 *       for EVERY row (Cauchy-Schwarz; slack = fp32 accumulation of both dot products), so every row of the exact top-K has a bf16
 *       score within 2 eps_b of the K-th best bf16 score: those rows -- K plus the few inside the margin -- are rescored with the exact
 *       chain from `gallery` and ranked.  Nothing about the result depends on the bf16 scores.  Queries whose candidates do not fit
 *       (galleries of near-ties) take fern_sim_topk's exact pass, as there.  D % 64 == 0 and D <= 768 use the pre-filter; other
 *       shapes run fern_sim_topk itself.  `gallery_bf16` / `meta` must come from fern_gallery_prepare on the same `gallery`. */
FERN_API int fern_gallery_prepare(fern_ctx* ctx, const float* gallery /*[N,D]*/, int64_t N, int D, uint16_t* out_bf16 /*[N,D]*/,
                                  float* out_meta /*[4], device*/, void* stream);
FERN_API int fern_sim_topk_prefiltered(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32*/,
                                       const uint16_t* gallery_bf16 /*[N,D]*/, const float* meta /*[4]*/, int B, int64_t N, int D, int K,
                                       float* out_scores /*[B,K]*/, int32_t* out_idx /*[B,K]*/, int64_t idx_offset,
                                       const int32_t* exclude_idx, void* stream);
/* Which form of fern_sim_topk_prefiltered's stage runs on this context (forks inherit at fork time).  Every form returns the same bits;
 * AUTO picks by a cost model of (B, N, D).  A tuning / test knob like fern_tuner_*: no reference counterpart. */
typedef enum {
    FERN_RANK_AUTO = 0,
    FERN_RANK_PLAIN = 1,   /* fern_sim_topk's fp32-MFMA sweep (the pre-filter copy is not read) */
    FERN_RANK_LISTS = 2,   /* bf16 sample pass -> bound - margin -> filtered bf16 sweep into candidate lists -> rescoring: large galleries */
    FERN_RANK_DENSE = 3    /* bf16 sweep storing its [B, N] scores -> one select + rescore kernel; offered while min(B, 1024) * N * 4 bytes of scores stay <= 1.1e9
                            * (~4.3M rows at B <= 64; up to 1.1 GB of workspace per lane) -- the cost model picks it up to ~600k rows at B = 64 */
} fern_rank_strategy;
FERN_API int fern_rank_set_strategy(fern_ctx* ctx, int strategy);
/* The bf16 sweep on its own: scores[b * ld + n] = the fp32-accumulated dot product of bf16(q[b]) and gallery_bf16[n] (v_mfma_f32_32x32x16_bf16,
 * k ascending) for every n < N -- the APPROXIMATE score the pre-filter selects on; tile_max (may be NULL) [B, ldt]: per 32 consecutive
 * gallery rows the largest of those scores (one wave tile of the sweep, reduced across its lanes), which is what the dense form of
 * fern_sim_topk_prefiltered reads instead of the rows.  ld >= N, ldt >= ceil(N / 32) (any such value; elements outside [B, N] /
 * [B, ceil(N / 32)] are not written); D % 64 == 0, D <= 768.  For tests of the
 * certificate (|exact - approximate| <= eps_b) and for callers that want the whole approximate score matrix. */
FERN_API int fern_sweep_bf16_scores(fern_ctx* c, const float* q, const uint16_t* gallery_bf16, int B, int64_t N, int D, float* scores, int64_t ld,
                                    float* tile_max, int64_t ldt, void* stream);
/* Deep ranking: the exact top-K for 1 <= K <= 1024 (the K <= 64 entry points above stop at 64).  Output contract of fern_sim_topk:
 * score descending, then gallery index ascending; idx_offset / exclude_idx as there; unfilled slots -inf / -1 when K > N.  The gallery
 * form follows from the pointers given:
 *   gallery only                      exact: the fp32 fma-chain scores of fern_sim_topk (oracle/chain.c order), whatever fern_set_precision says;
 *   gallery + gallery_bf16 + meta     exact through the certified bf16 pre-filter (fern_gallery_prepare): the same bits as the exact form.
 *                                     Shapes the bf16 sweep does not cover (D % 64 != 0, D > 768) and FERN_RANK_PLAIN run the exact form;
 *   gallery_bf16 only                 bf16 similarity (fern_sim_topk_bf16's contract): the scores fern_sweep_bf16_scores produces, ranked
 *                                     exactly on those values.  Needs D % 64 == 0, D <= 768.
 * For K' <= 64 the first K' columns equal what fern_sim_topk / _prefiltered / _bf16 return for K', bit for bit.  The stage stores the
 * [m, N] scores of a query chunk (m queries within a 1.1 GB workspace), selects per query in LDS and rescores the pre-filter's survivors;
 * a query without room (tie floods) is ranked by a capacity-free exact pass inside the same call, with nothing read back to the host. */
FERN_API int fern_sim_topk_deep(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                                const uint16_t* gallery_bf16 /*[N,D] or NULL*/, const float* meta /*[4] device or NULL*/, int B, int64_t N,
                                int D, int K, float* out_scores /*[B,K]*/, int32_t* out_idx /*[B,K]*/, int64_t idx_offset,
                                const int32_t* exclude_idx, void* stream);
/* Exact target ranks.  The reference ranks with a full argsort of 1 - q @ g.T and looks the target up in it (run/test/test_fiq.py:49-60),
 * so it knows the place of every gallery row; the top-K entry points above know the first K <= 1024 places.  A place is a COUNT -- the
 * number of rows whose ranking key is greater than the target's -- and these two entry points compute it with one more gallery pass and
 * no list: any depth, no capacity, no fallback, nothing read back; asynchronous on `stream` and graph-capturable after one warm-up call.
 * The ranking key is the one the top-K kernels sort, orderable(score) << 32 | ~global_index (score descending, index ascending as one
 * unsigned compare), so a count is the 0-based position of the target in the ordering fern_sim_topk / fern_sim_topk_deep define.
 * Counts are additive over gallery shards: take each target's key from the shard that owns it, count on every shard, add.
 * The gallery form follows from the pointers given, as for fern_sim_topk_deep:
 *   gallery (gallery_bf16 ignored)    the exact fp32 fma-chain scores of fern_sim_topk, whatever fern_set_precision says; D % 32 == 0;
 *   gallery_bf16 only                 the bf16 similarity: the values fern_sweep_bf16_scores produces; D % 64 == 0, D <= 768.
 * fern_rank_keys: out_keys[b][j] = the key of gallery row targets[b][j] - idx_offset for query b, its score bit for bit what the sweep of
 * the same form gives that row; 0 when the target is < 0 or not a row of this gallery (shard). */
FERN_API int fern_rank_keys(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                            const uint16_t* gallery_bf16 /*[N,D] or NULL*/, int B, int64_t N, int D, const int32_t* targets /*[B,m] global indices*/,
                            int m, int64_t idx_offset, uint64_t* out_keys /*[B,m]*/, void* stream);
/* fern_rank_count: out_count[b][j] = the number of rows n < N with key(score(b, n), n + idx_offset) > keys[b][j]; the row exclude_idx[b]
 * (a global index, may be NULL; CIRR's reference removal, run/test/test_cirr.py) is not counted; a key of 0 gives -1.  Any m >= 1: a
 * gallery pass serves 8 targets per query.  Queries are processed in chunks of 1024 (bf16 form: within a 1.1 GB score workspace). */
FERN_API int fern_rank_count(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                             const uint16_t* gallery_bf16 /*[N,D] or NULL*/, int B, int64_t N, int D, const uint64_t* keys /*[B,m]*/, int m,
                             int64_t idx_offset, const int32_t* exclude_idx /*[B] or NULL*/, int32_t* out_count /*[B,m]*/, void* stream);
/* Filtered ranking: per-query gallery row filters.  The reference never ranks against everything it has encoded: it builds one index
 * per FashionIQ category and ranks each query inside its own (run/test/test_fiq.py:157-177), and ranks CIRR's target inside the query's
 * six-member img_set (run/test/test_cirr.py:63-66).  Here the gallery carries one 32-bit tag per row, tags[N] (device), a query carries
 * mask[b] and value[b], and row n is ELIGIBLE for query b iff
 *     (tags[n] & mask[b]) == value[b]
 * mask = value = 0 accepts every row; bit fields give equality on several attributes at once (a live bit, a category field, a group id);
 * a value with bits outside mask matches nothing, which is a valid, empty filter.  The result is the unfiltered exact ranking with the
 * ineligible rows removed: the same score bits, the same order (score descending, global index ascending), idx_offset / exclude_idx as
 * for the unfiltered entry points, unfilled places -inf / -1.  The predicate is applied where scores are produced (ineligible pairs are
 * stored as -inf) and again wherever exact scores are recomputed from the gallery, so an ineligible row is never rescored and never
 * leaves a fallback.  Asynchronous on `stream`, nothing read back, graph-capturable after one warm-up call.
 * fern_sim_topk_filtered: the arguments of fern_sim_topk_deep + the filter; 1 <= K <= 1024; the gallery form follows from the pointers as
 * there (fp32 only, fp32 + bf16 copy + meta, bf16 only), with the same constraints on D.  tags == NULL is an argument error: unfiltered
 * callers keep the entry points above.  Routing (every route returns the same bits):
 *   masked dense form   K <= 64, a prepared gallery (all three pointers), D % 64 == 0, D <= 768, min(B, 1024) * N * 4 bytes of scores
 *                       <= 1.1e9: the bf16 sweep stores masked scores (and masked tile maxima), the dense form's select kernels run on them;
 *   deep stage          everything else: fern_sim_topk_deep's stage on masked score rows.
 * fern_rank_set_strategy: FERN_RANK_PLAIN forces exact fp32 scores (the bf16 copy is not read); FERN_RANK_DENSE forces the masked dense
 * form wherever it is offered (which is also what FERN_RANK_AUTO does); FERN_RANK_LISTS has no filtered form and behaves as AUTO. */
FERN_API int fern_sim_topk_filtered(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                                    const uint16_t* gallery_bf16 /*[N,D] or NULL*/, const float* meta /*[4] device or NULL*/, int B, int64_t N,
                                    int D, int K, float* out_scores /*[B,K]*/, int32_t* out_idx /*[B,K]*/, int64_t idx_offset,
                                    const int32_t* exclude_idx, const uint32_t* tags /*[N]*/, const uint32_t* mask /*[B]*/,
                                    const uint32_t* value /*[B]*/, void* stream);
/* fern_rank_count_filtered: fern_rank_count over the rows that are eligible for each query (the per-category ranks of
 * run/test/test_fiq.py:157-177, the img_set ranks of run/test/test_cirr.py:63-66): the arguments of fern_rank_count + the filter, same
 * predicate; an ineligible row is not counted.  fern_rank_keys needs no filtered form: a row's key does not depend on a filter (whether a
 * TARGET is eligible is the caller's question: a count is returned for any non-zero key). */
FERN_API int fern_rank_count_filtered(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                                      const uint16_t* gallery_bf16 /*[N,D] or NULL*/, int B, int64_t N, int D, const uint64_t* keys /*[B,m]*/,
                                      int m, int64_t idx_offset, const int32_t* exclude_idx /*[B] or NULL*/, int32_t* out_count /*[B,m]*/,
                                      const uint32_t* tags /*[N]*/, const uint32_t* mask /*[B]*/, const uint32_t* value /*[B]*/, void* stream);
/* Candidate ranking: every query ranks inside its OWN list of gallery rows.  The reference ranks CIRR's target inside the query's named
 * member set by the ranking's own scores (run/test/test_cirr.py:55-69); a serving process has such a set whenever a refined query is ranked
 * over the rows an earlier page returned, or a catalogue database answers a request with a list of row ids.  A tag field cannot express a
 * set per query (sets overlap, and there are 32 bits), and fern_gather_scores returns other score bits in no order.
 * Query b ranks the SET of rows named by cand[b][0 .. M) (device, global row indices in the frame of idx_offset, like exclude_idx and
 * rank targets).  An entry takes no place if it is negative, outside [idx_offset, idx_offset + N), equal to exclude_idx[b] or ineligible
 * under the row filter (tags == NULL: unfiltered; otherwise fern_sim_topk_filtered's predicate); a row named more than once counts once.
 * The result is the exact ranking of the whole gallery with every other row removed: the score bits the other entry points return for
 * that (query, row) on that gallery form, the same order (score descending, global index ascending), unfilled places -inf / -1.
 * The gallery form follows from the pointers: `gallery` given: the exact fp32 fma-chain scores in oracle/chain.c order (gallery_bf16 is
 * ignored: a prepared gallery ranks from its fp32 rows, with or without its copy), D % 32 == 0; gallery_bf16 only: the values
 * fern_sweep_bf16_scores produces, D % 64 == 0, D <= 768.
 * Limits: 1 <= M <= 4096, 1 <= K <= 1024 (K may exceed M: the extra places are padded), any B >= 0, N >= 0.  A longer list is a row
 * filter's job (fern_sim_topk_filtered) or a full ranking's.
 * out_place (may be NULL) [B, M]: out_place[b][j] = the 0-based place of entry j in query b's candidate ranking -- the number of distinct
 * place-taking candidates with a greater key -- or -1 if the entry takes no place; duplicates share a place.
 * Asynchronous on `stream`, nothing read back, no workspace, graph-capturable after one warm-up call; one launch per 1024 queries. */
FERN_API int fern_sim_topk_candidates(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                                      const uint16_t* gallery_bf16 /*[N,D] or NULL*/, int B, int64_t N, int D,
                                      const int32_t* cand /*[B,M] device, global indices*/, int M, int K, float* out_scores /*[B,K]*/,
                                      int32_t* out_idx /*[B,K]*/, int32_t* out_place /*[B,M] or NULL*/, int64_t idx_offset,
                                      const int32_t* exclude_idx /*[B] or NULL*/, const uint32_t* tags /*[N] or NULL: unfiltered*/,
                                      const uint32_t* mask /*[B]*/, const uint32_t* value /*[B]*/, void* stream);
/* Ranking pages: the rows at places [offset, offset + K) of a query's ranking, at any depth.  The reference's full argsort of 1 - q @ g.T
 * (run/test/test_fiq.py:49-50) answers two questions about every place: which place a named row holds -- fern_rank_keys + fern_rank_count
 * above -- and which row holds a place, which the top-K entry points answer for places 0 .. 1023 only.  These three answer the second
 * question at any depth, without forming a sorted [B, N] matrix: a radix select over the stored score rows of a query chunk finds the
 * ranking KEY at a place (at most eight passes over a row, every row spread over many workgroups, no capacity, deterministic: each digit is
 * picked from a summed integer histogram), and the deep stage's selection takes a per-query key CEILING: rows whose key is greater take no place.
 * They follow the contract of the ranks and item entry points: asynchronous on `stream`, nothing read back, graph-capturable after one
 * warm-up call; the gallery form follows from the pointers: `gallery` given: the exact fp32 fma-chain scores in oracle/chain.c order
 * (gallery_bf16 is ignored), D % 32 == 0; gallery_bf16 only: the values fern_sweep_bf16_scores produces, D % 64 == 0, D <= 768.  There is no
 * certified pre-filtered form: whether a row's exact key lies at or below a ceiling cannot be decided from an approximate score within
 * eps_b of it.  tags == NULL: unfiltered (mask / value ignored); otherwise fern_sim_topk_filtered's predicate.  idx_offset / exclude_idx
 * as everywhere else; rows scoring -inf, the excluded row and ineligible rows take no place.  Queries are processed in chunks whose [m, N]
 * fp32 score rows stay inside the deep stage's 1.1 GB workspace; a single query that does not fit is an argument error.
 * fern_rank_select: out_keys[b][j] = the ranking key (orderable(score) << 32 | ~global_index) of the row at 0-based place places[b][j] of
 *     query b's ranking; 0 when the place is < 0 or at or past the number of rows that take a place.  The inverse of fern_rank_count: on
 *     finite scores fern_rank_count of a returned key is the place asked for, and the key equals fern_rank_keys of the row at that place
 *     bit for bit.  Any m >= 1: one walk of a row serves 8 places. */
FERN_API int fern_rank_select(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                              const uint16_t* gallery_bf16 /*[N,D] or NULL*/, int B, int64_t N, int D, const int32_t* places /*[B,m]*/, int m,
                              int64_t idx_offset, const int32_t* exclude_idx /*[B] or NULL*/, uint64_t* out_keys /*[B,m]*/,
                              const uint32_t* tags /*[N] or NULL*/, const uint32_t* mask /*[B]*/, const uint32_t* value /*[B]*/, void* stream);
/* fern_sim_topk_from: the exact top-K, 1 <= K <= 1024, among the rows whose ranking key is <= from_keys[b] (device): a result list continued
 *     from a cursor.  A key of 0 makes nothing eligible (every slot -inf / -1); ~0 makes everything eligible, and the result is then
 *     fern_sim_topk_deep's (with tags: fern_sim_topk_filtered's) bit for bit.  The key carries the GLOBAL row index, which need not belong
 *     to this gallery (shard): rows are compared as (orderable(score), ~(n + idx_offset)) against the 64-bit key, the ceiling is never
 *     rebased by idx_offset into 32 bits.  So every shard answers "my best K at or below this key" and fern_topk_merge merges the answers.
 *     The cursor of the page after a result is (the key of its last filled place) - 1: keys are unique per row. */
FERN_API int fern_sim_topk_from(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                                const uint16_t* gallery_bf16 /*[N,D] or NULL*/, int B, int64_t N, int D, int K, const uint64_t* from_keys /*[B]*/,
                                float* out_scores /*[B,K]*/, int32_t* out_idx /*[B,K]*/, int64_t idx_offset, const int32_t* exclude_idx /*[B] or NULL*/,
                                const uint32_t* tags /*[N] or NULL*/, const uint32_t* mask /*[B]*/, const uint32_t* value /*[B]*/, void* stream);
/* fern_sim_topk_page: places [offsets[b], offsets[b] + K) of query b (offsets int32, device; a negative offset counts as 0), 1 <= K <= 1024;
 *     slots past the end of the ranking are -inf / -1.  The fused form: a chunk's score rows are computed once, the select writes the key at
 *     place offsets[b] into workspace and the ceilinged selection runs on the same rows.  offset 0 gives fern_sim_topk_deep's bits. */
FERN_API int fern_sim_topk_page(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                                const uint16_t* gallery_bf16 /*[N,D] or NULL*/, int B, int64_t N, int D, int K, const int32_t* offsets /*[B]*/,
                                float* out_scores /*[B,K]*/, int32_t* out_idx /*[B,K]*/, int64_t idx_offset, const int32_t* exclude_idx /*[B] or NULL*/,
                                const uint32_t* tags /*[N] or NULL*/, const uint32_t* mask /*[B]*/, const uint32_t* value /*[B]*/, void* stream);
/* Item-level ranking: galleries whose rows belong to items.  The reference's galleries are not all made of distinct rows: in Fashion200k
 * the gallery name of an image is its caption (dataloader/fashion200k_patch.py:282-290), index_names holds many duplicates and
 * run/test/test_200k.py:52-60 scores "any row with the target's name"; a product with several photographs is the same case.  Here the
 * gallery carries one int32 item id per row, items[N] (device), and the caller gives the number of items G.  The item-level ranking of
 * query b is the exact row ranking the entry points above define -- score descending, global row index ascending, exclude_idx and the row
 * filter applied first -- with every row that is not the FIRST row of its item removed.  So an item is represented by its best eligible
 * row, an item without an eligible row takes no place, ties between items break by the representatives' global row index (item ids play no
 * part), and a row whose id is outside [0, G) belongs to no item and is ignored.  Exact for any grouping: the stage stores the score rows
 * of a query chunk, reduces them into a [B, G] table of the items' best ranking keys and ranks the representatives with the deep stage.
 * The gallery form follows from the pointers, as for fern_rank_count: `gallery` given: the exact fp32 fma-chain scores (gallery_bf16 is
 * ignored), D % 32 == 0; gallery_bf16 only: the values fern_sweep_bf16_scores produces, D % 64 == 0, D <= 768.  There is no certified
 * pre-filtered form: a group maximum over approximate scores certifies nothing.  tags == NULL: unfiltered (mask / value ignored);
 * otherwise fern_sim_topk_filtered's predicate.  Asynchronous on `stream`, nothing read back, graph-capturable after one warm-up call.
 * Queries are processed in chunks whose [m, N] fp32 score rows plus [m, G] 64-bit table stay inside the deep stage's 1.1 GB workspace;
 * a single query that does not fit is an argument error.
 * fern_sim_topk_items: 1 <= K <= 1024; out_idx = the representative row's global index, out_item = its item id, unfilled places
 * -inf / -1 / -1. */
FERN_API int fern_sim_topk_items(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                                 const uint16_t* gallery_bf16 /*[N,D] or NULL*/, int B, int64_t N, int D, int K, const int32_t* items /*[N]*/, int G,
                                 float* out_scores /*[B,K]*/, int32_t* out_idx /*[B,K]*/, int32_t* out_item /*[B,K]*/, int64_t idx_offset,
                                 const int32_t* exclude_idx /*[B] or NULL*/, const uint32_t* tags /*[N] or NULL*/, const uint32_t* mask /*[B]*/,
                                 const uint32_t* value /*[B]*/, void* stream);
/* fern_item_rank: out_rank[b][j] = the number of items that come before item target_items[b][j] in the ranking above (its 0-based place,
 * any depth: a count over the table, no selection); -1 when the id is outside [0, G) or the item has no eligible row for query b. */
FERN_API int fern_item_rank(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                            const uint16_t* gallery_bf16 /*[N,D] or NULL*/, int B, int64_t N, int D, const int32_t* items /*[N]*/, int G,
                            const int32_t* target_items /*[B,m]*/, int m, int64_t idx_offset, const int32_t* exclude_idx /*[B] or NULL*/,
                            int32_t* out_rank /*[B,m]*/, const uint32_t* tags /*[N] or NULL*/, const uint32_t* mask /*[B]*/,
                            const uint32_t* value /*[B]*/, void* stream);
/* The two halves of fern_item_rank, for galleries sharded so that no item has rows in two shards (fern_rank_keys / fern_rank_count's
 * scheme): fern_item_keys: out_keys[b][j] = the ranking key of item target_items[b][j]'s representative row in this shard (the key holds
 * the GLOBAL row index), 0 when the id is outside [0, G) or no row of this shard can represent it; fern_item_count: out_count[b][j] = the
 * number of this shard's items whose representative's key is greater than keys[b][j], -1 for a key of 0.  Take each target's key from
 * the shard that owns the item (the maximum over the shards), count on every shard, add. */
FERN_API int fern_item_keys(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                            const uint16_t* gallery_bf16 /*[N,D] or NULL*/, int B, int64_t N, int D, const int32_t* items /*[N]*/, int G,
                            const int32_t* target_items /*[B,m]*/, int m, int64_t idx_offset, const int32_t* exclude_idx /*[B] or NULL*/,
                            uint64_t* out_keys /*[B,m]*/, const uint32_t* tags /*[N] or NULL*/, const uint32_t* mask /*[B]*/,
                            const uint32_t* value /*[B]*/, void* stream);
FERN_API int fern_item_count(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D] f32 or NULL*/,
                             const uint16_t* gallery_bf16 /*[N,D] or NULL*/, int B, int64_t N, int D, const int32_t* items /*[N]*/, int G,
                             const uint64_t* keys /*[B,m]*/, int m, int64_t idx_offset, const int32_t* exclude_idx /*[B] or NULL*/,
                             int32_t* out_count /*[B,m]*/, const uint32_t* tags /*[N] or NULL*/, const uint32_t* mask /*[B]*/,
                             const uint32_t* value /*[B]*/, void* stream);
/* Live gallery: change rows of a gallery store in place.  The reference builds its index once per evaluation (run/test/test_fiq.py:45-46)
 * and never changes it; a serving process keeps one [capacity, D] store for its lifetime -- fp32 rows, their bf16 copy and its three norms
 * (fern_gallery_prepare), one tag and one item id per row -- while its catalogue changes a few hundred rows at a time.  These three entry
 * points write chosen SLOTS (row indices in [0, capacity)) of that store without a pass over the rows that stay; the addresses and shapes
 * of the store never change, so hipGraphs captured against it stay valid.  Which slots are in use is the caller's bookkeeping (the Python
 * layer's SlotTable); a free or withdrawn slot is hidden from the ranking by a "live" bit in its tag (fern_sim_topk_filtered).
 * fern_gallery_upsert, for each p < m: row = rows[p * ld .. + D), optionally x / max(||x||, 1e-12) (`normalize`: the F.normalize of
 *     run/test/test_fiq.py:45, fern_l2_normalize's arithmetic bit for bit; needs D <= 1280 like it); then gallery[slots[p]] = row,
 *     gallery_bf16[slots[p]] = bf16(row) (round to nearest even) and meta[0..2] = max(meta[0..2], {||row - bf16(row)||, ||bf16(row)||,
 *     ||row||}).  A row's bits and norms are computed by the device code of fern_gallery_prepare, so upserting every row of a gallery into a
 *     zeroed store with zeroed meta gives that function's output byte for byte, and normalize = 1 equals fern_l2_normalize followed by
 *     normalize = 0.  meta is NOT reset: a maximum that is only ever raised remains an upper bound over the rows present, which is all the
 *     certificate of fern_sim_topk_prefiltered needs (results stay exact; fern_gallery_prepare over the store makes the bound tight again
 *     after many replacements).  NaN / inf rows poison meta upwards, as there.  The gallery form follows from the pointers, as everywhere:
 *     gallery + gallery_bf16 + meta (prepared), gallery only, gallery_bf16 only (the bf16-similarity store).  FERN_ERR_ARG: meta without
 *     both arrays, neither array, ld < D, ld % 4 != 0, D % 4 != 0.  m == 0 succeeds and launches nothing.
 *     Duplicate slots within one call are the caller's error: the contents of a duplicated slot are then undefined (its forms may come from
 *     different rows) and a prepared store must be re-prepared.
 * fern_gallery_move: gallery[dst[p]] = gallery[src[p]], and the same for whichever of gallery_bf16, tags, items are given (at least one of
 *     gallery / gallery_bf16) -- compaction.  The index sets src and dst must be DISJOINT and dst free of duplicates.  meta is untouched: a
 *     move changes no norm.
 * fern_scatter_u32: dst[slots[p]] = src[p] -- tags and, as bits, item ids of upserted rows.
 * Slots (src / dst of a move included) outside [0, capacity): that position writes nothing, the other positions of the call are written,
 *     and FERN_ERR_ARG naming the entry point and the position is reported by fern_sync and by the next call of one of these three entry
 *     points on the context (a host-mapped flag, as for fern_text_encode's token ids: a bounds check, not a fault path).
 * ORDERING CONTRACT.  All three are asynchronous on `stream`, read nothing back and are graph-capturable.  A ranking call that reads the
 *     store must be stream-ordered AFTER the update that wrote it, and an update must be stream-ordered after every ranking call still
 *     reading the store: a sweep that overlaps an upsert can see a new fp32 row next to its old bf16 copy, and no certificate covers that.
 *     Updates racing with sweeps are forbidden, not made safe. */
FERN_API int fern_gallery_upsert(fern_ctx* ctx, const float* rows /*[m, ld], ld >= D*/, int64_t ld, const int32_t* slots /*[m] device*/, int m,
                                 float* gallery /*[capacity, D] or NULL*/, uint16_t* gallery_bf16 /*[capacity, D] or NULL*/,
                                 float* meta /*[4] device or NULL*/, int64_t capacity, int D, int normalize, void* stream);
FERN_API int fern_gallery_move(fern_ctx* ctx, const int32_t* src /*[m]*/, const int32_t* dst /*[m]*/, int m, float* gallery, uint16_t* gallery_bf16,
                               uint32_t* tags /*[capacity] or NULL*/, int32_t* items /*[capacity] or NULL*/, int64_t capacity, int D, void* stream);
FERN_API int fern_scatter_u32(fern_ctx* ctx, const uint32_t* src /*[m]*/, const int32_t* slots /*[m]*/, int m, uint32_t* dst /*[capacity]*/,
                              int64_t capacity, void* stream);
/* scores of explicitly named gallery rows (CIRR subset ranking, run/test/test_cirr.py:64-66);
 * idx < 0 -> -inf */
FERN_API int fern_gather_scores(fern_ctx* ctx, const float* q /*[B,D]*/, const float* gallery /*[N,D]*/,
                       const int32_t* idx /*[B,m]*/, float* out /*[B,m]*/, int B, int m, int D,
                       void* stream);
/* merge R per-shard top-K lists (gallery sharded over R GPUs; SURVEY.md 8e alternative); 1 <= K <= 1024, R * K <= 16384 when K > 64 */
FERN_API int fern_topk_merge(fern_ctx* ctx, const float* scores /*[R,B,K]*/, const int32_t* idx /*[R,B,K]*/,
                    float* out_scores /*[B,K]*/, int32_t* out_idx /*[B,K]*/, int R, int B, int K,
                    void* stream);

/* building blocks (exported for kernel-level parity tests) -------------------------------- */
/* Leading dimensions, for every entry point of this section that takes one (pinned by tests/test_gpu_frames.py): ld >= width
 * (lda, ldw >= K; ldc >= N; ldq, ldk, ldv, ldo >= heads * head_dim; ldx, ldy >= d; FERN_ERR_ARG otherwise: rows would overlap and
 * stores race), and elements outside [rows, width] are neither read into the result nor written -- the gap columns width .. ld of
 * every row, the rows before the first and after the last, bias / scale entries past N or M, scale bytes of rows >= `rows`.  The
 * same holds for the [B, K] outputs of the ranking entry points above: nothing before row 0 or after row B - 1 is written.
 * C[M,N] = A[M,K] W[N,K]^T (+ epilogue); fp32 MFMA.  K % 32 == 0, lda/ldw % 4 == 0, lda >= K, ldw >= K, ldc >= N (any ldc >= N;
 * `residual` shares ldc and may be C itself). */
FERN_API int fern_gemm(fern_ctx* ctx, const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
              const float* residual, float* C, int64_t ldc, int M, int N, int K, int epilogue,
              void* stream);
/* bf16 operand form of fern_gemm ("perf mode" of the encoder GEMMs): A [M,lda] and W [N,ldw] hold bf16
 * bit patterns (fern_gallery_to_bf16 converts any fp32 buffer, round to nearest even), products accumulate in fp32 on
 * v_mfma_f32_32x32x16_bf16; C is fp32, or bf16 when out_bf16 != 0 (not with the residual epilogue).  K % 32 == 0,
 * lda/ldw % 8 == 0, lda >= K, ldw >= K, ldc >= N (any ldc >= N, odd ones included: bf16 rows may be 2-byte aligned); elements outside
 * [rows, width] are neither read into the result nor written. */
FERN_API int fern_gemm_bf16(fern_ctx* ctx, const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, const float* bias,
                   const float* residual, void* C, int64_t ldc, int M, int N, int K, int epilogue, int out_bf16,
                   void* stream);
/* fp8 (OCP e4m3fn) operand form: A [M,lda] / W [N,ldw] bytes with per-row scales (fern_quantize_rows_fp8 produces both:
 * scale[r] = max|row r| / 448, or 1 for a zero row; y = fp8(x / scale[r]), round to nearest even);
 * C = (sum_k A8 W8) * scale_a[row] * scale_w[col] + bias (+ GELU | + residual), fp32 accumulation on
 * v_mfma_f32_32x32x16_fp8_fp8.  K % 64 == 0, lda/ldw % 16 == 0; `x` of the quantiser is bf16 when x_is_bf16 else fp32,
 * d % 8 == 0, d <= 4096, ldx / ldy % 8 == 0.  lda >= K, ldw >= K, ldc >= N, ldx >= d, ldy >= d; elements outside [rows, width] --
 * scale_a[row >= M] and scale_w[col >= N] included -- are neither read into the result nor written. */
FERN_API int fern_quantize_rows_fp8(fern_ctx* ctx, const void* x, int x_is_bf16, int64_t ldx, uint8_t* y, int64_t ldy, float* scale,
                           int64_t rows, int d, void* stream);
FERN_API int fern_gemm_fp8(fern_ctx* ctx, const uint8_t* A, int64_t lda, const float* scale_a, const uint8_t* W, int64_t ldw,
                  const float* scale_w, const float* bias, const float* residual, void* C, int64_t ldc, int M, int N, int K,
                  int epilogue, int out_bf16, void* stream);
/* MX (block-scaled) fp8 operand form, the operand format of gfx950's v_mfma_scale_f32_32x32x64_f8f6f4 (twice the bf16 / plain-fp8
 * matrix rate): OCP e4m3fn bytes with ONE E8M0 scale byte per (row, 32 consecutive k).  fern_quantize_mx8 produces both from a
 * bf16 or fp32 [rows, d] matrix: e = the smallest power-of-two exponent with max|block| * 2^-(e-127) <= 448 (clamped to [1, 253];
 * an all-zero block gets 1), y = fp8(x * 2^(127-e)) -- the scaling is exact, the cast rounds to nearest even.
 * Scale layout (uint8, (d / 128) * scale_rows * 4 bytes): byte of (row r, block b = k / 32) at ((b / 4) * scale_rows + r) * 4 + b % 4,
 * scale_rows >= rows.  fern_gemm_mx8: C = sum over blocks of 2^(ea-127) 2^(ew-127) (A8 . W8) + bias (+ GELU | + residual), fp32
 * accumulation, scales applied inside the MFMA.  K % 128 == 0, d % 128 == 0, d <= 4096, lda / ldw % 16 == 0, ldx / ldy % 8 == 0.
 * FERN_EPI_BIAS_RESIDUAL with out_bf16 != 0 is the bf16 RESIDUAL-STREAM form (FERN_PREC_MX8's token stream): `residual` then points
 * at bf16 [M, ldc] (may alias C) and C = bf16(sum + bias + float(residual)), one round-to-nearest-even per element.
 * lda >= K, ldw >= K, ldc >= N, ldx >= d, ldy >= d; elements outside [rows, width] -- scale bytes of rows >= `rows` included -- are
 * neither read into the result nor written. */
FERN_API int fern_quantize_mx8(fern_ctx* ctx, const void* x, int x_is_bf16, int64_t ldx, uint8_t* y, int64_t ldy, uint8_t* scales,
                      int64_t scale_rows, int64_t rows, int d, void* stream);
FERN_API int fern_gemm_mx8(fern_ctx* ctx, const uint8_t* A, int64_t lda, const uint8_t* scales_a, int64_t scale_rows_a, const uint8_t* W,
                  int64_t ldw, const uint8_t* scales_w, int64_t scale_rows_w, const float* bias, const float* residual, void* C,
                  int64_t ldc, int M, int N, int K, int epilogue, int out_bf16, void* stream);
/* fern_gemm_mx8 whose output is quantised where it is produced: C8 [M, ldc] e4m3fn bytes + scales_c (the layout above, scale_rows_c
 * rows) = fern_quantize_mx8 applied to the fp32 values bias + sum (+ GELU), bit for bit -- the A operand of the next
 * fern_gemm_mx8.  N % 128 == 0, ldc % 16 == 0, ldc >= N (lda, ldw >= K); epilogue BIAS, BIAS_GELU or BIAS_QUICKGELU.  Bytes of C8 outside
 * [M, N] and scale bytes of rows >= M are not written. */
FERN_API int fern_gemm_mx8_quant(fern_ctx* ctx, const uint8_t* A, int64_t lda, const uint8_t* scales_a, int64_t scale_rows_a, const uint8_t* W,
                        int64_t ldw, const uint8_t* scales_w, int64_t scale_rows_w, const float* bias, uint8_t* C8, int64_t ldc,
                        uint8_t* scales_c, int64_t scale_rows_c, int M, int N, int K, int epilogue, void* stream);
/* y = LayerNorm(x (+ residual)) * gamma + beta, rows of width d */
FERN_API int fern_layernorm(fern_ctx* ctx, const float* x, const float* residual, const float* gamma,
                   const float* beta, float* y, int64_t rows, int d, float eps, void* stream);
/* softmax(scale * Q K^T (+causal)) V per (batch, head); q/k/v row strides in floats.  head_dim % 4 == 0, <= 96; s_q and s_k are
 * independent when not causal, s_k <= 4096 (up to 224 keys K / V stay resident in LDS, beyond that they stream through it in chunks of 128
 * keys: the same arithmetic per (query, key) in the same order); causal: s_q == s_k <= 96.  ldq, ldk, ldv, ldo % 4 == 0 and
 * >= heads * head_dim (q, k, v may be column slices of one packed [rows, 3 W] buffer); elements outside [rows, heads * head_dim] --
 * K / V rows past s_k of the last batch included -- are neither read into the result nor written. */
FERN_API int fern_attention(fern_ctx* ctx, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                   int64_t ldv, float* out, int64_t ldo, int batch, int heads, int head_dim, int s_q,
                   int s_k, int causal, float scale, void* stream);
/* Attention of ONE query per (image, head) over tokens whose keys and values are NOT projected: what the last ViT block (class token)
 * and the ModifiedResNet's attention pool run in the fp32 data flow.  With E = heads * head_dim:
 *   out[b, h hd + d] = bv[h hd + d] + Wv[h hd + d, :] . sum_j p_j t[b, j, :],   p = softmax_j((Wk_h^T q[b, h]) . t[b, j, :] / sqrt(hd))
 * which equals softmax(q (t Wk^T + bk)^T / sqrt(hd)) (t Wv^T + bv) for every key bias bk (a constant per softmax), so none is taken.
 * q [batch, E] is the projected query, its bias included; tokens [batch, s, E] with row stride ldt and image stride image_stride
 * (floats); wk, wv [E, E] are the key and value rows of the in-proj weight in their [out, in] layout, leading dimension E; bv [E];
 * out [batch, E].  head_dim % 4 == 0, <= 128; E <= 4096; 1 <= s <= 1024; ldq, ldt, ldo >= E, every stride % 4 == 0, pointers 16-byte
 * aligned.  Every sum has one order that depends on (s, E, heads) alone: a row's bits do not depend on the batch around it.  The
 * scratch is a fresh workspace frame of ctx; no host synchronisation. */
FERN_API int fern_pooled_attention(fern_ctx* ctx, const float* q, int64_t ldq, const float* tokens, int64_t ldt, int64_t image_stride,
                   const float* wk, const float* wv, const float* bv, float* out, int64_t ldo, int batch, int heads,
                   int head_dim, int s, void* stream);
/* bf16 operand form (perf mode of the CLIP towers): q/k/v/out hold bf16 bit patterns (strides in elements, % 8 == 0);
 * QK^T and PV on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, `scale` applied to the fp32 scores, softmax statistics
 * in fp32, the un-normalised weights rounded to bf16 for the PV product.  head_dim % 8 == 0, <= 96; s_k <= 4096 (causal: <= 96),
 * resident up to 224 keys and key-streaming beyond, as fern_attention.  Every ld >= heads * head_dim; elements outside
 * [rows, heads * head_dim] are neither read into the result nor written. */
FERN_API int fern_attention_bf16(fern_ctx* ctx, const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v,
                        int64_t ldv, uint16_t* out, int64_t ldo, int batch, int heads, int head_dim, int s_q, int s_k,
                        int causal, float scale, void* stream);
/* The producers that fuse a quantiser into another kernel, reached through the launchers the towers call, so that the dispatch under
 * test is the production dispatch.  Arguments are validated before any HIP call.
 * fern_layernorm_q: LayerNorm (eps, fp32 statistics) of rows [rows, d] read with stride ldx, written in `out_form` with stride ldy.
 *   FERN_QFORM_BF16 / _FP8: x is fp32 (x_is_bf16 == 0), d % 4 == 0, d <= 1280; FP8: `scales` is float [rows] (max|y| / 448).
 *   FERN_QFORM_MX8: x is fp32 or bf16 (x_is_bf16), d % 128 == 0, d <= 1280, `scales` uint8 in fern_quantize_mx8's layout with
 *   scale_rows >= rows rows (bytes of rows >= `rows` are not written).  ldx / ldy % 4 == 0, >= d; x, gamma, beta, y and scales
 *   16-byte aligned.  The launcher picks the kernel from the width, the strides and the alignment, as in the towers.
 * fern_attention_mx8: fern_attention_bf16 whose output is e4m3fn bytes [batch * s_q, ldo] + E8M0 scales per 32 output columns
 *   (fern_quantize_mx8's layout, scale_rows >= batch * s_q rows), quantised from the kernel's fp32 output values -- the MX operand of
 *   the out-projection in FERN_PREC_MX8 / _MX8_IMG.  head_dim % 32 == 0, heads * head_dim % 128 == 0, ldo % 16 == 0.
 *   s_k <= 4096 (causal: <= 96); the key-streaming form past 224 keys stores the same way.
 * fern_im2col_q: the patch rows of [b, 3, img, img] fp32 images, row (image, gy, gx) = 3 x patch x patch pixels in (channel, y, x)
 *   order, as FERN_QFORM_BF16 ([rows, d] uint16) or FERN_QFORM_MX8 ([rows, d] bytes + scales with scale_rows >= rows rows), with
 *   rows = b * (img / patch)^2 and d = 3 * patch^2: the patch embedding's A operand.  patch % 4 == 0, img % patch == 0, d <= 1280;
 *   d % 32 == 0 (BF16) or d % 128 == 0 (MX8). */
FERN_API int fern_layernorm_q(fern_ctx* ctx, const void* x, int x_is_bf16, int64_t ldx, const float* gamma, const float* beta, int out_form,
                     void* y, int64_t ldy, void* scales, int64_t scale_rows, int64_t rows, int d, float eps, void* stream);
FERN_API int fern_attention_mx8(fern_ctx* ctx, const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v,
                       int64_t ldv, uint8_t* out, int64_t ldo, uint8_t* scales, int64_t scale_rows, int batch, int heads,
                       int head_dim, int s_q, int s_k, int causal, float scale, void* stream);
FERN_API int fern_im2col_q(fern_ctx* ctx, const float* images, int b, int img, int patch, int out_form, void* y, void* scales,
                  int64_t scale_rows, void* stream);
/* The kernels of the open_clip ModifiedResNet image tower (RN50x4), each behind the launcher the tower calls with the descriptor the
 * tower builds, so that tile choice, tuner and forced configurations are the tower's own.  Activations are NHWC fp32 with the channel
 * count as the row stride; BatchNorm is whatever the caller folded into w / bias.  Arguments are validated before any HIP call;
 * b == 0 (M == 0) returns FERN_OK without a launch.
 * fern_conv3x3_nhwc: out [b,H,W,cout] = relu(conv3x3(x [b,H,W,cin], stride 1, zero padding 1) + bias), w [cout, 9 * cin] with
 *   k = (ky * 3 + kx) * cin + c: the fp32 GEMM over the b * H * W pixel rows with the 3x3-window LDS-DMA loader (taps outside the
 *   image come from a zeroed piece of a fresh workspace frame of ctx).  cin % 16 == 0, b * H * W < 2^31, x and w 16-byte aligned.
 * fern_conv1x1_nhwc: out [M,cout] = x [M,cin] w [cout,cin]^T + bias, then relu when `relu`, and relu(. + residual [M,cout]) when a
 *   residual is given (the bottleneck's closing convolution; `relu` must then be set): the fp32 GEMM over pixel rows with the
 *   tower's three epilogues.  cin % 16 == 0, x and w 16-byte aligned.
 * fern_stem_conv: out [b,S/2,S/2,cout_pad] (NHWC) = relu(conv3x3(images [b,3,S,S] NCHW, stride 2, zero padding 1) + bias),
 *   w [cout_pad, 27] with k = (c * 3 + ky) * 3 + kx.  S % 2 == 0, cout_pad % 4 == 0 (48 runs the one-thread-per-pixel kernel, bit
 *   identical per channel to the other); bias and out 16-byte aligned.
 * fern_avgpool_nhwc: y [b,H/k,W/k,C] = the mean over k x k windows of x [b,H,W,C] (stride k).  C % 4 == 0, H % k == 0, W % k == 0,
 *   pointers 16-byte aligned.
 * fern_attnpool_tokens: the attention pool's token rows, T [b,HW+1,C]: T[i,0] = mean_j x[i,j] + pos[0], T[i,j+1] = x[i,j] + pos[j+1]
 *   for x [b,HW,C], pos [HW+1,C]; T0 [b,C] = T[:,0] (the compact query rows).  HW >= 1, C % 4 == 0, pointers 16-byte aligned; the
 *   [b,C] means go through a fresh workspace frame of ctx. */
FERN_API int fern_conv3x3_nhwc(fern_ctx* ctx, const float* x, const float* w, const float* bias, float* out, int b, int H, int W, int cin,
                      int cout, void* stream);
FERN_API int fern_conv1x1_nhwc(fern_ctx* ctx, const float* x, const float* w, const float* bias, const float* residual, float* out, int M,
                      int cin, int cout, int relu, void* stream);
FERN_API int fern_stem_conv(fern_ctx* ctx, const float* images, const float* w, const float* bias, float* out, int b, int S, int cout_pad,
                   void* stream);
FERN_API int fern_avgpool_nhwc(fern_ctx* ctx, const float* x, float* y, int b, int H, int W, int C, int k, void* stream);
FERN_API int fern_attnpool_tokens(fern_ctx* ctx, const float* x, const float* pos, float* T, float* T0, int b, int HW, int C, void* stream);

/* The GEMM launchers time their tile candidates once per new shape (all candidates are bit-identical).  This
 * returns the choices made so far in this process as text, one line per shape ("f32|bf16|fp8 M N K epilogue loader cfg");
 * the return value is the full length.  Setting FERN_GEMM_TILES=<file of such lines> before the first launch pins those
 * shapes (no timing runs, same kernels on every box).  No reference counterpart (cuBLAS picks its own kernels). */
FERN_API int64_t fern_tuner_export(char* buf, int64_t cap);
/* The reverse: `text` (NUL-terminated lines of the export format) replaces this process's choices for the shapes it lists, e.g.
 * rank 0's export broadcast to all ranks of a job so that every rank runs the same kernels (the step time of a multi-GPU job is
 * the max over ranks).  Lines that do not parse or name an inapplicable configuration are skipped.  Never changes a result. */
FERN_API int fern_tuner_import(const char* text);
/* The number of batches the caller keeps in flight on separate streams (the query pipeline's lanes; process-wide, default 1).
 * With more than one, the bf16 / fp8 / block-scaled GEMM families score a tile trial by duration x (share of the chip's
 * workgroup slots the launch fills)^0.75 instead of duration alone: a launch that leaves CUs to the other streams' kernels is worth more
 * to the pipeline than its own latency says.  Call before the first launch of a shape; tuned shapes keep their
 * choice.  The fp32 family is not affected.  Never changes a result.  No reference counterpart. */
FERN_API int fern_tuner_set_concurrency(int lanes);
/* Force ONE tile configuration of a GEMM family ("f32", "f32x3", "bf16", "fp8", "mx8"), process-wide, until cfg < 0 releases it (the
 * value of FERN_GEMM_CFG / _SPLIT_CFG / _BF16_CFG / _FP8_CFG / _MX8_CFG then applies again).  Every configuration of a family returns the
 * same bits, so this never changes a result: it exists so that one test process can walk all variants. */
FERN_API int fern_tuner_force_config(const char* family, int cfg);

/* Workspace generation of a context: incremented each time the context frees workspace memory it had handed to kernels before
 * (it consolidates its arena at the start of the next call after one that had to grow it).  A hipGraph captured from calls on
 * this context holds those addresses: re-capture it when the value differs from the one read right after the capture. */
FERN_API uint64_t fern_ws_generation(const fern_ctx* ctx);

/* profiling ----------------------------------------------------------------------------- */
/* While on, GEMM / attention / sweep launches are dispatched with a (start, stop) event pair each and timed by the dispatch's own begin /
 * end timestamps; the ranking STAGE (sample, bound, sweep, select, exact gate and the boundaries between them) is, for
 * fern_sim_topk_prefiltered / fern_sim_topk_bf16, the span first dispatch begin -> last dispatch end from those same timestamps, and for the
 * plain fern_sim_topk one stream-marker interval.  A launch that fails while instrumented leaves no record behind. */
FERN_API int fern_prof_enable(fern_ctx* ctx, int on);
FERN_API int fern_prof_collect(fern_ctx* ctx, fern_prof_stats* out);  /* synchronises, sums, resets */

#ifdef __cplusplus
}
#endif
#endif /* FERN_H */

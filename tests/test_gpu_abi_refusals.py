"""The refusals of the public building blocks (include/fern.h: fern_gemm*, fern_quantize_*, fern_attention*, fern_layernorm_q,
fern_im2col_q), pinned: which check answers, with which return code and which exact fern_last_error() text, and which check answers
first where two apply.  The texts are the library's as they stood before these entries moved into a file of their own with one
shared check per family; a refactor of that layer must leave every row as it is.

Every check tests the context first, so the rows need a real one; nothing is launched and no pointer is dereferenced: a row is a
refusal, or a call that returns FERN_OK before it looks at its operands (M == 0, rows == 0, b == 0)."""
import pytest

pytestmark = pytest.mark.gpu

P = 0x10000          # a "device pointer": 16-byte aligned, never dereferenced
ODD = P + 8          # ... and one that is not 16-byte aligned
ERR = -1             # FERN_ERR_ARG
BIAS, GELU, RELU, RESIDUAL, QUICKGELU = 0, 1, 2, 3, 4      # fern_epilogue
BF16, FP8, MX8 = 0, 1, 2                                    # fern_qform

# entry -> its parameters after ctx, in order, with the values of a call that every check accepts
ENTRIES = {
    "fern_gemm": dict(A=P, lda=32, W=P, ldw=32, bias=0, residual=0, C=P, ldc=8, M=4, N=8, K=32, epilogue=BIAS, stream=0),
    "fern_gemm_bf16": dict(A=P, lda=32, W=P, ldw=32, bias=0, residual=0, C=P, ldc=8, M=4, N=8, K=32, epilogue=BIAS, out_bf16=0, stream=0),
    "fern_gemm_fp8": dict(A=P, lda=64, scale_a=P, W=P, ldw=64, scale_w=P, bias=0, residual=0, C=P, ldc=8, M=4, N=8, K=64, epilogue=BIAS,
                          out_bf16=0, stream=0),
    "fern_gemm_mx8": dict(A=P, lda=128, scales_a=P, scale_rows_a=4, W=P, ldw=128, scales_w=P, scale_rows_w=8, bias=0, residual=0, C=P, ldc=8,
                          M=4, N=8, K=128, epilogue=BIAS, out_bf16=0, stream=0),
    "fern_gemm_mx8_quant": dict(A=P, lda=128, scales_a=P, scale_rows_a=4, W=P, ldw=128, scales_w=P, scale_rows_w=128, bias=0, C8=P, ldc=128,
                                scales_c=P, scale_rows_c=4, M=4, N=128, K=128, epilogue=BIAS, stream=0),
    "fern_quantize_rows_fp8": dict(x=P, x_is_bf16=0, ldx=128, y=P, ldy=128, scale=P, rows=4, d=128, stream=0),
    "fern_quantize_mx8": dict(x=P, x_is_bf16=0, ldx=128, y=P, ldy=128, scales=P, scale_rows=4, rows=4, d=128, stream=0),
    "fern_attention": dict(q=P, ldq=8, k=P, ldk=8, v=P, ldv=8, out=P, ldo=8, batch=1, heads=2, head_dim=4, s_q=5, s_k=5, causal=0, scale=0.5,
                           stream=0),
    "fern_attention_bf16": dict(q=P, ldq=8, k=P, ldk=8, v=P, ldv=8, out=P, ldo=8, batch=1, heads=2, head_dim=4, s_q=5, s_k=5, causal=0,
                                scale=0.5, stream=0),
    "fern_attention_mx8": dict(q=P, ldq=128, k=P, ldk=128, v=P, ldv=128, out=P, ldo=128, scales=P, scale_rows=5, batch=1, heads=4, head_dim=32,
                               s_q=5, s_k=5, causal=0, scale=0.5, stream=0),
    "fern_layernorm_q": dict(x=P, x_is_bf16=0, ldx=128, gamma=P, beta=P, out_form=MX8, y=P, ldy=128, scales=P, scale_rows=4, rows=4, d=128,
                             eps=1e-5, stream=0),
    "fern_im2col_q": dict(images=P, b=1, img=32, patch=16, out_form=MX8, y=P, scales=P, scale_rows=4, stream=0),
}

LD_TEXT = "need lda >= K, ldw >= K, ldc >= N (rows must not overlap)"
LIST4 = "epilogue must be BIAS, BIAS_GELU, BIAS_QUICKGELU or BIAS_RESIDUAL"
ATTN_LD = "need ldq, ldk, ldv, ldo >= heads * head_dim (rows must not overlap)"
MXA_SHAPE = "need head_dim % 32 == 0, head_dim <= 96, heads * head_dim % 128 == 0"
MXA_LD = "need ldq / ldk / ldv % 8 == 0, ldo % 16 == 0, ld >= heads * head_dim, scale_rows >= batch * s_q"
LNQ_SHAPE = "need d % 4 == 0, d <= 1280, ld % 4 == 0, ld >= d"
IM2COL_SHAPE = "need patch % 4 == 0, img % patch == 0, 3 * patch^2 <= 1280 and % 32 (BF16) / % 128 (MX8) == 0"
ALIGN = "pointers must be 16-byte aligned"
NOCTX = dict(ctx=None)

# (entry, what differs from the accepted call, return code, the text after "<entry>: " or None where FERN_OK leaves the text alone)
ROWS = []


def rows(entry, *cases):
    ROWS.extend((entry, over, code, text) for over, code, text in cases)


# ---- the five GEMM entries: context and sizes, M == 0 || N == 0, operands, epilogue, residual, multiples, leading dimensions ----------
for name, null_operand, k_bad, k_text, ld_odd in [
        ("fern_gemm", "W", 33, "K must be a multiple of 32", None),
        ("fern_gemm_bf16", "W", 48, "K % 32, lda % 8 and ldw % 8 must be 0", 36),
        ("fern_gemm_fp8", "scale_w", 96, "K % 64, lda % 16 and ldw % 16 must be 0", 72),
        ("fern_gemm_mx8", "scales_a", 192, "K % 128, lda % 16 and ldw % 16 must be 0, scale_rows >= rows", 136),
        ("fern_gemm_mx8_quant", "scales_c", 192, "K % 128, N % 128, lda / ldw / ldc % 16 must be 0, scale_rows >= rows", 136)]:
    out = "C8" if name == "fern_gemm_mx8_quant" else "C"
    k = ENTRIES[name]["K"]
    rows(name,
         (NOCTX, ERR, "bad argument"),
         (dict(M=-1), ERR, "bad argument"),
         (dict(N=-1), ERR, "bad argument"),
         (dict(K=0), ERR, "bad argument"),
         (dict(M=0, A=0, W=0, **{out: 0}), 0, None),                                   # FERN_OK before the NULL check: behaviour
         (dict(N=0, A=0, W=0, **{out: 0}, epilogue=9), 0, None),
         (dict(M=0, K=0), ERR, "bad argument"),                                        # ... but behind the size check
         (dict(A=0), ERR, "NULL argument"),
         ({out: 0}, ERR, "NULL argument"),
         ({null_operand: 0}, ERR, "NULL argument"),
         (dict(K=k_bad, lda=k_bad + 64, ldw=k_bad + 64), ERR, k_text),
         (dict(K=k_bad), ERR, k_text),                                                 # multiples before lda >= K
         (dict(lda=k - 16), ERR, LD_TEXT),
         (dict(ldw=k - 16), ERR, LD_TEXT),
         (dict(ldc=ENTRIES[name]["N"] - 16 if name == "fern_gemm_mx8_quant" else 4), ERR, LD_TEXT),
         (dict(A=0, epilogue=9), ERR, "NULL argument"))                                # operands before the epilogue
    if ld_odd:
        rows(name, (dict(lda=ld_odd), ERR, k_text), (dict(ldw=ld_odd), ERR, k_text))
for name in ("fern_gemm", "fern_gemm_bf16"):
    rows(name,
         (dict(epilogue=5), ERR, "unknown epilogue"),
         (dict(epilogue=-1), ERR, "unknown epilogue"),
         (dict(epilogue=5, K=33), ERR, "unknown epilogue"))                            # the epilogue before K's multiple
rows("fern_gemm",
     (dict(epilogue=RESIDUAL), ERR, "residual is NULL"),
     (dict(epilogue=RESIDUAL, K=33), ERR, "residual is NULL"))
for name in ("fern_gemm_bf16", "fern_gemm_fp8"):
    rows(name,
         (dict(epilogue=RESIDUAL), ERR, "the residual epilogue needs a residual and fp32 output"),
         (dict(epilogue=RESIDUAL, residual=P, out_bf16=1), ERR, "the residual epilogue needs a residual and fp32 output"))
for name in ("fern_gemm_fp8", "fern_gemm_mx8"):
    rows(name,
         (dict(epilogue=RELU), ERR, LIST4),
         (dict(epilogue=5), ERR, LIST4),
         (dict(epilogue=RELU, K=32), ERR, LIST4))
rows("fern_gemm_mx8",
     (dict(epilogue=RESIDUAL), ERR, "the residual epilogue needs a residual"),
     (dict(epilogue=RESIDUAL, out_bf16=1, K=32), ERR, "the residual epilogue needs a residual"),
     (dict(scale_rows_a=3), ERR, "K % 128, lda % 16 and ldw % 16 must be 0, scale_rows >= rows"),
     (dict(scale_rows_w=7), ERR, "K % 128, lda % 16 and ldw % 16 must be 0, scale_rows >= rows"))
rows("fern_gemm_mx8_quant",
     (dict(epilogue=RESIDUAL), ERR, "epilogue must be BIAS, BIAS_GELU or BIAS_QUICKGELU"),
     (dict(epilogue=RELU, K=32), ERR, "epilogue must be BIAS, BIAS_GELU or BIAS_QUICKGELU"),
     (dict(N=64), ERR, "K % 128, N % 128, lda / ldw / ldc % 16 must be 0, scale_rows >= rows"),
     (dict(ldc=136), ERR, "K % 128, N % 128, lda / ldw / ldc % 16 must be 0, scale_rows >= rows"),
     (dict(scale_rows_w=127), ERR, "K % 128, N % 128, lda / ldw / ldc % 16 must be 0, scale_rows >= rows"),
     (dict(scale_rows_c=3), ERR, "K % 128, N % 128, lda / ldw / ldc % 16 must be 0, scale_rows >= rows"))

# ---- the two quantiser entries ----------------------------------------------------------------------------------------------------
FP8_SHAPE = "need d % 8 == 0, d <= 4096, ld % 8 == 0"
MXQ_SHAPE = "need d % 128 == 0, d <= 4096, ld % 8 == 0, scale_rows >= rows"
QUANT_LD = "need ldx >= d and ldy >= d (rows must not overlap)"
rows("fern_quantize_rows_fp8",
     (NOCTX, ERR, "bad argument"),
     (dict(rows=-1), ERR, "bad argument"),
     (dict(x=0), ERR, "bad argument"),
     (dict(scale=0), ERR, "bad argument"),
     (dict(d=0), ERR, FP8_SHAPE),
     (dict(d=4), ERR, FP8_SHAPE),
     (dict(d=4104, ldx=4104, ldy=4104), ERR, FP8_SHAPE),
     (dict(ldx=132), ERR, FP8_SHAPE),
     (dict(ldy=132), ERR, FP8_SHAPE),
     (dict(ldx=120), ERR, QUANT_LD),
     (dict(ldy=120), ERR, QUANT_LD),
     (dict(y=0, d=4), ERR, "bad argument"),                                            # operands before the shape
     (dict(d=4, ldx=0), ERR, FP8_SHAPE))                                               # the shape before ld >= d
rows("fern_quantize_mx8",
     (NOCTX, ERR, "bad argument"),
     (dict(rows=-1), ERR, "bad argument"),
     (dict(y=0), ERR, "bad argument"),
     (dict(scales=0), ERR, "bad argument"),
     (dict(d=0), ERR, MXQ_SHAPE),
     (dict(d=64), ERR, MXQ_SHAPE),
     (dict(d=4224, ldx=4224, ldy=4224), ERR, MXQ_SHAPE),
     (dict(ldx=132), ERR, MXQ_SHAPE),
     (dict(scale_rows=3), ERR, MXQ_SHAPE),
     (dict(ldx=120), ERR, QUANT_LD),
     (dict(ldy=120), ERR, QUANT_LD),
     (dict(scale_rows=3, ldx=120), ERR, MXQ_SHAPE))

# ---- the three attention entries --------------------------------------------------------------------------------------------------
for name in ("fern_attention", "fern_attention_bf16"):
    rows(name,
         (NOCTX, ERR, "NULL argument"),
         (dict(q=0), ERR, "NULL argument"),
         (dict(out=0), ERR, "NULL argument"),
         (dict(ldq=7), ERR, ATTN_LD),
         (dict(ldk=7), ERR, ATTN_LD),
         (dict(ldv=7), ERR, ATTN_LD),
         (dict(ldo=7), ERR, ATTN_LD),
         (dict(v=0, ldo=7), ERR, "NULL argument"))                                     # operands before the leading dimensions
rows("fern_attention_mx8",
     (NOCTX, ERR, "ctx is NULL"),
     (dict(batch=0), ERR, "bad shape"),
     (dict(heads=0), ERR, "bad shape"),
     (dict(s_q=0), ERR, "bad shape"),
     (dict(s_k=0), ERR, "bad shape"),
     (dict(causal=1, s_k=6, scale_rows=6), ERR, "bad shape"),
     (dict(causal=1, s_q=97, s_k=97, scale_rows=97), ERR, "bad shape"),
     (dict(s_k=4097), ERR, "bad shape"),
     (dict(head_dim=0), ERR, MXA_SHAPE),
     (dict(heads=8, head_dim=16), ERR, MXA_SHAPE),
     (dict(heads=1, head_dim=128), ERR, MXA_SHAPE),
     (dict(heads=3), ERR, MXA_SHAPE),
     (dict(q=0), ERR, "NULL argument"),
     (dict(scales=0), ERR, "NULL argument"),
     (dict(ldq=132), ERR, MXA_LD),
     (dict(ldk=120), ERR, MXA_LD),
     (dict(ldo=136), ERR, MXA_LD),
     (dict(ldo=112), ERR, MXA_LD),
     (dict(scale_rows=4), ERR, MXA_LD),
     (dict(q=ODD), ERR, ALIGN),
     (dict(out=ODD), ERR, ALIGN),
     (dict(batch=0, q=0), ERR, "bad shape"),                                           # the shape before the operands
     (dict(heads=3, k=0), ERR, MXA_SHAPE),
     (dict(v=0, ldv=120), ERR, "NULL argument"),                                       # the operands before the leading dimensions
     (dict(ldq=120, q=ODD), ERR, MXA_LD))                                              # ... and those before the alignment

# ---- fern_layernorm_q, fern_im2col_q ------------------------------------------------------------------------------------------------
rows("fern_layernorm_q",
     (NOCTX, ERR, "ctx is NULL"),
     (dict(rows=-1), ERR, "bad argument"),
     (dict(out_form=3), ERR, "bad argument"),
     (dict(rows=0, x=0, y=0, gamma=0, beta=0, scales=0), 0, None),
     (dict(x=0), ERR, "NULL argument"),
     (dict(gamma=0), ERR, "NULL argument"),
     (dict(out_form=FP8, scales=0), ERR, "NULL argument"),
     (dict(d=0), ERR, LNQ_SHAPE),
     (dict(d=6), ERR, LNQ_SHAPE),
     (dict(d=1284, ldx=1284, ldy=1284), ERR, LNQ_SHAPE),
     (dict(ldx=124), ERR, LNQ_SHAPE),
     (dict(ldy=130), ERR, LNQ_SHAPE),
     (dict(x=ODD), ERR, ALIGN),
     (dict(beta=ODD), ERR, ALIGN),
     (dict(scales=ODD), ERR, ALIGN),
     (dict(d=64), ERR, "the MX form needs d % 128 == 0 and scale_rows >= rows"),
     (dict(scale_rows=3), ERR, "the MX form needs d % 128 == 0 and scale_rows >= rows"),
     (dict(out_form=BF16, x_is_bf16=1), ERR, "bf16 rows are read by the MX form only"),
     (dict(out_form=FP8, x_is_bf16=1), ERR, "bf16 rows are read by the MX form only"),
     (dict(rows=0, out_form=3), ERR, "bad argument"),                                  # the form before rows == 0
     (dict(y=0, d=6), ERR, "NULL argument"),                                           # operands, shape, alignment, the MX form's own
     (dict(d=6, x=ODD), ERR, LNQ_SHAPE),
     (dict(y=ODD, scale_rows=3), ERR, ALIGN))
rows("fern_im2col_q",
     (NOCTX, ERR, "ctx is NULL"),
     (dict(b=-1), ERR, "bad argument"),
     (dict(out_form=FP8), ERR, "bad argument"),
     (dict(b=0, images=0, y=0, scales=0), 0, None),
     (dict(images=0), ERR, "NULL argument"),
     (dict(y=0), ERR, "NULL argument"),
     (dict(scales=0), ERR, "NULL argument"),
     (dict(patch=0), ERR, IM2COL_SHAPE),
     (dict(patch=6, img=6), ERR, IM2COL_SHAPE),
     (dict(img=0), ERR, IM2COL_SHAPE),
     (dict(img=40), ERR, IM2COL_SHAPE),
     (dict(patch=24, img=48), ERR, IM2COL_SHAPE),
     (dict(patch=4, img=8, out_form=BF16, scales=0), ERR, IM2COL_SHAPE),
     (dict(patch=8, img=16), ERR, IM2COL_SHAPE),
     (dict(scale_rows=3), ERR, "scale_rows >= rows"),
     (dict(images=ODD), ERR, ALIGN),
     (dict(y=ODD), ERR, ALIGN),
     (dict(scales=ODD), ERR, ALIGN),
     (dict(b=0, out_form=FP8), ERR, "bad argument"),                                   # the form before b == 0
     (dict(images=0, patch=6), ERR, "NULL argument"),                                  # operands, shape, scale rows, alignment
     (dict(patch=6, img=6, scale_rows=0), ERR, IM2COL_SHAPE),
     (dict(scale_rows=3, y=ODD), ERR, "scale_rows >= rows"))


# entry -> (rows, distinct refusal texts = the refusal branches of the entry in the source the table was written from, rows that return
# FERN_OK): deleting a family of branches from the table changes a figure here
COVERAGE = {
    "fern_gemm": (21, 6, 2), "fern_gemm_bf16": (23, 6, 2), "fern_gemm_fp8": (23, 6, 2), "fern_gemm_mx8": (25, 6, 2),
    "fern_gemm_mx8_quant": (24, 5, 2), "fern_quantize_rows_fp8": (13, 3, 0), "fern_quantize_mx8": (12, 3, 0), "fern_attention": (8, 2, 0),
    "fern_attention_bf16": (8, 2, 0), "fern_attention_mx8": (25, 6, 0), "fern_layernorm_q": (23, 7, 1), "fern_im2col_q": (22, 6, 1),
}


def test_table_covers_every_entry():
    got = {e: (sum(r[0] == e for r in ROWS), len({r[3] for r in ROWS if r[0] == e and r[3] is not None}), sum(r[0] == e and r[2] == 0 for r in ROWS))
           for e in ENTRIES}
    assert got == COVERAGE


def test_refusals(engine):
    lib = engine.lib
    assert lib.fern_tuner_import(None) == ERR
    untouched = lib.fern_last_error()      # the text a row finds in place: a row that returns FERN_OK must leave it as it is
    wrong = []
    for entry, over, code, text in ROWS:
        kw = dict(ENTRIES[entry], **{k: v for k, v in over.items() if k != "ctx"})
        assert set(kw) == set(ENTRIES[entry]), (entry, over)
        ctx = over.get("ctx", engine._h)
        assert lib.fern_tuner_import(None) == ERR      # puts that text back: a row's text is then its own, not an earlier row's
        got = getattr(lib, entry)(ctx, *kw.values())
        err = lib.fern_last_error()
        want = f"{entry}: {text}".encode() if text is not None else untouched
        if got != code or err != want:
            wrong.append((entry, over, got, err))
    assert not wrong, wrong

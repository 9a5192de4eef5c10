"""Kernel-level parity of the producers that fuse a quantiser into another kernel: LayerNorm -> bf16 / per-row fp8 / MX8 (the
half-wave and one-row kernels, and the several-rows fp32 kernel), the attention kernel's block-scaled output, im2col -> bf16 / MX8, reached through
fern_layernorm_q / fern_attention_mx8 / fern_im2col_q, i.e. through the launchers the towers call.  Every MX output is written
with scale_rows > rows into a sentinel-filled scale array, and the padding rows must come back untouched."""
import pytest
import torch
import torch.nn.functional as F

from fashionern_aaai2024_amd.engine import QFORM_BF16, QFORM_FP8, QFORM_MX8
from gemm_refs import e4m3_code, e8m0_byte, mx_scales_by_block
from oracle.clip import mx8_dequantize, mx8_quantize

pytestmark = pytest.mark.gpu

EPS = 1e-5
SENTINEL = 0xA5
# Relative error of an fp32 LayerNorm against fp64, per element and relative to the magnitude of what is summed,
# (|x - mean| + mean|x|) * rstd * |gamma| + |beta|: the row sums of d <= 1024 fp32 values carry ~log2(d) roundings (~10 ulp
# of the sum of |x|), rsqrtf ~2 ulp, the affine map 3 more.  Measured 2^-22 for torch's fp32 LayerNorm on these inputs and
# checked for the library's own fp32 LayerNorm in test_layernorm_fp32_error_is_within_delta; 2^-18 leaves a factor 16.
DELTA = 2.0 ** -18


def _ln_inputs(rows, d, seed, bf16=False):
    """CLIP-like rows: a 32-block of outlier channels (x50), per-row offsets, a constant row of 0.5 (its sums are exact: zero
    variance, the output is exactly beta), and a 32-column block with gamma = beta = 0 (an all-zero output block: scale byte 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, generator=g) + 0.5 * torch.randn(rows, 1, generator=g)
    x[:, 32:64] *= 50.0
    if rows > 1:
        x[rows // 2] = 0.5
    gamma = 1.0 + 0.2 * torch.randn(d, generator=g)
    beta = 0.2 * torch.randn(d, generator=g)
    gamma[64:96] = 0.0
    beta[64:96] = 0.0
    if bf16:
        x = x.bfloat16().float()
    return x, gamma, beta


def _ln64(x, gamma, beta):
    """fp64 LayerNorm and the per-element magnitude DELTA is relative to."""
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + EPS)
    y = (x - mu) * r * gamma.double() + beta.double()
    mag = ((x - mu).abs() + x.abs().mean(-1, keepdim=True)) * r * gamma.double().abs() + beta.double().abs()
    return y, mag


def _scales(d, srows):
    return torch.full((d // 128, srows, 4), SENTINEL, dtype=torch.uint8, device="cuda")


def _by_block(sc, rows):
    """[d/128, scale_rows, 4] scale array -> [rows, d/32] (block b = k // 32), after checking that the padding rows are untouched."""
    sc = sc.cpu()
    assert (sc[:, rows:] == SENTINEL).all(), "scale bytes beyond `rows` were written"
    return mx_scales_by_block(sc[:, :rows])


def _ord(b):
    return torch.where(b >= 128, -(b & 0x7F), b)


def _check_fp64_rule(y8, e_got, y64, tol):
    """The fp64 rule of the MX LayerNorm producers.  Reference: mx8_quantize of the fp64 LayerNorm.  A block's scale byte may differ
    only when [max - tol, max + tol] holds a 448 * 2^k boundary (then by one), an element byte only when its scaled interval holds an
    e4m3 rounding midpoint (then by exactly one code step; elements are compared on the kernel's own scale).  Returns the fraction
    of elements whose byte differs under such an excuse."""
    rows, d = y64.shape
    nb = d // 32
    blk = y64.reshape(rows, nb, 32)
    tb = tol.reshape(rows, nb, 32)
    m = blk.abs().amax(-1)
    tm = tb.amax(-1)
    e_lo, e_hi, e_mid = e8m0_byte((m - tm).clamp_min(0)), e8m0_byte(m + tm), e8m0_byte(m)
    e_got = e_got.int()
    exact_blk = e_lo == e_hi
    assert torch.equal(e_got[exact_blk], e_mid[exact_blk].int()), "scale byte differs outside the excused blocks"
    assert ((e_got >= e_lo) & (e_got <= e_hi) & (e_hi - e_lo <= 1)).all(), "scale byte outside its excuse"
    sc = torch.ldexp(torch.ones((), dtype=torch.float64), 127 - e_got).unsqueeze(-1)
    v, tv = blk * sc, tb * sc
    c_ref, o_ref = e4m3_code(v)
    c_lo, o_lo = e4m3_code(v - tv)
    c_hi, o_hi = e4m3_code(v + tv)
    got = y8.cpu().int().reshape(rows, nb, 32)
    o_got = _ord(got)
    excused = c_lo != c_hi
    assert torch.equal(got[~excused], c_ref[~excused]), "element byte differs outside the excused elements"
    assert ((o_got >= o_lo) & (o_got <= o_hi))[excused].all(), "excused element outside its interval"
    mism = excused & (got != c_ref)
    assert ((o_got - o_ref).abs()[mism] <= 1).all(), "an excused mismatch is more than one e4m3 code step"
    return mism.sum().item() / got.numel()


# ---- LayerNorm -> bf16 / fp8 / MX8, exact forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 6, 197])
@pytest.mark.parametrize("d", [128, 256, 384, 512, 640, 768, 1024])
def test_layernorm_bf16_and_fp8_are_bit_exact(engine, rows, d):
    """LN -> bf16 == to_bf16(layernorm(x)); LN -> fp8 == quantize_rows_fp8(layernorm(x)), bytes and scale floats.  The fused kernels
    are the one-row kernel with another store (layernorm_kernel<float, Out>: one row_layernorm, and LN -> fp8 stores through the
    row_store_fp8 that quantize_rows_fp8_kernel uses), so the fp32 values they round are those fern_layernorm returns."""
    x, gamma, beta = _ln_inputs(rows, d, 7 * d + rows)
    xc = x.cuda()
    ln = engine.layernorm(xc, gamma, beta, EPS, residual=torch.zeros_like(xc))      # the one-row kernel
    yb = engine.layernorm_q(xc, gamma, beta, EPS, QFORM_BF16)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb.cpu(), ln.cpu().bfloat16())
    y8, s8 = engine.layernorm_q(xc, gamma, beta, EPS, QFORM_FP8)
    r8, rs = engine.quantize_rows_fp8(ln)
    assert torch.equal(s8.cpu(), rs.cpu()) and torch.equal(y8.cpu(), r8.cpu())
    if rows > 1:
        assert torch.equal(yb[rows // 2].cpu(), beta.bfloat16())                  # the constant row: exactly beta


@pytest.mark.parametrize("rows", [1, 6, 197])
@pytest.mark.parametrize("d", [128, 384, 640])
@pytest.mark.parametrize("bf16", [False, True])
def test_layernorm_mx8_one_row_kernel_is_bit_exact(engine, rows, d, bf16):
    """Widths that are not a multiple of 256 take layernorm_kernel<T, RowToMx8> (one row per wave, fp32 or bf16 rows): equal to
    quantize_mx8(layernorm(x)) bit for bit, and to the fp64 rule.  scale_rows = rows + 5, padding untouched."""
    x, gamma, beta = _ln_inputs(rows, d, 11 * d + rows, bf16)
    ln = engine.layernorm(x.cuda(), gamma, beta, EPS)
    xin = x.bfloat16().cuda() if bf16 else x.cuda()
    y8, sc = engine.layernorm_q(xin, gamma, beta, EPS, QFORM_MX8, scales=_scales(d, rows + 5))
    r8, rsc = engine.quantize_mx8(ln)
    e = _by_block(sc, rows)
    assert torch.equal(e, _by_block(rsc, rows)) and torch.equal(y8.cpu(), r8.cpu())
    y64, mag = _ln64(x, gamma, beta)
    _check_fp64_rule(y8, e, y64, DELTA * mag)
    assert (e[:, 2] == 1).all() and (y8[:, 64:96] == 0).all()                     # gamma = beta = 0: an all-zero block, scale byte 1
    if rows > 1:
        q, eb = mx8_quantize(beta)
        assert torch.equal(y8[rows // 2].cpu(), q.view(torch.uint8)) and torch.equal(e[rows // 2], eb)


@pytest.mark.parametrize("rows", [1, 6, 197])
@pytest.mark.parametrize("d", [256, 768, 1024])
@pytest.mark.parametrize("bf16", [False, True])
def test_layernorm_mx8_several_rows_kernel_is_bit_exact(engine, rows, d, bf16):
    """(The name is from the four-rows-per-wave MX kernel these inputs once reached; the 18 cases keep their ids.)  A row stride with ldx % 8 == 4 (every pointer 16-byte aligned) is outside the half-wave kernel's 16-byte row loads, so at
    these widths, too, the launcher falls to the one-row kernel (layernorm_kernel<T, RowToMx8>; the four-rows-per-wave MX kernel
    that once took such calls is gone).  Equal to quantize_mx8(layernorm(x)) bit for bit, with a scale_rows > rows that is a
    multiple of 4 and one that is not, padding untouched."""
    x, gamma, beta = _ln_inputs(rows, d, 13 * d + rows, bf16)
    ldx = d + 4
    buf = torch.zeros(rows, ldx, dtype=torch.bfloat16 if bf16 else torch.float32)
    buf[:, :d] = x
    xin = buf.cuda()[:, :d]
    assert xin.stride(0) % 8 == 4 and xin.data_ptr() % 16 == 0
    ln = engine.layernorm(x.cuda(), gamma, beta, EPS)
    r8, rsc = engine.quantize_mx8(ln)
    y64, mag = _ln64(x, gamma, beta)
    p4 = 4 - rows % 4
    for pad in (p4, p4 + 1):
        y8, sc = engine.layernorm_q(xin, gamma, beta, EPS, QFORM_MX8, scales=_scales(d, rows + pad))
        e = _by_block(sc, rows)
        assert torch.equal(e, _by_block(rsc, rows)) and torch.equal(y8.cpu(), r8.cpu()), pad
        _check_fp64_rule(y8, e, y64, DELTA * mag)


@pytest.mark.parametrize("rows", [1, 6, 197, 1000])
@pytest.mark.parametrize("d", [256, 512, 768, 1024])
@pytest.mark.parametrize("bf16", [False, True])
def test_layernorm_mx8_half_wave_kernel_fp64_rule(engine, rows, d, bf16):
    """The towers' MX LayerNorm (layernorm_half_kernel<NV, T>: half a wave per row, statistics added in another order than the
    one-row kernel, so its fp32 values may differ in the last bits) against mx8_quantize of an fp64 LayerNorm, under the fp64 rule
    (_check_fp64_rule, DELTA above).  The excused fraction must stay below 1e-3."""
    x, gamma, beta = _ln_inputs(rows, d, 17 * d + rows, bf16)
    xin = x.bfloat16().cuda() if bf16 else x.cuda()
    y8, sc = engine.layernorm_q(xin, gamma, beta, EPS, QFORM_MX8, scales=_scales(d, rows + 5))
    e = _by_block(sc, rows)
    y64, mag = _ln64(x, gamma, beta)
    frac = _check_fp64_rule(y8, e, y64, DELTA * mag)
    print(f"half-wave LN d={d} rows={rows} bf16={bf16}: excused fraction {frac:.2e}")
    assert frac < 1e-3
    assert (e[:, 2] == 1).all() and (y8[:, 64:96] == 0).all()
    if rows > 1:
        q, eb = mx8_quantize(beta)
        assert torch.equal(y8[rows // 2].cpu(), q.view(torch.uint8)) and torch.equal(e[rows // 2], eb)


@pytest.mark.parametrize("d", [256, 512, 768, 1024])
def test_layernorm_several_rows_kernel_equals_one_row_kernel(engine, d):
    """layernorm(x) (layernorm_rows_kernel<NV, 4>) == layernorm(x, residual=zeros) (layernorm_kernel<float, RowToF32>, one row per wave) bit for
    bit: the "statement for statement" claim that makes a row's LayerNorm independent of the kernel its batch size picks."""
    for rows in (1, 6, 197):
        x, gamma, beta = _ln_inputs(rows, d, 19 * d + rows)
        xc = x.cuda()
        assert torch.equal(engine.layernorm(xc, gamma, beta, EPS), engine.layernorm(xc, gamma, beta, EPS, residual=torch.zeros_like(xc))), rows


@pytest.mark.parametrize("d", [128, 384, 640, 768, 1024])
def test_layernorm_fp32_error_is_within_delta(engine, d):
    """DELTA's premise on this hardware: the library's fp32 LayerNorm (one-row and several-rows kernels) is within DELTA of fp64,
    relative to the magnitude of its summands, on the inputs the fp64 rule is applied to."""
    x, gamma, beta = _ln_inputs(197, d, 23 * d)
    y64, mag = _ln64(x, gamma, beta)
    for res in (None, torch.zeros(197, d)):
        got = engine.layernorm(x.cuda(), gamma, beta, EPS, residual=res).cpu().double()
        err = (got - y64).abs()
        assert (err[mag == 0] == 0).all()                                     # gamma = beta = 0: exact zeros
        worst = (err / mag)[mag > 0].max().item()
        print(f"fp32 LN d={d}: error {worst * 2 ** 18:.4f} * 2^-18")
        assert worst <= DELTA / 4


# ---- attention -> MX8 --------------------------------------------------------------------------------------------------------------
ATTN_CASES = [(3, 12, 64, 197, False), (2, 8, 64, 77, True), (2, 4, 32, 50, False), (1, 4, 96, 33, True), (2, 4, 96, 120, False)]


@pytest.mark.parametrize("b,heads,hd,s,causal", ATTN_CASES)
def test_attention_mx8_output(engine, b, heads, hd, s, causal):
    """The attention kernel's block-scaled output (AttnParams.out_q8: attn_bf16_kernel's epilogue).  attn.hip launches the SAME
    kernel instance for the bf16 and the MX output (launch_form picks the template from head_dim / s_k / causal only; out_q8 is
    a run-time branch of the store), so both round one fp32 value o * (1/sum): (a) the scale byte equals the one of the bf16
    output's block maximum unless that maximum's bf16 rounding interval holds a 448 * 2^k boundary, and each element byte equals
    e4m3(bf16 value * 2^(127-e)) unless its bf16 rounding interval holds an e4m3 midpoint (excused mismatches < 5 %: a bf16 value
    that IS a midpoint is 1 in 16); (b) against fp64 attention on the same bf16 operands, within the bf16 test's budget plus half
    an e4m3 step.  Written with ldo > width and scale_rows > rows; the gap columns and padding rows stay untouched."""
    g = torch.Generator().manual_seed(b * 100 + heads * 10 + hd + s)
    w = heads * hd
    q, k, v = (torch.randn(b, s, w, generator=g).bfloat16() for _ in range(3))
    v[..., :32] *= 30.0                                                     # an outlier block of the output
    rows = b * s
    ldo = w + 32
    out = torch.full((rows, ldo), SENTINEL, dtype=torch.uint8, device="cuda")
    y8, sc = engine.attention_mx8(q.cuda(), k.cuda(), v.cuda(), heads, causal=causal, out=out, scales=_scales(w, rows + 3))
    yb = engine.attention_bf16(q.cuda(), k.cuda(), v.cuda(), heads, causal=causal).cpu().reshape(rows, w)
    # The towers' input layout: q, k, v as column slices of ONE packed [rows, 3 W + 8] buffer (ldq = ldk = ldv = 3 W + 8) with NaN in its
    # gap columns and around it, the outputs inside 0xA5 frames (tests/framed.py): the same bytes and scales, nothing else written.
    import ctypes as C
    from framed import NAN, Framed
    from fashionern_aaai2024_amd import _lib
    from fashionern_aaai2024_amd.engine import _stream
    ldp = 3 * w + 8
    packed = Framed(rows, 3 * w, ldp, torch.bfloat16, NAN, "cuda").load(torch.cat([q, k, v], -1))
    fo = Framed(rows, w, ldo, torch.uint8, SENTINEL, "cuda")
    fsc = Framed(w // 128, rows * 4, (rows + 3) * 4, torch.uint8, SENTINEL, "cuda")
    p0 = packed.data_ptr()
    _lib.check(engine.lib.fern_attention_mx8(engine._h, C.c_void_p(p0), ldp, C.c_void_p(p0 + 2 * w), ldp, C.c_void_p(p0 + 4 * w), ldp,
                                             C.c_void_p(fo.data_ptr()), ldo, C.c_void_p(fsc.data_ptr()), rows + 3, b, heads, hd, s, s,
                                             int(causal), hd ** -0.5, _stream()), "fern_attention_mx8")
    torch.cuda.synchronize()
    fo.assert_intact("attention_mx8 out (packed QKV)")
    fsc.assert_intact("attention_mx8 scales (packed QKV)")
    packed.assert_intact("packed QKV (input)")
    assert torch.equal(fo.view, y8[:, :w]), "packed q / k / v: the e4m3fn bytes differ from the contiguous call"
    assert torch.equal(fsc.view.reshape(w // 128, rows, 4), sc[:, :rows]), "packed q / k / v: the scale bytes differ from the contiguous call"
    y8 = y8.cpu()
    assert (y8[:, w:] == SENTINEL).all(), "bytes beyond the width were written"
    y8 = y8[:, :w].int()
    e = _by_block(sc, rows).int()
    # (a) consistency with the bf16 output of the same kernel
    nb = w // 32
    bb = yb.double().reshape(rows, nb, 32)
    half = lambda t: torch.ldexp(torch.ones((), dtype=torch.float64), torch.frexp(t.float())[1] - 9)   # half a bf16 ulp of |t| (2^(E-8))
    m = bb.abs().amax(-1)
    e_lo, e_hi = e8m0_byte(m - half(m)), e8m0_byte(m + half(m))
    sure = e_lo == e_hi
    assert torch.equal(e[sure], e8m0_byte(m)[sure]), "scale byte differs from the bf16 output's block maximum"
    assert ((e >= e_lo) & (e <= e_hi)).all()
    scl = torch.ldexp(torch.ones((), dtype=torch.float64), 127 - e).unsqueeze(-1)
    hb = half(bb.abs())
    c_ref, o_ref = e4m3_code(bb * scl)
    c_lo, o_lo = e4m3_code((bb - hb) * scl)
    c_hi, o_hi = e4m3_code((bb + hb) * scl)
    got = y8.reshape(rows, nb, 32)
    o_got = _ord(got)
    excused = c_lo != c_hi
    assert torch.equal(got[~excused], c_ref[~excused]), "element byte differs from e4m3 of the bf16 output"
    assert ((o_got >= torch.minimum(o_lo, o_hi)) & (o_got <= torch.maximum(o_lo, o_hi)))[excused].all()
    frac = (excused & (got != c_ref)).sum().item() / got.numel()
    print(f"attention mx8 b={b} heads={heads} hd={hd} s={s} causal={causal}: excused fraction {frac:.3%}")
    assert frac < 0.05
    # (b) against fp64 attention on the same bf16 operands
    qd, kd, vd = (t.double().view(b, -1, heads, hd).transpose(1, 2) for t in (q, k, v))
    att = qd @ kd.transpose(-1, -2) * hd ** -0.5
    if causal:
        att = att + torch.full((s, s), float("-inf"), dtype=torch.float64).triu(1)
    ref = (torch.softmax(att, dim=-1) @ vd).transpose(1, 2).reshape(rows, w)
    dq = mx8_dequantize(y8.to(torch.uint8).view(torch.float8_e4m3fn), e.to(torch.uint8), torch.float64)
    step = 2.0 ** -4 * torch.maximum(dq.abs(), ref.abs()) + torch.ldexp(torch.ones((), dtype=torch.float64), e - 137).repeat_interleave(32, -1)
    budget = 2 ** -7 * max(1.0, ref.abs().max().item())
    assert ((dq - ref).abs() <= budget + step).all(), ((dq - ref).abs() - step).max().item()


def test_attention_mx8_refuses_head_dims_outside_the_mx_blocks(engine):
    """head_dim % 32 != 0 cannot be block-quantised per head: refused by the entry point's validation, before any launch."""
    from fashionern_aaai2024_amd._lib import FernError
    q = torch.zeros(1, 8, 8 * 48, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(FernError, match="head_dim % 32"):
        engine.attention_mx8(q, q, q, 8)
    q = torch.zeros(1, 8, 3 * 32, dtype=torch.bfloat16, device="cuda")     # heads * head_dim % 128 != 0: no whole 128-k scale tiles
    with pytest.raises(FernError, match="head_dim % 128"):
        engine.attention_mx8(q, q, q, 3)


# ---- im2col -> bf16 / MX8 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,img,patch", [(3, 224, 16), (5, 48, 16), (2, 64, 8)])
def test_im2col_is_bit_exact(engine, b, img, patch):
    """Patch rows (channel, y, x order) of the bf16-operand and block-scaled patch embeddings: to_bf16 / mx8_quantize of
    F.unfold(images, patch, stride=patch).transpose(1, 2), bit for bit; ViT-B/16 (224 / 16) and the tiny towers' shapes."""
    g = torch.Generator().manual_seed(b * img + patch)
    imgs = torch.randn(b, 3, img, img, generator=g)
    imgs[0, 1, :patch, :patch] *= 40.0                                       # an outlier patch channel
    imgs[-1, :, -patch:, -patch:] = 0.0                                      # an all-zero patch: scale bytes 1
    rows, d = b * (img // patch) ** 2, 3 * patch * patch
    ref = F.unfold(imgs, patch, stride=patch).transpose(1, 2).reshape(rows, d)
    yb = engine.im2col_q(imgs.cuda(), patch, QFORM_BF16)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb.cpu(), ref.bfloat16())
    if d % 128 == 0:
        y8, sc = engine.im2col_q(imgs.cuda(), patch, QFORM_MX8, scales=_scales(d, rows + 5))
        q, e = mx8_quantize(ref)
        assert torch.equal(_by_block(sc, rows), e) and torch.equal(y8.cpu(), q.view(torch.uint8))
        assert (e[-1] == 1).all()


# ---- scale rows beyond the row count -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k", [(197, 384, 256), (64, 128, 768), (333, 640, 512)])
def test_mx8_scale_rows_beyond_rows(engine, m, n, k):
    """The MX scale layout is interleaved by 128-k tile (byte ((b/4) * scale_rows + r) * 4 + b % 4): quantize_mx8 with
    scale_rows > rows writes the compact form's bytes at the padded positions and nothing else, and gemm_mx8 with
    scale_rows_a = M + 3 / scale_rows_w = N + 5 equals the compact-layout result bit for bit."""
    g = torch.Generator().manual_seed(m + n + k)
    a = torch.randn(m, k, generator=g) * torch.logspace(-1, 1, k // 32).repeat_interleave(32)
    w = torch.randn(n, k, generator=g) * k ** -0.5
    bias = torch.randn(n, generator=g)
    a8, sa = engine.quantize_mx8(a)
    w8, sw = engine.quantize_mx8(w)
    a8p, sap = engine.quantize_mx8(a, scales=_scales(k, m + 3))
    w8p, swp = engine.quantize_mx8(w, scale_rows=n + 5)
    assert torch.equal(a8p, a8) and torch.equal(w8p, w8) and swp.shape[1] == n + 5
    assert torch.equal(_by_block(sap, m), _by_block(sa, m))
    assert torch.equal(swp[:, :n].cpu(), sw.cpu())
    ref = engine.gemm_mx8(a8, sa, w8, sw, bias=bias)
    got = engine.gemm_mx8(a8p, sap, w8p, swp, bias=bias, scale_rows_a=m + 3, scale_rows_w=n + 5)
    assert torch.equal(got, ref)

"""Leading dimensions and output frames of the kernel-level ABI (include/fern.h, "building blocks" and the ranking outputs).

Every other kernel-level test goes through the engine wrappers: ld == width, outputs of exactly rows * width elements.  Here each entry
is called directly with pointers of FRAMED operands (tests/framed.py): strided views with ld > width inside one allocation whose every
other byte is a known pattern -- 0xA5 around outputs, NaN (fp32 / bf16 / e4m3fn) or 2^127 (E8M0) around inputs.  Per case:
  (a) the strided result is BIT-IDENTICAL to the same entry on contiguous, unframed copies of the operands (the tile choice is keyed on
      (M, N, K, epilogue, loader), never on a stride, and every configuration of a family gives the same bits: kernels.h);
  (b) the contiguous result is within the family's existing reference and bound (tests/gemm_refs.py: shared with test_gpu_kernels.py);
  (c) no byte outside the [rows, width] view of an output was written -- gap columns, the rows before and after, in-place forms included;
  (d) the result is finite although everything around A, W, bias, residual and the scales is NaN (implied by (a); asserted on its own so
      that a failure names its cause).
No case had to fall back from (a) to a reference comparison.  Nothing here can reach unmapped memory: every band is 256 rows of ld
elements, one full workgroup tile of the largest configuration."""

import pytest
import torch

import gemm_refs as R
from framed import E8M0_HUGE, FP8_NAN, NAN, SENTINEL, Framed, framed_like, framed_vec
from support import assert_same_bits, ptr, unit
from fashionern_aaai2024_amd import _lib
from fashionern_aaai2024_amd.engine import _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _moat(t):
    return NAN if t.is_floating_point() else FP8_NAN      # uint8 operands here are e4m3fn bytes


# ====================================================================================================================================
# GEMM families
# ====================================================================================================================================
KMIN = {"f32": 32, "f32x3": 32, "bf16": 32, "fp8": 64, "mx8": 128, "mx8q": 128}
GAP = {"f32": 4, "f32x3": 4, "bf16": 8, "fp8": 16, "mx8": 16, "mx8q": 16}          # the smallest legal lda / ldw gap of the entry
SHAPES = [(1, 32), (33, 65), (257, 129), (300, 520)]      # one row; tails in both dimensions; an odd N; the edges of the 128- and 256-wide tiles
QUANT_SHAPES = [(m, n) for m in (1, 33, 257, 300) for n in (128, 384)]              # fern_gemm_mx8_quant: N % 128 == 0
# (epilogue, bf16 output, residual == C) forms each entry stores
FORMS = {
    "f32": [(e, False, False) for e in (0, 1, 2, 3, 4)] + [(3, False, True)],
    "bf16": [(e, o, False) for e in (0, 1, 2, 4) for o in (False, True)] + [(3, False, False), (3, False, True)],
    "fp8": [(e, o, False) for e in (0, 1, 4) for o in (False, True)] + [(3, False, False), (3, False, True)],
    "mx8": [(e, o, False) for e in (0, 1, 4) for o in (False, True)] + [(3, False, False), (3, False, True), (3, True, False), (3, True, True)],
    "mx8q": [(e, False, False) for e in (0, 1, 4)],
}
FORMS["f32x3"] = FORMS["f32"]


def _operands(engine, fam, M, N, K, epi, out_bf16):
    """Contiguous device operands of one case + `base`, the fp64 value of A W^T + bias on the operands the kernel multiplies."""
    o = {"sa": None, "sw": None}
    if fam in ("f32", "f32x3"):
        a, w, b, r, base = R.f32_case(M, N, K)
    elif fam == "bf16":
        _, a, w, b, r, base = R.bf16_case(M, N, K, epi)
    elif fam == "fp8":
        a, o["sa"], w, o["sw"], b, r, base, _ = R.fp8_case(engine, M, N, K, epi)
    else:
        a, o["sa"], w, o["sw"], b, r, base, _ = R.mx8_case(engine, M, N, K, epi)
    if fam == "mx8" and epi == 3 and out_bf16:
        r = r.bfloat16()                                   # the bf16 residual stream
    o.update(a=a.to(DEV).contiguous(), w=w.to(DEV).contiguous(), b=b.to(DEV), r=r.to(DEV).contiguous(), r_cpu=r, base=base)
    return o


def _launch(engine, fam, M, N, K, epi, out_bf16, a, lda, w, ldw, bias, resid, c, ldc, sa=None, sra=0, sw=None, srw=0, sc=None, src=0):
    lib, h, st, ob = engine.lib, engine._h, _stream(), int(bool(out_bf16))
    if fam in ("f32", "f32x3"):
        code = lib.fern_gemm(h, a, lda, w, ldw, bias, resid, c, ldc, M, N, K, epi, st)
    elif fam == "bf16":
        code = lib.fern_gemm_bf16(h, a, lda, w, ldw, bias, resid, c, ldc, M, N, K, epi, ob, st)
    elif fam == "fp8":
        code = lib.fern_gemm_fp8(h, a, lda, sa, w, ldw, sw, bias, resid, c, ldc, M, N, K, epi, ob, st)
    elif fam == "mx8":
        code = lib.fern_gemm_mx8(h, a, lda, sa, sra, w, ldw, sw, srw, bias, resid, c, ldc, M, N, K, epi, ob, st)
    else:
        code = lib.fern_gemm_mx8_quant(h, a, lda, sa, sra, w, ldw, sw, srw, bias, c, ldc, sc, src, M, N, K, epi, st)
    _lib.check(code, f"{fam} gemm")


def _out_dtype(fam, out_bf16):
    return torch.uint8 if fam == "mx8q" else torch.bfloat16 if out_bf16 else torch.float32


def _contiguous_call(engine, fam, o, M, N, K, epi, out_bf16, inplace):
    """The entry on contiguous, unframed operands: lda = ldw = K, ldc = N, scale_rows = rows."""
    resid = o["r"] if epi == 3 else None
    c = o["r"].clone() if inplace else torch.empty(M, N, dtype=_out_dtype(fam, out_bf16), device=DEV)
    if inplace:
        resid = c
    sc = torch.empty(N // 128, M, 4, dtype=torch.uint8, device=DEV) if fam == "mx8q" else None
    _launch(engine, fam, M, N, K, epi, out_bf16, ptr(o["a"]), K, ptr(o["w"]), K, ptr(o["b"]), ptr(resid), ptr(c), N,
            ptr(o["sa"]), M, ptr(o["sw"]), N, ptr(sc), M)
    torch.cuda.synchronize()
    return c, sc


def _framed_call(engine, fam, o, M, N, K, epi, out_bf16, inplace, gap_mul=1):
    """The entry on framed, strided operands.  Returns (contiguous copy of the view, of the scale view or None); asserts (c)."""
    gap = GAP[fam] * gap_mul
    lda = ldw = K + gap
    ldc = N + 16 if fam == "mx8q" else N + 1               # N + 1: rows of odd length (2-byte aligned rows for bf16 outputs)
    fa, fw = framed_like(o["a"], lda, _moat(o["a"])), framed_like(o["w"], ldw, _moat(o["w"]))
    fb = framed_vec(o["b"], NAN)
    frames_in = [("A", fa), ("W", fw), ("bias", fb)]
    fsa = fsw = fsc = None
    sra = srw = src = 0
    if fam == "fp8":
        fsa, fsw = framed_vec(o["sa"], NAN), framed_vec(o["sw"], NAN)
    elif fam in ("mx8", "mx8q"):                           # E8M0 bytes [K/128, scale_rows, 4] with scale_rows = rows + 5
        sra, srw, src = M + 5, N + 5, M + 5
        fsa = Framed(K // 128, M * 4, sra * 4, torch.uint8, E8M0_HUGE, DEV).load(o["sa"].reshape(K // 128, M * 4))
        fsw = Framed(K // 128, N * 4, srw * 4, torch.uint8, E8M0_HUGE, DEV).load(o["sw"].reshape(K // 128, N * 4))
        if fam == "mx8q":
            fsc = Framed(N // 128, M * 4, src * 4, torch.uint8, SENTINEL, DEV)
    if fsa is not None:
        frames_in += [("scale_a", fsa), ("scale_w", fsw)]
    resid = None
    if inplace:                                            # residual == C: the stream is updated in place, inside an output frame
        fc = framed_like(o["r"], ldc, SENTINEL)
        resid = fc
    else:
        fc = Framed(M, N, ldc, _out_dtype(fam, out_bf16), SENTINEL, DEV)
        if epi == 3:
            resid = framed_like(o["r"], ldc, NAN)
            frames_in.append(("residual", resid))
    _launch(engine, fam, M, N, K, epi, out_bf16, ptr(fa), lda, ptr(fw), ldw, ptr(fb), ptr(resid), ptr(fc), ldc,
            ptr(fsa), sra, ptr(fsw), srw, ptr(fsc), src)
    torch.cuda.synchronize()
    what = f"{fam} M={M} N={N} K={K} epi={epi} out_bf16={out_bf16} inplace={inplace} lda={lda} ldc={ldc}"
    fc.assert_intact(f"C of {what}")
    if fsc is not None:
        fsc.assert_intact(f"scales_c of {what}")
    for name, f in frames_in:                              # inputs are read-only: not a byte of them or of their moats may change
        f.assert_intact(f"{name} (input) of {what}")
    return fc.contiguous(), (None if fsc is None else fsc.contiguous().reshape(N // 128, M, 4)), what


def _assert_finite(fam, got, sc, what):
    if fam == "mx8q":
        assert not ((got & 0x7F) == 0x7F).any(), f"{what}: NaN bytes in the e4m3fn output (something outside the operands was read)"
        assert not (sc == 0xFF).any(), f"{what}: NaN scale bytes"
    else:
        assert torch.isfinite(got.float()).all(), f"{what}: not finite (something outside the logical operands was read)"


def _check_reference(engine, fam, o, got, sc, M, N, K, epi, out_bf16):
    """(b): the contiguous result against the family's existing fp64 reference and bound."""
    ref = R.epi_ref(o["base"], epi, o["r_cpu"])
    if fam == "f32":
        R.close(got, ref)
    elif fam == "bf16":
        R.check_bf16_family(got, ref, out_bf16)
    elif fam == "fp8":
        R.check_fp8_family(got, ref, out_bf16)
    elif fam == "mx8":
        if epi == 1 and not out_bf16:
            # The block-scaled family's GELU is BY DEFINITION the tanh form x * sigmoid(2u) (gemm_epilogue.h: gelu_tanh2, up to 4.8e-4 from
            # the erf form: far below an e4m3 step, not below fp32).  test_gemm_mx8 sees it only through a bf16 rounding (atol 1e-3); an
            # fp32 output is held to the family's fp32 bound against the fp64 value of the form the family computes.
            ref = torch.nn.functional.gelu(o["base"], approximate="tanh")
        R.check_fp8_family(got, ref, out_bf16)
    else:      # mx8q: the quantiser applied to the fp32 output of fern_gemm_mx8, bit for bit (the existing test's statement)
        q_ref, s_ref = engine.quantize_mx8(engine.gemm_mx8(o["a"], o["sa"], o["w"], o["sw"], o["b"], epilogue=epi))
        assert torch.equal(sc, s_ref) and torch.equal(got, q_ref)


def _walk(engine, fam, M, N, K, gap_mul=1, reference=True, base=None):
    """Every stored form of the family at one shape.  `base`: {form: contiguous result} to compare against instead of a fresh contiguous
    call (the forced-tile walks compare every configuration with configuration 0)."""
    out = {}
    for epi, out_bf16, inplace in FORMS[fam]:
        o = _operands(engine, fam, M, N, K, epi, out_bf16)
        if base is None:
            ref_c, ref_s = _contiguous_call(engine, fam, o, M, N, K, epi, out_bf16, inplace)
        else:
            ref_c, ref_s = base[(epi, out_bf16, inplace)]
        got, sc, what = _framed_call(engine, fam, o, M, N, K, epi, out_bf16, inplace, gap_mul)
        assert_same_bits(got, ref_c, what)                                                         # (a)
        if sc is not None:
            assert_same_bits(sc, ref_s, "scales_c of " + what)
        _assert_finite(fam, got, sc, what)                                                   # (d)
        if reference and fam != "f32x3":
            _check_reference(engine, fam, o, ref_c, ref_s, M, N, K, epi, out_bf16)           # (b)
        out[(epi, out_bf16, inplace)] = (ref_c, ref_s)
    return out


@pytest.mark.parametrize("kmul", [1, 3])
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("fam", ["f32", "bf16", "fp8", "mx8"])
def test_gemm_frames(engine, fam, M, N, kmul):
    """fern_gemm / _bf16 / _fp8 / _mx8: lda = ldw = K + the smallest legal gap, ldc = N + 1, scale_rows = rows + 5, every stored
    epilogue with both output types, the in-place residual forms (fp32 residual == C; the block-scaled family's bf16 residual stream)
    included.  Assertions (a) - (d) of the module docstring."""
    _walk(engine, fam, M, N, KMIN[fam] * kmul)


@pytest.mark.parametrize("fam", ["f32", "bf16", "fp8", "mx8", "mx8q"])
def test_gemm_frames_with_a_wide_gap(engine, fam):
    """lda = ldw = K + 5 gaps, once per family: the stride is not the width plus one vector."""
    M, N = (300, 384) if fam == "mx8q" else (300, 520)
    _walk(engine, fam, M, N, KMIN[fam] * 3, gap_mul=5, reference=False)


@pytest.mark.parametrize("kmul", [1, 3])
@pytest.mark.parametrize("M,N", QUANT_SHAPES)
def test_gemm_mx8_quant_frames(engine, M, N, kmul):
    """fern_gemm_mx8_quant: e4m3fn bytes with ldc = N + 16 (16-byte stores per lane) and the E8M0 scale array with scale_rows_c = M + 5, both
    inside 0xA5 frames; (b) = the quantiser applied to fern_gemm_mx8's fp32 output, bit for bit."""
    _walk(engine, "mx8q", M, N, 128 * kmul)


@pytest.mark.parametrize("M,N", [(257, 129), (300, 520)])
def test_gemm_f32x3_frames(M, N):
    """FERN_PREC_F32X3 (its own engine, as the family's existing test): the split family serves M >= 256.  (a), (c), (d) per form, and (b)
    with the family's existing bound: the error against fp64 within 2x the fp32 kernel's own and below 1e-5 of the output rms."""
    from fashionern_aaai2024_amd.engine import FernEngine
    eng = FernEngine("cuda:0")
    try:
        for K in (32, 96):
            exact = {}
            for epi, out_bf16, inplace in FORMS["f32"]:
                o = _operands(eng, "f32", M, N, K, epi, out_bf16)
                exact[(epi, inplace)] = _contiguous_call(eng, "f32", o, M, N, K, epi, out_bf16, inplace)[0]
            eng.set_precision("f32x3")
            assert eng.precision == "f32x3"
            got = _walk(eng, "f32x3", M, N, K)
            eng.set_precision("fp32")
            for (epi, out_bf16, inplace), (x3, _) in got.items():
                o = _operands(eng, "f32", M, N, K, epi, out_bf16)
                ref = R.epi_ref(o["base"], epi, o["r_cpu"])
                rms = ref.pow(2).mean().sqrt().item()
                err_x3 = (x3.cpu().double() - ref).abs().max().item()
                err_f32 = (exact[(epi, inplace)].cpu().double() - ref).abs().max().item()
                assert err_x3 <= max(2.0 * err_f32, 2e-6 * rms) and err_x3 < 1e-5 * rms, (K, epi, err_x3, err_f32, rms)
    finally:
        eng.set_precision("fp32")
        eng.close()


# ---- forced tiles: the guards live in per-tile template instantiations ------------------------------------------------------------------
FORCED = {"f32": [0, 1, 2, 3, 6, 8, 9, 10, 11, 12, 13, 14, 15], "bf16": list(range(10)), "fp8": list(range(6)), "mx8": list(range(12))}


def _forced_walk(engine, family, fams, cfgs):
    """Each configuration of `family`, forced in process: the (33, 65) and (300, 520) cases ((33, 128) and (300, 384) for the quantising
    entry), (a) against configuration 0 and (c).  A configuration whose k tile does not divide K falls back by design."""
    shapes = {fam: ([(33, 128), (300, 384)] if fam == "mx8q" else [(33, 65), (300, 520)]) for fam in fams}
    base = {}
    try:
        for cfg in cfgs:
            engine.tuner_force_config(family, cfg)
            for fam in fams:
                for M, N in shapes[fam]:
                    for kmul in (1, 3):
                        key = (fam, M, N, kmul)
                        if cfg == cfgs[0]:
                            assert cfg == 0
                            base[key] = _walk(engine, fam, M, N, KMIN[fam] * kmul, reference=False)
                        else:
                            _walk(engine, fam, M, N, KMIN[fam] * kmul, reference=False, base=base[key])
    finally:
        engine.tuner_force_config(family, -1)


@pytest.mark.parametrize("family", ["f32", "bf16", "fp8"])
def test_every_forced_tile_honours_the_frame(engine, family):
    _forced_walk(engine, family, [family], FORCED[family])


def test_every_forced_block_scaled_tile_honours_the_frame(engine):
    """The block-scaled family: 0..11, the stored epilogues and the quantising one."""
    _forced_walk(engine, "mx8", ["mx8", "mx8q"], FORCED["mx8"])


def test_every_forced_f32x3_tile_honours_the_frame():
    """f32x3 0..7.  Forced through fern_tuner_force_config("f32x3"): a `tuner_import "f32x3 M N K epi cfg"` line is only consulted for
    launches of 2.5e8 flops or more (gemm.hip: launch_gemm_split), which these shapes are far below.  The family serves M >= 256 only:
    the (257, 129) and (300, 520) cases."""
    from fashionern_aaai2024_amd.engine import FernEngine
    eng = FernEngine("cuda:0")
    try:
        eng.set_precision("f32x3")
        base = {}
        for cfg in range(8):
            eng.tuner_force_config("f32x3", cfg)
            for M, N in ((257, 129), (300, 520)):
                for K in (32, 96):
                    if cfg == 0:
                        base[(M, N, K)] = _walk(eng, "f32x3", M, N, K)
                    else:
                        _walk(eng, "f32x3", M, N, K, base=base[(M, N, K)])
    finally:
        eng.tuner_force_config("f32x3", -1)
        eng.set_precision("fp32")
        eng.close()


@pytest.mark.parametrize("M,N,K", [(256, 520, 960), (300, 520, 832)])
def test_mixed_plans_honour_the_frame(engine, M, N, K):
    """One launch, three bands of rows (macro-tiles 256x128 `20` / 128x256 `21`, then 128x128, then 64x128 tiles), pinned through
    fern_tuner_import as test_mixed_geometry_plans_are_bit_identical does.  mixed_plan_ok (gemm.hip) wants rows_a a positive multiple of
    the macro-tile's 256 (`20`) or 128 (`21`) rows and rows_a <= cfg_b <= M, so M = 256 is the smallest M both kinds accept; a pinned
    plan is consulted only for launches of 2.5e8 flops or more (launch_gemm), hence K = 960.  M = 300 adds ragged last tiles in the second
    and third band."""
    plans = [(20, 256, 256), (20, 256, M), (21, 128, 128), (21, 128, 256), (21, 256, 256), (21, 128, M)]
    forms = FORMS["f32"]
    keys = sorted({11 if f[0] == 4 else f[0] for f in forms})      # the tuner's key holds the kernels' epilogue value: QUICKGELU is 11 there
    try:
        base = {}
        for epi in keys:
            engine.tuner_import(f"f32 {M} {N} {K} {epi} 0 8 0 8\n")
        for epi, out_bf16, inplace in forms:
            o = _operands(engine, "f32", M, N, K, epi, out_bf16)
            base[(epi, out_bf16, inplace)] = _contiguous_call(engine, "f32", o, M, N, K, epi, out_bf16, inplace)
        for cfg, ra, rb in plans:
            for epi in keys:
                engine.tuner_import(f"f32 {M} {N} {K} {epi} 0 {cfg} {ra} {rb}\n")
                assert f"f32 {M} {N} {K} {epi} 0 {cfg} {ra} {rb}" in engine.tuner_export(), "the plan was refused"
            _walk(engine, "f32", M, N, K, reference=False, base=base)
    finally:
        for epi in keys:
            engine.tuner_import(f"f32 {M} {N} {K} {epi} 0 8 0 8\n")


# ====================================================================================================================================
# attention
# ====================================================================================================================================
ATTN = [(2, 3, 64, 50, 50, 0), (2, 2, 80, 33, 33, 1), (2, 4, 32, 1, 40, 0), (1, 2, 16, 5, 40, 0), (1, 2, 96, 1, 224, 0),
        (1, 2, 64, 5, 300, 0)]      # b, heads, hd, s_q, s_k, causal: one per kernel form; the last one streams its keys (> 224)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("b,heads,hd,sq,sk,causal", ATTN)
def test_attention_frames(engine, b, heads, hd, sq, sk, causal, bf16):
    """fern_attention / fern_attention_bf16 in the towers' layout: Q, K, V are column slices of ONE packed [B * S, 3 W + gap] buffer
    (ldq = ldk = ldv = 3 W + gap); cross attention (s_q != s_k) reads Q from a [B * s_q, W + gap] buffer and K, V from a packed
    [B * s_k, 2 W + 2 gap] one; the output has ldo = W + gap.  gap = 4 floats / 8 bf16 elements.  Everything around the inputs is NaN,
    the rows after the last batch's K / V rows included: a masked key whose V row is NaN still poisons P V if the kernel reads past s_k
    instead of clamping.  Bit-identical to the contiguous call, which is within the existing tests' bounds (rel 2e-5 of the largest
    magnitude; 2^-7 max(1, |ref|) for bf16 operands) of fp64 attention; output frame intact; result finite."""
    dt, es, gap = (torch.bfloat16, 2, 8) if bf16 else (torch.float32, 4, 4)
    w = heads * hd
    g = torch.Generator().manual_seed(b * 100 + heads * 10 + hd + sq)
    q, k, v = (torch.randn(b, s, w, generator=g).to(dt) for s in (sq, sk, sk))
    scale = hd ** -0.5
    fn = engine.attention_bf16 if bf16 else engine.attention
    ref_c = fn(q.to(DEV), k.to(DEV), v.to(DEV), heads, causal=bool(causal), scale=scale).reshape(b * sq, w)
    ref = R.attn_ref(q, k, v, heads, bool(causal), scale).reshape(b * sq, w)
    if bf16:
        err = (ref_c.float().cpu().double() - ref).abs().max().item()
        assert err < 2 ** -7 * max(1.0, ref.abs().max().item()), err
    else:
        R.close(ref_c, ref, rel=2e-5)
    if sq == sk:
        ld = 3 * w + gap
        packed = Framed(b * sq, 3 * w, ld, dt, NAN, DEV).load(torch.cat([q, k, v], -1))
        ptrs = [(ptr(packed, i * w * es), ld) for i in range(3)]
        frames = [("packed QKV", packed)]
    else:
        fq = Framed(b * sq, w, w + gap, dt, NAN, DEV).load(q)
        fkv = Framed(b * sk, 2 * w, 2 * w + 2 * gap, dt, NAN, DEV).load(torch.cat([k, v], -1))
        ptrs = [(ptr(fq), w + gap), (ptr(fkv), 2 * w + 2 * gap), (ptr(fkv, w * es), 2 * w + 2 * gap)]
        frames = [("Q", fq), ("packed KV", fkv)]
    fo = Framed(b * sq, w, w + gap, dt, SENTINEL, DEV)
    entry = engine.lib.fern_attention_bf16 if bf16 else engine.lib.fern_attention
    (pq, ldq), (pk, ldk), (pv, ldv) = ptrs
    _lib.check(entry(engine._h, pq, ldq, pk, ldk, pv, ldv, ptr(fo), w + gap, b, heads, hd, sq, sk, causal, scale, _stream()), "attention")
    torch.cuda.synchronize()
    what = f"attention bf16={bf16} {(b, heads, hd, sq, sk, causal)}"
    fo.assert_intact("out of " + what)
    for name, f in frames:
        f.assert_intact(f"{name} (input) of {what}")
    got = fo.contiguous()
    assert torch.isfinite(got.float()).all(), f"{what}: not finite (a K / V row past s_k or a gap column was read into the result)"
    assert_same_bits(got, ref_c, what)


# ====================================================================================================================================
# quantisers
# ====================================================================================================================================
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", [1, 5, 197])
@pytest.mark.parametrize("d", [72, 768])
def test_quantize_rows_fp8_frames(engine, rows, d, bf16):
    """fern_quantize_rows_fp8 with ldx = ldy = d + 8: bytes and scales bit-identical to the contiguous call (pinned bit-exactly against
    torch by test_quantize_rows_fp8_is_bit_exact); y and scale frames intact; NaN in the gap columns of x."""
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g) * torch.logspace(-3, 3, rows).unsqueeze(1)
    x = (x.bfloat16() if bf16 else x).to(DEV)
    y_ref, s_ref = engine.quantize_rows_fp8(x)
    fx = framed_like(x, d + 8, NAN)
    fy = Framed(rows, d, d + 8, torch.uint8, SENTINEL, DEV)
    fs = Framed(1, rows, rows, torch.float32, SENTINEL, DEV)
    _lib.check(engine.lib.fern_quantize_rows_fp8(engine._h, ptr(fx), int(bf16), d + 8, ptr(fy), d + 8, ptr(fs), rows, d, _stream()), "quantize_rows_fp8")
    torch.cuda.synchronize()
    fy.assert_intact("y")
    fs.assert_intact("scale")
    fx.assert_intact("x (input)")
    assert_same_bits(fy.contiguous(), y_ref, "fp8 bytes")
    assert_same_bits(fs.contiguous()[0], s_ref, "row scales")
    assert torch.isfinite(fs.view).all() and not ((fy.view & 0x7F) == 0x7F).any()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", [1, 5, 197])
@pytest.mark.parametrize("d", [128, 640])
def test_quantize_mx8_frames(engine, rows, d, bf16):
    """fern_quantize_mx8 with ldx = ldy = d + 8 and scale_rows = rows + 5: as above (test_quantize_mx8_is_bit_exact pins the contiguous
    call); the scale bytes of rows >= `rows` are part of the frame."""
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g) * torch.logspace(-3, 3, rows).unsqueeze(1)
    x[:, 32:64] *= 50.0
    x = (x.bfloat16() if bf16 else x).to(DEV)
    y_ref, s_ref = engine.quantize_mx8(x)
    srows = rows + 5
    fx = framed_like(x, d + 8, NAN)
    fy = Framed(rows, d, d + 8, torch.uint8, SENTINEL, DEV)
    fs = Framed(d // 128, rows * 4, srows * 4, torch.uint8, SENTINEL, DEV)
    _lib.check(engine.lib.fern_quantize_mx8(engine._h, ptr(fx), int(bf16), d + 8, ptr(fy), d + 8, ptr(fs), srows, rows, d, _stream()), "quantize_mx8")
    torch.cuda.synchronize()
    fy.assert_intact("y")
    fs.assert_intact("scales")
    fx.assert_intact("x (input)")
    assert_same_bits(fy.contiguous(), y_ref, "e4m3fn bytes")
    assert_same_bits(fs.contiguous().reshape(d // 128, rows, 4), s_ref, "E8M0 scales")
    assert not ((fy.view & 0x7F) == 0x7F).any() and not (fs.view == 0xFF).any()


# ====================================================================================================================================
# the bf16 sweep
# ====================================================================================================================================
def _bands(t, fill=NAN):
    """A contiguous operand (no ld in the ABI) with a moat before its first and after its last row."""
    return framed_like(t, t.shape[1], fill)


@pytest.mark.parametrize("B", [3, 65])
@pytest.mark.parametrize("N", [33, 1000])
def test_sweep_bf16_scores_frames(engine, B, N):
    """fern_sweep_bf16_scores with ld = N + 7 (the entry asks for ld >= N only) and ldt = ceil(N / 32) + 3: scores and tile maxima
    bit-identical to the contiguous call, both output frames intact, NaN after the last gallery row and the last query."""
    D = 64
    q, gal = unit(B, D, 41).to(DEV), unit(N, D, 42).to(DEV)
    pg = engine.prepare_gallery(gal)
    s_ref, t_ref = engine.sweep_bf16_scores(q, pg)
    nt = (N + 31) // 32
    fq, fg = _bands(q), _bands(pg.bf16)
    fs = Framed(B, N, N + 7, torch.float32, SENTINEL, DEV)
    ft = Framed(B, nt, nt + 3, torch.float32, SENTINEL, DEV)
    _lib.check(engine.lib.fern_sweep_bf16_scores(engine._h, ptr(fq), ptr(fg), B, N, D, ptr(fs), N + 7, ptr(ft), nt + 3, _stream()), "sweep")
    torch.cuda.synchronize()
    fs.assert_intact("scores")
    ft.assert_intact("tile_max")
    fq.assert_intact("q (input)")
    fg.assert_intact("gallery (input)")
    assert torch.isfinite(fs.view).all() and torch.isfinite(ft.view).all()
    assert_same_bits(fs.contiguous(), s_ref, "scores")
    assert_same_bits(ft.contiguous(), t_ref, "tile maxima")


# ====================================================================================================================================
# ranking outputs [B, K]
# ====================================================================================================================================
RANK_N, RANK_D = 100, 64


def _rank_inputs(engine, B):
    q, gal = unit(B, RANK_D, 51 + B).to(DEV), unit(RANK_N, RANK_D, 52).to(DEV)
    return q, gal, engine.prepare_gallery(gal)


def _rank_frames(B, K):
    return Framed(B, K, K, torch.float32, SENTINEL, DEV), Framed(B, K, K, torch.int32, SENTINEL, DEV)


def _rank_check(fs, fi, ref, what):
    torch.cuda.synchronize()
    fs.assert_intact("out_scores of " + what)      # the bytes right after row B - 1 are what a 16-byte store of a ragged row would hit
    fi.assert_intact("out_idx of " + what)
    assert_same_bits(fs.contiguous(), ref[0], "scores of " + what)
    assert_same_bits(fi.contiguous(), ref[1], "indices of " + what)


RANK_CASES = [(3, 1), (3, 7), (3, 51), (1030, 7)]            # (B, K); B = 1030 crosses the 1024-query plan chunk
DEEP_CASES = [(3, 65), (3, 1000), (1030, 65)]


@pytest.mark.parametrize("B,K", RANK_CASES)
def test_sim_topk_output_frames(engine, B, K):
    """fern_sim_topk, fern_sim_topk_bf16 and fern_sim_topk_prefiltered (LISTS and DENSE) write [B, K] rows of odd length into framed
    outputs (ld = K, bands only): equal to the engine wrapper's result on the same inputs (pinned against the oracles elsewhere), nothing
    before row 0 or after row B - 1 written.  Queries and galleries sit in NaN moats."""
    lib, h = engine.lib, engine._h
    q, gal, pg = _rank_inputs(engine, B)
    fq, fg, fg16 = _bands(q), _bands(gal), _bands(pg.bf16)
    ref = engine.sim_topk(q, gal, K)
    fs, fi = _rank_frames(B, K)
    _lib.check(lib.fern_sim_topk(h, ptr(fq), ptr(fg), B, RANK_N, RANK_D, K, ptr(fs), ptr(fi), 0, None, _stream()), "fern_sim_topk")
    _rank_check(fs, fi, ref, f"fern_sim_topk B={B} K={K}")
    ref = engine.sim_topk_bf16(q, pg.bf16, K)
    fs, fi = _rank_frames(B, K)
    _lib.check(lib.fern_sim_topk_bf16(h, ptr(fq), ptr(fg16), B, RANK_N, RANK_D, K, ptr(fs), ptr(fi), 0, None, _stream()), "fern_sim_topk_bf16")
    _rank_check(fs, fi, ref, f"fern_sim_topk_bf16 B={B} K={K}")
    try:
        for strategy in ("lists", "dense"):
            engine.set_rank_strategy(strategy)
            ref = engine.sim_topk(q, pg, K)
            fs, fi = _rank_frames(B, K)
            _lib.check(lib.fern_sim_topk_prefiltered(h, ptr(fq), ptr(fg), ptr(fg16), ptr(pg.meta), B, RANK_N, RANK_D, K, ptr(fs), ptr(fi), 0, None,
                                                     _stream()), "fern_sim_topk_prefiltered")
            _rank_check(fs, fi, ref, f"fern_sim_topk_prefiltered ({strategy}) B={B} K={K}")
    finally:
        engine.set_rank_strategy("auto")
    for f in (fq, fg, fg16):
        f.assert_intact("a ranking input")


@pytest.mark.parametrize("B,K", DEEP_CASES)
def test_sim_topk_deep_output_frames(engine, B, K):
    """fern_sim_topk_deep, every gallery form (fp32 only; fp32 + bf16 copy + meta; bf16 only), K in {65, 1000} -- K = 1000 > N: the unfilled
    places are written too, and only they."""
    lib, h = engine.lib, engine._h
    q, gal, pg = _rank_inputs(engine, B)
    fq, fg, fg16 = _bands(q), _bands(gal), _bands(pg.bf16)
    for name, wrapper_gallery, args in (("fp32", gal, (ptr(fg), None, None)), ("prepared", pg, (ptr(fg), ptr(fg16), ptr(pg.meta))),
                                        ("bf16", pg.bf16, (None, ptr(fg16), None))):
        ref = engine.sim_topk_deep(q, wrapper_gallery, K)
        fs, fi = _rank_frames(B, K)
        _lib.check(lib.fern_sim_topk_deep(h, ptr(fq), *args, B, RANK_N, RANK_D, K, ptr(fs), ptr(fi), 0, None, _stream()), "fern_sim_topk_deep")
        _rank_check(fs, fi, ref, f"fern_sim_topk_deep ({name}) B={B} K={K}")
    for f in (fq, fg, fg16):
        f.assert_intact("a ranking input")


@pytest.mark.parametrize("B,K", RANK_CASES + DEEP_CASES)
def test_topk_merge_output_frames(engine, B, K):
    """fern_topk_merge of R = 2 shard lists, K <= 64 and K > 64 (two kernels)."""
    q, gal, _ = _rank_inputs(engine, B)
    top = engine.sim_topk_deep if K > 64 else engine.sim_topk
    parts = [top(q, gal[lo:hi].contiguous(), K, idx_offset=lo) for lo, hi in ((0, 37), (37, RANK_N))]
    s, i = torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])
    ref = engine.topk_merge(s, i)
    fin_s = Framed(2 * B, K, K, torch.float32, NAN, DEV).load(s.reshape(2 * B, K))
    fin_i = Framed(2 * B, K, K, torch.int32, SENTINEL, DEV).load(i.reshape(2 * B, K))
    fs, fi = _rank_frames(B, K)
    _lib.check(engine.lib.fern_topk_merge(engine._h, ptr(fin_s), ptr(fin_i), ptr(fs), ptr(fi), 2, B, K, _stream()), "fern_topk_merge")
    _rank_check(fs, fi, ref, f"fern_topk_merge B={B} K={K}")
    fin_s.assert_intact("shard scores (input)")
    fin_i.assert_intact("shard indices (input)")


@pytest.mark.parametrize("B,m", RANK_CASES)
def test_gather_scores_output_frame(engine, B, m):
    q, gal, _ = _rank_inputs(engine, B)
    g = torch.Generator().manual_seed(B + m)
    idx = torch.randint(-1, RANK_N, (B, m), generator=g, dtype=torch.int32).to(DEV)      # -1: -inf
    ref = engine.gather_scores(q, gal, idx)
    fq, fg = _bands(q), _bands(gal)
    fidx = Framed(B, m, m, torch.int32, 0xFF, DEV).load(idx)                              # moat of -1 indices
    fo = Framed(B, m, m, torch.float32, SENTINEL, DEV)
    _lib.check(engine.lib.fern_gather_scores(engine._h, ptr(fq), ptr(fg), ptr(fidx), ptr(fo), B, m, RANK_D, _stream()), "fern_gather_scores")
    torch.cuda.synchronize()
    fo.assert_intact(f"out of fern_gather_scores B={B} m={m}")
    assert_same_bits(fo.contiguous(), ref, "gathered scores")

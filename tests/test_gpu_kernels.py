"""Kernel-level parity through the C ABI (fern_gemm / fern_layernorm / fern_attention / rank ops)
against plain torch fp32/fp64 CPU references of the same op."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_refs
from gemm_refs import attn_ref as _attn_ref, close as _close, mx_scales_by_block as _mx_scales_by_block, rand as _rand
from oracle import rank as orank
from support import assert_same_order_up_to_near_ties, int_unit

pytestmark = pytest.mark.gpu


GEMM_SHAPES = [(64, 64, 32), (1, 32, 32), (100, 130, 64), (37, 200, 96), (300, 768, 768), (129, 513, 128),
               (1000, 3072, 256), (700, 64, 3072), (64, 4096, 512), (257, 129, 32)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("epi", [0, 1, 2, 3])
def test_gemm_matches_torch(engine, M, N, K, epi):
    a, w, b, r, base = gemm_refs.f32_case(M, N, K)
    got = engine.gemm(a, w, b, residual=r if epi == 3 else None, epilogue=epi)
    _close(got, gemm_refs.epi_ref(base, epi, r))


def test_gemm_exact_on_integer_data(engine):
    """Small-integer operands make every partial sum exact in fp32: any k-order must give identical bits.
    Asymmetric W catches a transposed C write."""
    g = torch.Generator().manual_seed(7)
    a = torch.randint(-3, 4, (193, 160), generator=g).float()
    w = torch.randint(-3, 4, (77, 160), generator=g).float()
    got = engine.gemm(a, w).cpu()
    assert torch.equal(got, a @ w.T)
    eye = torch.eye(64)
    w2 = torch.arange(64 * 64, dtype=torch.float32).reshape(64, 64) % 251
    assert torch.equal(engine.gemm(eye, w2).cpu(), w2.T)


def test_gemm_no_bias(engine):
    a, w = _rand(50, 64, seed=5), _rand(70, 64, seed=6)
    _close(engine.gemm(a, w), a.double() @ w.double().T)


@pytest.mark.parametrize("rows,d", [(1, 128), (7, 512), (33, 640), (1000, 768), (5, 192), (3, 1024)])
def test_layernorm(engine, rows, d):
    x, g, b, r = _rand(rows, d, seed=1, scale=3.0) + 0.7, _rand(d, seed=2), _rand(d, seed=3), _rand(rows, d, seed=4)
    for eps in (1e-5, 1e-12):
        _close(engine.layernorm(x, g, b, eps), F.layer_norm(x.double(), (d,), g.double(), b.double(), eps), rel=1e-5)
    _close(engine.layernorm(x, g, b, 1e-12, residual=r), F.layer_norm((x + r).double(), (d,), g.double(), b.double(), 1e-12), rel=1e-5)


ATTN_CASES = [  # batch, heads, hd, s_q, s_k, causal
    (2, 12, 64, 197, 197, False), (3, 8, 64, 77, 77, True), (2, 8, 64, 91, 91, False), (2, 8, 80, 91, 91, False),
    (3, 8, 16, 91, 91, False), (2, 8, 64, 13, 13, False), (2, 8, 80, 13, 13, False), (2, 4, 32, 17, 17, False),
    (2, 3, 64, 10, 10, False), (2, 4, 32, 77, 77, True), (1, 2, 64, 77, 77, True), (2, 10, 64, 77, 77, True),
    (1, 1, 32, 33, 33, True), (2, 2, 16, 5, 40, False), (1, 12, 64, 224, 224, False), (2, 8, 16, 13, 13, False),
    (1, 3, 64, 77, 77, True), (2, 2, 96, 70, 70, True), (2, 10, 80, 77, 77, True),      # odd head count, head dims 96 / 80 on the causal 3-tile shape
    (2, 12, 64, 1, 197, False), (3, 8, 32, 1, 40, False), (1, 2, 64, 1, 1000, False), (2, 3, 16, 1, 1, False),      # one query per head (the class token's block)
    (1, 2, 80, 1, 50, False), (1, 2, 96, 1, 224, False)]                                 # ... and beyond its head dimension: the tiled kernels


@pytest.mark.parametrize("b,heads,hd,sq,sk,causal", ATTN_CASES)
def test_attention(engine, b, heads, hd, sq, sk, causal):
    w = heads * hd
    q, k, v = _rand(b, sq, w, seed=1), _rand(b, sk, w, seed=2), _rand(b, sk, w, seed=3)
    scale = hd ** -0.5
    _close(engine.attention(q, k, v, heads, causal=causal, scale=scale), _attn_ref(q, k, v, heads, causal, scale), rel=2e-5)


def test_attention_sharp_softmax(engine):
    """Large logits: the running-max rescale path of the online softmax must be exact when the max moves
    between key tiles (spike placed in the last tile)."""
    b, heads, hd, s = 1, 2, 64, 197
    w = heads * hd
    q, k, v = _rand(b, s, w, seed=4), _rand(b, s, w, seed=5), _rand(b, s, w, seed=6)
    k[:, 190] = q[:, 5] * 4.0          # query 5 sees a huge score at key 190 (tile 5) after small ones
    k[:, 3] = q[:, 100] * 4.0          # and query 100 at key 3 (tile 0)
    _close(engine.attention(q, k, v, heads, scale=1.0), _attn_ref(q, k, v, heads, False, 1.0), rel=5e-5)


@pytest.mark.parametrize("B,N,D,K", [(5, 1000, 64, 50), (64, 9001, 128, 51), (3, 40, 32, 50), (2, 64, 32, 64),
                                      (1, 1, 32, 1), (7, 20000, 64, 10), (130, 3000, 64, 50)])
def test_sim_topk_bit_exact_with_ties(engine, B, N, D, K):
    q, g = int_unit(B, D, 1), int_unit(N, D, 2)
    rs, ri = orank.cosine_topk(q, g, K)
    s, i = engine.sim_topk(q, g, K)
    assert torch.equal(i.cpu(), ri), "index order differs (tie rule: score desc, index asc)"
    assert torch.equal(s.cpu(), rs)


def test_sim_topk_offset_and_exclude(engine):
    q, g = int_unit(9, 64, 3), int_unit(777, 64, 4)
    ex = torch.tensor([1000 + 5, -1, 1000 + 776, 3, 1000, 1000 + 100, -1, 1000 + 1, 1000 + 2], dtype=torch.int32)
    rs, ri = orank.cosine_topk(q, g, 51, idx_offset=1000, exclude_idx=ex)
    s, i = engine.sim_topk(q, g, 51, idx_offset=1000, exclude_idx=ex)
    assert torch.equal(i.cpu(), ri) and torch.equal(s.cpu(), rs)


def test_sim_topk_random_unit_rows(engine):
    """C2's shape on random unit rows.  Against the fma-chain oracle (oracle/chain.c: the sweep's exact fp32 summation order)
    scores AND ordering are bit-identical; against the BLAS-ordered torch oracle scores agree to 1e-5 (north_star: 1e-3) and a
    swap is tolerated only between neighbours the oracle itself separates by less than 2e-6."""
    from fashionern_aaai2024_amd import synth
    from oracle import chain
    q, g = torch.from_numpy(synth.unit_rows(64, 512, tag="q")), torch.from_numpy(synth.unit_rows(46000, 512, tag="g"))
    s, i = engine.sim_topk(q, g, 50)
    s, i = s.cpu(), i.cpu()
    cs, ci = chain.chain_topk(q.numpy(), g.numpy(), 50)
    assert np.array_equal(i.numpy(), ci), "top-50 order differs from the fma-chain restatement of the sweep"
    assert np.array_equal(s.numpy().view(np.uint32), cs.view(np.uint32)), "scores are not bit-identical to the fma chain"
    rs, ri = orank.cosine_topk(q, g, 50)
    assert (s - rs).abs().max().item() < 1e-5
    full = q @ g.T
    assert_same_order_up_to_near_ties(full, i, ri, gap=2e-6)


@pytest.mark.parametrize("B,N,D", [(3, 1000, 64), (64, 9001, 640), (130, 3000, 128), (1, 70_000, 512)])
def test_sim_topk_bit_identical_to_the_fma_chain(engine, B, N, D):
    """Every tile configuration the tuner may pick adds an element's products in the same k order (gemm.hip), and that order is
    what oracle/chain.c restates: random operands, any shape -> identical bits, identical ranking."""
    from oracle import chain
    q, g = _rand(B, D, seed=B + N), _rand(N, D, seed=N + D, scale=D ** -0.5)
    s, i = engine.sim_topk(q, g, 50)
    cs, ci = chain.chain_topk(q.numpy(), g.numpy(), 50)
    assert np.array_equal(i.cpu().numpy(), ci) and np.array_equal(s.cpu().numpy().view(np.uint32), cs.view(np.uint32))
    full = torch.from_numpy(chain.chain_scores(q.numpy(), g.numpy()))
    assert torch.equal(engine.gemm(q, g).cpu(), full), "the plain GEMM epilogue sees the same accumulators"


def test_gather_scores_and_merge(engine):
    q, g = int_unit(6, 64, 5), int_unit(300, 64, 6)
    idx = torch.tensor([[0, 5, 299, -1, 7, 7]] * 6, dtype=torch.int32)
    assert torch.equal(engine.gather_scores(q, g, idx).cpu(), orank.gather_scores(q, g, idx))
    # shard the gallery 3 ways, top-K per shard with offsets, merge == global top-K
    parts = [(0, 100), (100, 250), (250, 300)]
    ss, ii = zip(*[engine.sim_topk(q, g[a:b], 20, idx_offset=a) for a, b in parts])
    ms, mi = engine.topk_merge(torch.stack(ss), torch.stack(ii))
    rs, ri = orank.cosine_topk(q, g, 20)
    assert torch.equal(mi.cpu(), ri) and torch.equal(ms.cpu(), rs)
    os_, oi = orank.topk_merge(torch.stack(ss).cpu(), torch.stack(ii).cpu())
    assert torch.equal(oi, ri) and torch.equal(os_, rs)


def test_l2_normalize(engine):
    x = _rand(100, 512, seed=9)
    x[3] = 0
    _close(engine.l2_normalize(x), F.normalize(x.double(), dim=-1), rel=1e-6)


def test_empty_and_degenerate_inputs(engine):
    """Zero-sized batches / galleries are legal (a rank's gallery shard can be empty) and must not launch garbage."""
    q, g = int_unit(4, 64, 1), int_unit(10, 64, 2)
    s, i = engine.sim_topk(q, g[:0], 5)
    assert (i.cpu() == -1).all() and torch.isinf(s.cpu()).all() and (s.cpu() < 0).all()
    s, i = engine.sim_topk(q[:0], g, 5)
    assert s.shape == (0, 5) and i.shape == (0, 5)
    assert engine.gemm(torch.zeros(0, 64), torch.zeros(8, 64)).shape == (0, 8)
    assert engine.l2_normalize(torch.zeros(0, 64)).shape == (0, 64)
    # K larger than the gallery: the tail is (-inf, -1), the head is the full ranking
    s, i = engine.sim_topk(q, g, 64)
    rs, ri = orank.cosine_topk(q, g, 64)
    assert torch.equal(i.cpu(), ri) and torch.equal(s.cpu(), rs)


def test_bad_arguments_are_reported_not_executed(engine):
    from fashionern_aaai2024_amd._lib import FernError
    with pytest.raises(FernError, match="K"):
        engine.sim_topk(int_unit(2, 64, 1), int_unit(10, 64, 2), 65)
    with pytest.raises(FernError, match="multiple of 32"):
        engine.gemm(torch.zeros(4, 48), torch.zeros(4, 48))
    with pytest.raises(ValueError):
        engine.sim_topk(int_unit(2, 64, 1), int_unit(10, 32, 2), 5)
    # ld < width makes rows overlap and stores race: FERN_ERR_ARG before any launch, and the framed output stays untouched
    import ctypes as C
    from framed import SENTINEL, Framed
    from fashionern_aaai2024_amd.engine import _stream
    lib, h, st = engine.lib, engine._h, _stream()
    M, N = 8, 32
    out = Framed(M, N, N, torch.float32, SENTINEL, "cuda")
    out.view.fill_(7.0)
    before = out.flat.clone()
    z = torch.zeros(64 * 512, dtype=torch.float32, device="cuda")      # operands large enough for any of the shapes below
    one = torch.ones(64, dtype=torch.float32, device="cuda")
    po, pz, p1 = C.c_void_p(out.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(one.data_ptr())

    def refused(code, what):
        torch.cuda.synchronize()
        assert code == -1, f"{what}: expected FERN_ERR_ARG, got {code}"
        assert "ld" in lib.fern_last_error().decode(), what
        assert torch.equal(out.flat.view(torch.int32), before.view(torch.int32)), f"{what}: the refused call wrote to its output"

    for fam, K, step in (("f32", 32, 4), ("bf16", 32, 8), ("fp8", 64, 16), ("mx8", 128, 16), ("mx8q", 128, 16)):
        n = 128 if fam == "mx8q" else N
        for lda, ldw, ldc in ((K - step, K, n), (K, K - step, n), (K, K, n - (16 if fam == "mx8q" else 1))):
            if fam == "f32":
                code = lib.fern_gemm(h, pz, lda, pz, ldw, None, None, po, ldc, M, n, K, 0, st)
            elif fam == "bf16":
                code = lib.fern_gemm_bf16(h, pz, lda, pz, ldw, None, None, po, ldc, M, n, K, 0, 0, st)
            elif fam == "fp8":
                code = lib.fern_gemm_fp8(h, pz, lda, p1, pz, ldw, p1, None, None, po, ldc, M, n, K, 0, 0, st)
            elif fam == "mx8":
                code = lib.fern_gemm_mx8(h, pz, lda, pz, M, pz, ldw, pz, n, None, None, po, ldc, M, n, K, 0, 0, st)
            else:
                code = lib.fern_gemm_mx8_quant(h, pz, lda, pz, M, pz, ldw, pz, n, None, po, ldc, pz, M, M, n, K, 0, st)
            refused(code, f"{fam} gemm lda={lda} ldw={ldw} ldc={ldc}")
    heads, hd, s = 2, 16, 4
    w = heads * hd
    for name, entry, g in (("fern_attention", lib.fern_attention, 4), ("fern_attention_bf16", lib.fern_attention_bf16, 8)):
        for bad in range(4):
            lds = [w - g if i == bad else w for i in range(4)]
            refused(entry(h, pz, lds[0], pz, lds[1], pz, lds[2], po, lds[3], 1, heads, hd, s, s, 0, 1.0, st), f"{name} ldq, ldk, ldv, ldo = {lds}")
    for ldx, ldy in ((56, 64), (64, 56)):
        refused(lib.fern_quantize_rows_fp8(h, pz, 0, ldx, po, ldy, pz, 4, 64, st), f"fern_quantize_rows_fp8 ldx={ldx} ldy={ldy}")
    for ldx, ldy in ((120, 128), (128, 120)):
        refused(lib.fern_quantize_mx8(h, pz, 0, ldx, po, ldy, pz, 4, 4, 128, st), f"fern_quantize_mx8 ldx={ldx} ldy={ldy}")
    out.assert_intact("the output frame of the refused calls")


def test_topk_large_gallery_many_segments(engine):
    """200k rows = 25 level-1 segments per query; merge must still be exact (ties included)."""
    q, g = int_unit(3, 32, 11), int_unit(200_000, 32, 12)
    rs, ri = orank.cosine_topk(q, g, 51)
    s, i = engine.sim_topk(q, g, 51)
    assert torch.equal(i.cpu(), ri) and torch.equal(s.cpu(), rs)


# ---- forced tile variants ---------------------------------------------------------------------------------------------------------
# Every tile configuration of a family gives the same bits, and the launcher picks (or tunes) one per shape -- so each variant is also
# FORCED over its family's whole shape / epilogue suite.  One pytest child process per family walks all of that family's variants:
# FERN_TEST_FORCE="family:c0,c1,..." makes the autouse fixture below parametrise every selected test over the configurations and force
# each through fern_tuner_force_config (rounds 2-4 forced them through environment variables the library read once per process: 37
# children, ~400 s of interpreter start-up).  Marked `slow`; tests/conftest.py runs `slow` tests last.
_FORCE = os.environ.get("FERN_TEST_FORCE", "")


def pytest_generate_tests(metafunc):
    if _FORCE and "forced_tile" in metafunc.fixturenames:
        family, cfgs = _FORCE.split(":")
        metafunc.parametrize("forced_tile", [(family, int(c)) for c in cfgs.split(",")], indirect=True,
                             ids=[f"{family}{c}" for c in cfgs.split(",")])


@pytest.fixture(autouse=True)
def forced_tile(request):
    param = getattr(request, "param", None)
    if param is None:
        yield None
        return
    from fashionern_aaai2024_amd import _lib
    lib = _lib.load()
    family, cfg = param
    _lib.check(lib.fern_tuner_force_config(family.encode(), cfg), "fern_tuner_force_config")
    try:
        yield param
    finally:
        lib.fern_tuner_force_config(family.encode(), -1)


def _forced_family_result(family, cfgs, key):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FERN_TEST_FORCE=f"{family}:{','.join(str(c) for c in cfgs)}")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_kernels.py", "-m", "gpu and not slow", "-q", "-x", "-k", key,
                        "-p", "no:cacheprovider"], cwd=root, env=env, capture_output=True, text=True, timeout=1500)
    import re
    m = re.search(r"(\d+) passed", r.stdout)
    assert r.returncode == 0 and m, r.stdout[-3000:]
    assert int(m.group(1)) >= 10 * len(cfgs), f"the suite was not walked once per configuration: {r.stdout[-500:]}"
    return r


@pytest.mark.slow
def test_every_gemm_tile_variant_passes_the_shape_suite():
    """fp32 family: the whole GEMM shape / epilogue suite, incl. the integer-exactness test, under each of the 13 forced configurations."""
    r = _forced_family_result("f32", [0, 1, 2, 3, 6, 8, 9, 10, 11, 12, 13, 14, 15], "test_gemm and not bf16 and not fp8 and not mx8")
    assert r.returncode == 0


@pytest.mark.parametrize("m,n,k", [(3000, 768, 768), (2500, 700, 256), (4100, 1536, 512)])
def test_mixed_geometry_plans_are_bit_identical(engine, m, n, k):
    """One launch, three bands of rows -- 8-wave macro-tiles (256x128 or 128x256), 128x128, 64x128 -- cut at arbitrary legal rows
    (plans pinned through fern_tuner_import): every plan must give the bits of the plain 128x128 configuration, ragged last tiles,
    empty bands and every row-independent epilogue included."""
    a, w, b, r = _rand(m, k, seed=21), _rand(n, k, seed=22, scale=k ** -0.5), _rand(n, seed=23), _rand(m, n, seed=24)
    hi = (m // 256) * 256
    plans = [(20, hi, m), (20, hi, hi), (20, 1024, 1024 + ((m - 1024) // 128) * 128), (20, 256, 256), (20, 512, m),
             (21, (m // 128) * 128, m), (21, 1152, 2048), (21, 128, 128), (21, 2048, 2048 + 256)]
    # bulk + remainder pairs (two launches): rows [0, ra) on `cfg`, the rest on `rb` -- incl. the 16x16-tile kernel (6) as the remainder
    # of 64x64 / 64x128 / 128x64 bulks (k % 64 == 0), a ragged last row block included
    plans += [(8, 1024, 11), (12, 2048, 8)] + ([(11, 2048, 6), (9, 1984, 6), (10, 1280, 6)] if k % 64 == 0 else [])
    for epi in (0, 1, 2, 3):
        run = lambda: engine.gemm(a, w, b, residual=r if epi == 3 else None, epilogue=epi).cpu()  # noqa: E731
        engine.tuner_import(f"f32 {m} {n} {k} {epi} 0 8 0 8\n")
        base = run()
        for cfg, ra, rb in plans:
            engine.tuner_import(f"f32 {m} {n} {k} {epi} 0 {cfg} {ra} {rb}\n")
            assert f"f32 {m} {n} {k} {epi} 0 {cfg} {ra} {rb}" in engine.tuner_export(), "the plan was refused"
            assert torch.equal(run(), base), (epi, cfg, ra, rb)
        engine.tuner_import(f"f32 {m} {n} {k} {epi} 0 8 0 8\n")


@pytest.mark.parametrize("m,n,k", [(1000, 520, 256), (4096, 768, 768), (300, 96, 64)])
def test_gemm_f32x3_is_fp32_accurate_and_configuration_independent(m, n, k):
    """FERN_PREC_F32X3: fp32 operands as three bf16 planes (truncation split in registers), six bf16 MFMAs per pair of fp32 ones.
    Tolerance: the error against double-precision arithmetic must stay within 2x the fp32 MFMA kernel's own and below 1e-5 of the output
    rms.  All six tile configurations of the family are bit-identical (pinned through fern_tuner_import), a row's bits do not depend on
    the batch it travels in, and shapes below 256 rows run the exact fp32 kernels."""
    from fashionern_aaai2024_amd.engine import FernEngine
    eng = FernEngine("cuda:0")
    a, w, b, r = _rand(m, k, seed=31), _rand(n, k, seed=32, scale=k ** -0.5), _rand(n, seed=33), _rand(m, n, seed=34)
    for epi in (0, 1, 2, 3):
        ref = a.double() @ w.double().T + b.double()
        ref = F.gelu(ref) if epi == 1 else F.relu(ref) if epi == 2 else ref + r.double() if epi == 3 else ref
        run = lambda: eng.gemm(a, w, b, residual=r if epi == 3 else None, epilogue=epi).cpu()  # noqa: E731
        eng.set_precision("fp32")
        exact = run()
        eng.set_precision("f32x3")
        assert eng.precision == "f32x3"
        outs = []
        for cfg in range(8):
            eng.tuner_import(f"f32x3 {m} {n} {k} {epi} {cfg}\n")
            outs.append(run())
        if m >= 2048:      # one-launch mixed plans of the family (fat-wave macro-tiles + 128x128 + 64x128 bands)
            for cfg, ra, rb in ((20, 2048, m), (20, 3840, 3840), (21, 1920, 3072), (21, 4096, 4096)):
                eng.tuner_import(f"f32x3 {m} {n} {k} {epi} {cfg} {ra} {rb}\n")
                assert f"f32x3 {m} {n} {k} {epi} {cfg} {ra} {rb}" in eng.tuner_export(), "the plan was refused"
                outs.append(run())
        for o in outs[1:]:
            assert torch.equal(o, outs[0]), "f32x3 tile configurations must be bit-identical"
        rms = ref.pow(2).mean().sqrt().item()
        err_x3 = (outs[0].double() - ref).abs().max().item()
        err_f32 = (exact.double() - ref).abs().max().item()
        assert err_x3 <= max(2.0 * err_f32, 2e-6 * rms) and err_x3 < 1e-5 * rms, (epi, err_x3, err_f32, rms)
        lo, hi = 17, 17 + 256                                   # a 256-row slice is still served by the split family
        part = eng.gemm(a[lo:hi], w, b, residual=r[lo:hi] if epi == 3 else None, epilogue=epi).cpu()
        assert torch.equal(part, outs[0][lo:hi]), "batch invariance"
        small = eng.gemm(a[:100], w, b, residual=r[:100] if epi == 3 else None, epilogue=epi).cpu()
        assert torch.equal(small, exact[:100]), "fewer than 256 rows: the exact fp32 kernels"
    eng.close()


def test_gemm_variants_are_bit_identical(engine):
    """Same k summation order in every tile shape: forcing nothing but changing M (which changes the tuned tile) must not
    change a row's bits."""
    a, w, b = _rand(3000, 768, seed=11), _rand(768, 768, seed=12, scale=768 ** -0.5), _rand(768, seed=13)
    full = engine.gemm(a, w, b, epilogue=1).cpu()
    for lo, hi in ((0, 1), (0, 64), (100, 1124), (2990, 3000)):
        assert torch.equal(engine.gemm(a[lo:hi], w, b, epilogue=1).cpu(), full[lo:hi])


@pytest.mark.parametrize("family,m,n,k", [("f32", 320, 512, 1024), ("f32", 2112, 256, 256), ("f32x3", 320, 512, 1024), ("f32x3", 2112, 256, 256),
                                          ("bf16", 320, 512, 1024), ("fp8", 320, 512, 1024), ("mx8", 320, 512, 1024)])
def test_first_sight_of_a_shape_is_tuned_once_and_stored_as_one_line(engine, family, m, n, k):
    """The first unforced call of a shape inside the tuning window times the family's candidates and stores ONE choice: one new export
    line of the family's kind under the shape's key, which an import accepts back; the result has the bits of a forced configuration
    (a forced call tunes nothing and stores nothing), and later calls neither add a line nor change a bit.  320 x 512 x 1024 (3.4e8 flop,
    just over the 2.5e8 floor) is ragged against every tile height; 2112 x 256 x 256 (2.8e8 flop, M >= 2048) also brings the bulk +
    remainder and mixed plans into the fp32 trials.  No other test uses these two shapes: the tuner's state is process-wide."""
    from fashionern_aaai2024_amd.engine import FernEngine
    eng = FernEngine("cuda:0") if family == "f32x3" else engine
    try:
        if family in ("f32", "f32x3"):
            a, w, b, _, _ = gemm_refs.f32_case(m, n, k)
            if family == "f32x3":
                eng.set_precision("f32x3")
            run = lambda: eng.gemm(a, w, b, epilogue=0).cpu()  # noqa: E731
            key = f"f32 {m} {n} {k} 0 0 " if family == "f32" else f"f32x3 {m} {n} {k} 0 "
        elif family == "bf16":
            _, ab, wb, b, _, _ = gemm_refs.bf16_case(m, n, k, 0)
            ab, wb = ab.cuda(), wb.cuda()
            run = lambda: eng.gemm_bf16(ab, wb, b, epilogue=0, out_bf16=False).cpu()  # noqa: E731
            key = f"bf16 {m} {n} {k} 0 0 "
        elif family == "fp8":
            a8, sa, w8, sw, b, _, _, _ = gemm_refs.fp8_case(eng, m, n, k, 0)
            run = lambda: eng.gemm_fp8(a8, sa, w8, sw, b, epilogue=0, out_bf16=False).cpu()  # noqa: E731
            key = f"fp8 {m} {n} {k} 0 2 "
        else:
            a8, sa, w8, sw, b, _, _, _ = gemm_refs.mx8_case(eng, m, n, k, 0)
            run = lambda: eng.gemm_mx8(a8, sa, w8, sw, b, epilogue=0, out_bf16=False).cpu()  # noqa: E731
            key = f"mx8 {m} {n} {k} 0 4 "
        eng.tuner_force_config(family, 8 if family == "f32" else 0)
        try:
            forced = run()
        finally:
            eng.tuner_force_config(family, -1)
        before = eng.tuner_export().splitlines()
        assert not [ln for ln in before if ln.startswith(key)], "a forced call stored a choice"
        first = run()
        after = eng.tuner_export().splitlines()
        new = [ln for ln in after if ln not in before]
        assert len(new) == 1 and new[0].startswith(key), new
        assert len(after) == len(before) + 1
        eng.tuner_import(new[0] + "\n")
        assert eng.tuner_export().splitlines() == after, "the exported line was not accepted back as it is"
        assert torch.equal(first.view(torch.int32), forced.view(torch.int32))
        again = run()
        assert eng.tuner_export().splitlines() == after
        assert torch.equal(again.view(torch.int32), forced.view(torch.int32))
    finally:
        if eng is not engine:
            eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(64, 128, 64), (197, 384, 96), (1000, 520, 256), (4096, 768, 768)])
@pytest.mark.parametrize("epi", [0, 1, 2, 3])
@pytest.mark.parametrize("out_bf16", [False, True])
def test_gemm_bf16(engine, m, n, k, epi, out_bf16):
    """bf16-operand GEMM against fp64 math on the SAME rounded operands: only the fp32 accumulation order differs."""
    if epi == 3 and out_bf16:
        pytest.skip("the residual epilogue keeps the fp32 residual stream")
    a, ab, wb, b, r, base = gemm_refs.bf16_case(m, n, k, epi)
    ref = gemm_refs.epi_ref(base, epi, r)
    got = engine.gemm_bf16(ab.cuda(), wb.cuda(), b, residual=r if epi == 3 else None, epilogue=epi, out_bf16=out_bf16)
    # the engine's own fp32 -> bf16 conversion is RNE, i.e. torch's
    assert torch.equal(engine.to_bf16(a).cpu().view(torch.int16), ab.view(torch.int16))
    gemm_refs.check_bf16_family(got, ref, out_bf16)


@pytest.mark.gpu
@pytest.mark.parametrize("b,heads,hd,sq,sk,causal", [
    (3, 12, 64, 197, 197, False), (2, 8, 64, 77, 77, True), (2, 4, 32, 50, 50, False), (1, 2, 80, 91, 91, False),
    (2, 3, 64, 13, 13, False), (1, 2, 96, 33, 33, True), (2, 2, 64, 224, 224, False), (1, 1, 8, 5, 5, False)])
def test_attention_bf16(engine, b, heads, hd, sq, sk, causal):
    """bf16 operand attention against fp64 softmax attention on the SAME bf16-rounded q, k, v."""
    g = torch.Generator().manual_seed(b * 100 + heads * 10 + hd + sq)
    w = heads * hd
    q, k, v = (torch.randn(b, s, w, generator=g).bfloat16() for s in (sq, sk, sk))
    got = engine.attention_bf16(q.cuda(), k.cuda(), v.cuda(), heads, causal=causal)
    assert got.dtype == torch.bfloat16
    qd, kd, vd = (t.double().view(b, -1, heads, hd).transpose(1, 2) for t in (q, k, v))
    att = qd @ kd.transpose(-1, -2) * hd ** -0.5
    if causal:
        att = att + torch.full((sq, sk), float("-inf"), dtype=torch.float64).triu(1)
    ref = (torch.softmax(att, dim=-1) @ vd).transpose(1, 2).reshape(b, sq, w)
    # error budget: weights rounded to bf16 (2^-9 relative each, averaged over the keys) + one bf16 rounding of the output
    err = (got.float().cpu().double() - ref).abs().max().item()
    assert err < 2 ** -7 * max(1.0, ref.abs().max().item()), err


def _q8_ref(x):
    """torch statement of the product's per-row e4m3fn quantiser (same operation order: scale = max * (1/448), q = x * (1/scale))."""
    am = x.abs().amax(dim=-1, keepdim=True)
    sc = torch.where(am > 0, am * torch.tensor(1.0 / 448.0, dtype=torch.float32), torch.ones_like(am))
    return (x * (1.0 / sc)).to(torch.float8_e4m3fn), sc.squeeze(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,d,bf16", [(5, 64, False), (197, 768, True), (64, 3072, True), (33, 4096, False), (1000, 512, True)])
def test_quantize_rows_fp8_is_bit_exact(engine, rows, d, bf16):
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g) * torch.logspace(-3, 3, rows).unsqueeze(1)     # rows of very different magnitude
    x[rows // 2] = 0                                                                     # an all-zero row keeps scale 1
    if bf16:
        x = x.bfloat16()
    y, sc = engine.quantize_rows_fp8(x.cuda())
    q_ref, sc_ref = _q8_ref(x.float())
    assert torch.equal(sc.cpu(), sc_ref)
    assert torch.equal(y.cpu(), q_ref.view(torch.uint8))          # same e4m3fn bytes as torch's round-to-nearest-even cast
    assert sc[rows // 2].item() == 1.0 and int(y[rows // 2].max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(64, 128, 64), (197, 384, 192), (1000, 520, 256), (4096, 768, 768)])
@pytest.mark.parametrize("epi,out_bf16", [(0, False), (0, True), (1, True), (3, False)])
def test_gemm_fp8(engine, m, n, k, epi, out_bf16):
    """fp8-operand GEMM against fp64 math on the SAME quantised operands and scales."""
    a8, sa, w8, sw, b, r, base, g = gemm_refs.fp8_case(engine, m, n, k, epi)
    ref = gemm_refs.epi_ref(base, epi, r)
    got = engine.gemm_fp8(a8, sa, w8, sw, b, residual=r if epi == 3 else None, epilogue=epi, out_bf16=out_bf16)
    gemm_refs.check_fp8_family(got, ref, out_bf16)      # (the fp8 MFMA is exact on integer data: checked below)
    if epi == 0 and not out_bf16:
        ai = torch.randint(-4, 5, (m, k), generator=g).float()
        wi = torch.randint(-4, 5, (n, k), generator=g).float()
        ones_m, ones_n = torch.ones(m, device="cuda"), torch.ones(n, device="cuda")
        gi = engine.gemm_fp8(ai.to(torch.float8_e4m3fn).view(torch.uint8).cuda(), ones_m, wi.to(torch.float8_e4m3fn).view(torch.uint8).cuda(),
                             ones_n, None)
        assert torch.equal(gi.cpu(), ai @ wi.T)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(64, 128, 128), (197, 384, 256), (1000, 512, 640), (4097, 3072, 768)])
@pytest.mark.parametrize("epi", [0, 1])
def test_gemm_mx8_quantising_epilogue_is_the_quantiser_applied_to_the_fp32_output(engine, m, n, k, epi):
    """fern_gemm_mx8_quant == fern_quantize_mx8(fern_gemm_mx8(... fp32 output)), bytes and scales, bit for bit."""
    g = torch.Generator().manual_seed(m + n + k + epi)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) * k ** -0.5
    b = torch.randn(n, generator=g)
    a8, sa = engine.quantize_mx8(a)
    w8, sw = engine.quantize_mx8(w)
    q_ref, s_ref = engine.quantize_mx8(engine.gemm_mx8(a8, sa, w8, sw, b, epilogue=epi))
    q, sc = engine.gemm_mx8_quant(a8, sa, w8, sw, b, epilogue=epi)
    assert torch.equal(sc, s_ref)
    assert torch.equal(q, q_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,d,bf16", [(5, 128, False), (197, 768, True), (64, 3072, True), (33, 4096, False), (1000, 512, True)])
def test_quantize_mx8_is_bit_exact(engine, rows, d, bf16):
    """Block-scaled quantiser: scale bytes, e4m3fn bytes and the scale layout against the oracle's restatement."""
    from oracle.clip import mx8_quantize, mx8_dequantize
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g) * torch.logspace(-3, 3, rows).unsqueeze(1)
    x[:, 32:64] *= 50.0                                   # an outlier block: its neighbours keep their own scales
    x[rows // 2, :32] = 0                                  # an all-zero block
    x[0, 64] = 448.0; x[0, 65:96] = 0                      # maximum exactly 448 * 2^0: scale byte 127, element byte 0x7E
    x[1, 64] = 480.0; x[1, 65:96] = 0                      # above (and a bf16 value): the next power of two
    if bf16:
        x = x.bfloat16()
    y, sc = engine.quantize_mx8(x.cuda())
    q_ref, e_ref = mx8_quantize(x.float())
    assert torch.equal(_mx_scales_by_block(sc.cpu()), e_ref)
    assert torch.equal(y.cpu(), q_ref.view(torch.uint8))
    e = _mx_scales_by_block(sc.cpu())
    assert e[rows // 2, 0] == 1 and int(y[rows // 2, :32].max()) == 0
    assert e[0, 2] == 127 and y[0, 64] == 0x7E and e[1, 2] == 128
    # no element is clipped: dequantised values stay within half an e4m3 step (2^-4 relative) of the input, block maximum included
    dq = mx8_dequantize(q_ref, e_ref)
    blk = x.float().reshape(rows, d // 32, 32)
    assert ((dq.reshape(rows, d // 32, 32) - blk).abs() <= blk.abs().amax(-1, keepdim=True) * 2.0 ** -4).all()


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(64, 128, 128), (197, 384, 256), (1000, 520, 640), (4096, 768, 768), (333, 2304, 768)])
@pytest.mark.parametrize("epi,out_bf16", [(0, False), (0, True), (1, True), (3, False), (3, True)])
def test_gemm_mx8(engine, m, n, k, epi, out_bf16):
    """Block-scaled fp8 GEMM (v_mfma_scale_f32_32x32x64_f8f6f4) against fp64 math on the SAME quantised operands and scales."""
    from oracle.clip import mx8_dequantize
    a8, sa, w8, sw, b, r, base, g = gemm_refs.mx8_case(engine, m, n, k, epi)
    ref = gemm_refs.epi_ref(base, epi, r)
    if epi == 3 and out_bf16:
        # the bf16 residual-stream form (FERN_PREC_MX8's token stream): bf16 residual in, C = bf16(acc + bias + residual) -- ONE rounding
        rb = r.bfloat16()
        ref = gemm_refs.epi_ref(base, 3, rb)
        got = engine.gemm_mx8(a8, sa, w8, sw, b, residual=rb, epilogue=3, out_bf16=True)
        f32 = engine.gemm_mx8(a8, sa, w8, sw, b, residual=rb.float(), epilogue=3, out_bf16=False)
        assert got.dtype == torch.bfloat16 and torch.equal(got.cpu(), f32.cpu().bfloat16())      # exactly the fp32 epilogue's value, rounded once
        assert torch.allclose(got.float().cpu().double(), ref, rtol=2 ** -7, atol=1e-3)
        inplace = rb.cuda().clone()                                                                 # R == C: the stream is updated in place
        from fashionern_aaai2024_amd import _lib
        from fashionern_aaai2024_amd.engine import _ptr, _stream
        bias_d = b.cuda()
        _lib.check(engine.lib.fern_gemm_mx8(engine._h, _ptr(a8), k, _ptr(sa), sa.shape[1], _ptr(w8), k, _ptr(sw), sw.shape[1], _ptr(bias_d),
                                            _ptr(inplace), _ptr(inplace), n, m, n, k, 3, 1, _stream()), "fern_gemm_mx8")
        assert torch.equal(inplace.cpu(), got.cpu())
        return
    got = engine.gemm_mx8(a8, sa, w8, sw, b, residual=r if epi == 3 else None, epilogue=epi, out_bf16=out_bf16)
    gemm_refs.check_fp8_family(got, ref, out_bf16)
    if epi == 0 and not out_bf16:
        # integer data, power-of-two block scales: every product and partial sum is exact in fp32
        ai = torch.randint(-4, 5, (m, k), generator=g).float()
        wi = torch.randint(-4, 5, (n, k), generator=g).float()
        ea = torch.randint(125, 130, (k // 128, m, 4), generator=g, dtype=torch.uint8)
        ew = torch.randint(125, 130, (k // 128, n, 4), generator=g, dtype=torch.uint8)
        gi = engine.gemm_mx8(ai.to(torch.float8_e4m3fn).view(torch.uint8).cuda(), ea.cuda(), wi.to(torch.float8_e4m3fn).view(torch.uint8).cuda(),
                             ew.cuda(), None)
        da = mx8_dequantize(ai, _mx_scales_by_block(ea))
        dw = mx8_dequantize(wi, _mx_scales_by_block(ew))
        assert torch.equal(gi.cpu(), da @ dw.T)


@pytest.mark.gpu
def test_tuner_concurrency_score_never_changes_a_result(engine):
    """fern_tuner_set_concurrency(3) makes the reduced-precision families score their tile trials for a 3-lane pipeline (other
    tiles may win); a row's bits must not depend on that choice, nor on the batch it travels in."""
    g = torch.Generator().manual_seed(7)
    k, n = 768, 768
    a = torch.randn(6400, k, generator=g)
    w = torch.randn(n, k, generator=g) * k ** -0.5
    b = torch.randn(n, generator=g)
    a8, sa = engine.quantize_mx8(a)
    w8, sw = engine.quantize_mx8(w)
    ab, wb = engine.to_bf16(a.cuda()), engine.to_bf16(w.cuda())
    try:
        engine.tuner_set_concurrency(1)
        ref_mx = engine.gemm_mx8(a8[:6272], sa[:, :6272].contiguous(), w8, sw, b, epilogue=0, out_bf16=True)
        ref_bf = engine.gemm_bf16(ab[:6272], wb, b, epilogue=0, out_bf16=True)
        engine.tuner_set_concurrency(3)
        got_mx = engine.gemm_mx8(a8, sa, w8, sw, b, epilogue=0, out_bf16=True)           # new shape key: tuned under the new score
        got_bf = engine.gemm_bf16(ab, wb, b, epilogue=0, out_bf16=True)
    finally:
        engine.tuner_set_concurrency(1)                                                   # process-wide setting
    assert torch.equal(got_mx[:6272].view(torch.int16), ref_mx.view(torch.int16))
    assert torch.equal(got_bf[:6272].view(torch.int16), ref_bf.view(torch.int16))
    with pytest.raises(RuntimeError):
        engine.tuner_set_concurrency(0)


@pytest.mark.gpu
@pytest.mark.slow
@pytest.mark.parametrize("family,n,key", [("bf16", 10, "test_gemm_bf16"), ("fp8", 6, "test_gemm_fp8"), ("mx8", 12, "test_gemm_mx8")])
def test_every_reduced_precision_gemm_tile_variant(family, n, key):
    """The bf16 / fp8 / block-scaled launchers pick (or tune) a tile per shape; each variant is also forced over its family's suite."""
    r = _forced_family_result(family, list(range(n)), key)
    assert r.returncode == 0


@pytest.mark.gpu
def test_reduced_precision_gemms_are_batch_invariant(engine):
    """Every tile shape of the bf16 / fp8 kernels sums the k groups in the same order: a row's bits do not depend on M."""
    g = torch.Generator().manual_seed(5)
    a = torch.randn(3000, 768, generator=g)
    w = torch.randn(768, 768, generator=g) * 768 ** -0.5
    b = torch.randn(768, generator=g)
    ab, wb = engine.to_bf16(a), engine.to_bf16(w)
    full = engine.gemm_bf16(ab, wb, b, epilogue=1, out_bf16=True).cpu()
    a8, sa = engine.quantize_rows_fp8(a)
    w8, sw = engine.quantize_rows_fp8(w)
    full8 = engine.gemm_fp8(a8, sa, w8, sw, b, epilogue=0).cpu()
    am, sam = engine.quantize_mx8(a)
    wq, swm = engine.quantize_mx8(w)
    fullm = engine.gemm_mx8(am, sam, wq, swm, b, epilogue=0).cpu()
    for lo, hi in ((0, 1), (0, 64), (100, 1124), (2990, 3000)):
        assert torch.equal(engine.gemm_mx8(am[lo:hi].contiguous(), sam[:, lo:hi].contiguous(), wq, swm, b, epilogue=0).cpu(), fullm[lo:hi])
        assert torch.equal(engine.gemm_bf16(ab[lo:hi].contiguous(), wb, b, epilogue=1, out_bf16=True).cpu(), full[lo:hi])
        assert torch.equal(engine.gemm_fp8(a8[lo:hi].contiguous(), sa[lo:hi].contiguous(), w8, sw, b, epilogue=0).cpu(), full8[lo:hi])


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(300, 320, 128), (1000, 260, 256), (257, 480, 384), (64, 512, 512), (2049, 1000, 1536), (12608, 768, 768)])
def test_ping_pong_tile_is_bit_identical_to_the_family(engine, m, n, k):
    """csrc/gemm_pp.h (round 6): the 256 x 256 ping-pong tile -- cfg 7 of the bf16 family, 11 of the block-scaled fp8 family -- against
    configuration 0 of its family, bit for bit: ragged M / N edges, K shorter than the 4-slot ring (1 .. 3 k tiles), every stored
    epilogue incl. the bf16 residual stream and the quantising epilogue."""
    g = torch.Generator().manual_seed(m + n + k)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) * k ** -0.5
    b = torch.randn(n, generator=g)
    r = torch.randn(m, n, generator=g)
    ab, wb, rb = engine.to_bf16(a), engine.to_bf16(w), engine.to_bf16(r)
    (a8, sa), (w8, sw) = engine.quantize_mx8(a), engine.quantize_mx8(w)

    def outputs(family, cfg):
        engine.tuner_force_config(family, cfg)
        try:
            outs = []
            if family == "bf16":
                for epi, res, ob in ((0, None, True), (1, None, True), (2, None, False), (3, r, False), (0, None, False)):
                    outs.append(engine.gemm_bf16(ab, wb, b, residual=res, epilogue=epi, out_bf16=ob))
            else:
                for epi, res, ob in ((0, None, True), (1, None, True), (3, r, False), (3, rb, True), (0, None, False)):
                    outs.append(engine.gemm_mx8(a8, sa, w8, sw, b, residual=res, epilogue=epi, out_bf16=ob))
                if n % 128 == 0:
                    for epi in (0, 1):
                        outs.extend(engine.gemm_mx8_quant(a8, sa, w8, sw, b, epilogue=epi))
            torch.cuda.synchronize()
            return [o.cpu().view(torch.uint8) if o.dtype != torch.float32 else o.cpu() for o in outs]
        finally:
            engine.tuner_force_config(family, -1)

    for family, new in (("bf16", 7), ("mx8", 11)):
        ref, got = outputs(family, 0), outputs(family, new)
        assert len(ref) == len(got) and len(ref) >= 5
        for i, (x, y) in enumerate(zip(ref, got)):
            assert torch.equal(x, y), (family, i)
        assert all(torch.isfinite(x.float()).all() for x in ref if x.dtype == torch.float32)


@pytest.mark.gpu
def test_resnet_tower_is_bit_identical_on_every_lds_dma_tile(tmp_path):
    """The ModifiedResNet's convolutions (3x3-window loader and 1x1, 80 / 160 / 320 / ... output channels) through the 128x128 tile
    and through the odd-width tiles built for those channel counts (configs 14: 128x96, 15: 128x160): identical features."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for cfg in ("8", "14", "15"):
        path = str(tmp_path / f"rn_{cfg}.npy")
        env = dict(os.environ, FERN_GEMM_CFG=cfg)
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "_resnet_dump.py"), path], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(path))
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    for other in outs[1:]:
        assert np.array_equal(outs[0].view(np.uint32), other.view(np.uint32))


@pytest.mark.gpu
def test_small_m_16x16_kernel_is_bit_identical_to_the_32x32_kernels(tmp_path):
    """The small-M kernel (v_mfma_f32_16x16x4_f32, config 6) adds every output's products in the same order as the 32x32
    kernels: plain GEMMs of every epilogue kind and the fused combiner (reduce epilogue) must match BIT FOR BIT, whichever
    kernel the launcher is forced to (FERN_GEMM_CFG is read once per process, hence the two subprocesses)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for cfg in ("6", "3", "11"):
        path = str(tmp_path / f"dump_{cfg}.npz")
        env = dict(os.environ, FERN_GEMM_CFG=cfg)
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "_gemm_dump.py"), path], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(path))
    for other in outs[1:]:
        assert sorted(outs[0].files) == sorted(other.files)
        for k in outs[0].files:
            assert np.array_equal(outs[0][k].view(np.uint32), other[k].view(np.uint32)), k

"""Model-level parity through the C ABI: fusion (ERN mode="test"/"index", CombinerSimple, VisualSR) and the
CLIP towers against the CPU oracle on the same seeded weights and inputs.  Tolerances are absolute on
unit-norm (fusion) or O(1) (CLIP) features; north_star asks for cosine scores within 1e-3."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fashionern_aaai2024_amd import synth
from fashionern_aaai2024_amd._lib import FernError
from fashionern_aaai2024_amd.engine import (COMBINER_DVR_FINAL, COMBINER_DVR_GLOBAL, COMBINER_DVR_LOCAL, COMBINER_TARGET,
                                             SR_DVR, SR_TARGET, FernEngine)
from oracle import clip as oclip
from oracle import fusion as ofusion

import support
from support import maxerr, tower_engine, t as _t      # `t` is a parameter of the dvr_fuse cases

pytestmark = pytest.mark.gpu

FUSION_TOL = 2e-5


def fusion_engine(d):
    return support.fusion_engine(d, seed=11)


@pytest.mark.parametrize("d", [128, 512, 640])
def test_combiner_and_sr(d):
    eng, sd = fusion_engine(d)
    n = 70
    img, txt = _t(synth.global_feats(n, d, tag="ci")), _t(synth.global_feats(n, d, tag="ct"))
    for which, prefix in ((COMBINER_TARGET, "Combiner_module"), (COMBINER_DVR_GLOBAL, "DVR.combiner_global"),
                          (COMBINER_DVR_LOCAL, "DVR.combiner_local"), (COMBINER_DVR_FINAL, "DVR.combiner")):
        ref = ofusion.combiner_simple(sd, prefix, img, txt)
        assert maxerr(eng.combiner(which, img, txt), ref) < FUSION_TOL
    loc = _t(synth.local_feats(n, d, tag="sl"))
    for which, prefix in ((SR_TARGET, "SR_module"), (SR_DVR, "DVR.SR_module")):
        assert maxerr(eng.visual_sr(which, loc), ofusion.visual_sr(sd, prefix, loc)) < FUSION_TOL


@pytest.mark.parametrize("d,n", [(128, 1), (128, 300), (512, 129), (640, 65)])
def test_index_fuse(d, n):
    eng, sd = fusion_engine(d)
    raw, loc = _t(synth.global_feats(n, d, tag="ir")), _t(synth.local_feats(n, d, tag="il"))
    ref = ofusion.index_fuse(sd, F.normalize(raw, dim=-1), loc)
    assert maxerr(eng.index_fuse(raw, loc, normalize_input=True), ref) < FUSION_TOL
    assert maxerr(eng.index_fuse(F.normalize(raw, dim=-1), loc), ref) < FUSION_TOL


def test_index_fuse_tiles_large_gallery():
    """More rows than one internal tile (8192): results must not depend on the tiling."""
    d, n = 128, 8192 + 777
    eng, sd = fusion_engine(d)
    raw, loc = _t(synth.global_feats(n, d, tag="big")), _t(synth.local_feats(n, d, tag="bigl"))
    got = eng.index_fuse(raw, loc, normalize_input=True).cpu()
    sel = torch.cat((torch.arange(0, 64), torch.arange(8160, 8260), torch.arange(n - 50, n)))
    ref = ofusion.index_fuse(sd, F.normalize(raw[sel], dim=-1), loc[sel])
    assert maxerr(got[sel], ref) < FUSION_TOL
    small = eng.index_fuse(raw[8192:], loc[8192:], normalize_input=True).cpu()
    assert torch.equal(small, got[8192:])


@pytest.mark.parametrize("d,b,t", [(128, 5, 77), (128, 1, 77), (512, 9, 77), (640, 6, 77), (128, 3, 40)])
def test_dvr_fuse(d, b, t):
    eng, sd = fusion_engine(d)
    rg, rl = _t(synth.global_feats(b, d, tag="rg")), _t(synth.local_feats(b, d, tag="rl"))
    tg = _t(synth.global_feats(b, d, tag="tg"))
    ts = _t(synth._normal(42, f"tseq/{d}", (b, t, d)))
    ref = ofusion.dvr_fuse(sd, rl, ts, rg, tg)
    got = eng.dvr_fuse(rg, rl, tg, ts)
    assert maxerr(got, ref) < 5e-5
    assert abs(got.norm(dim=1).cpu() - 1).max().item() < 1e-5


def test_dvr_fuse_without_cls_token():
    """GPU-trained checkpoints lack DVR.transformer_layer.cls_token (fusion_model.py:185): it defaults to zeros."""
    d = 128
    sd_np = synth.fusion_state_dict(d, seed=12, with_cls_token=False)
    eng = FernEngine("cuda:0")
    eng.load_tensors(sd_np)
    eng.finalize_fusion(d)
    sd = ofusion.as_torch(sd_np)
    b = 4
    rg, rl = _t(synth.global_feats(b, d, tag="rg")), _t(synth.local_feats(b, d, tag="rl"))
    tg, ts = _t(synth.global_feats(b, d, tag="tg")), _t(synth._normal(42, "tseq", (b, 77, d)))
    assert maxerr(eng.dvr_fuse(rg, rl, tg, ts), ofusion.dvr_fuse(sd, rl, ts, rg, tg)) < 5e-5
    eng.close()


def test_missing_weight_fails_loudly():
    from fashionern_aaai2024_amd._lib import FernError
    eng = FernEngine("cuda:0")
    sd = synth.fusion_state_dict(128, seed=1)
    del sd["SR_module.embedding_common.weight"]
    eng.load_tensors(sd)
    with pytest.raises(FernError, match="missing weight"):
        eng.finalize_fusion(128)
    with pytest.raises(FernError, match="not finalised"):
        eng.lib  # noqa
        eng.feature_dim = 128
        eng.index_fuse(torch.zeros(2, 128), torch.zeros(2, 13, 128))
    eng.close()


@pytest.mark.parametrize("name", ["tiny", "tiny-hd64"])
def test_clip_towers_tiny(name):
    cfg, sd_np, eng = tower_engine(name, seed=5)
    sd = ofusion.as_torch(sd_np)
    imgs = _t(synth.images(5, cfg))
    ref = oclip.encode_image(sd, cfg, imgs)
    got = eng.encode_image(imgs)
    assert maxerr(got, ref) < 2e-4 * max(1.0, ref.abs().max().item())
    for full in (True, False):
        toks = _t(synth.captions(6, cfg, full_length=full))
        rg, rs = oclip.encode_text(sd, cfg, toks)
        g, s = eng.encode_text(toks)
        scale = max(1.0, rs.abs().max().item())
        assert maxerr(s, rs) < 2e-4 * scale and maxerr(g, rg) < 2e-4 * scale
        g2, _ = eng.encode_text(toks, want_seq=False)
        assert maxerr(g2, rg) < 2e-4 * scale
    eng.close()


def test_clip_vit_b16_full_size():
    """The real ViT-B/16 shape (197 tokens, 12 x 64 heads, 12 layers) on 3 images / captions."""
    cfg, sd_np, eng = tower_engine("ViT-B-16", seed=6)
    sd = ofusion.as_torch(sd_np)
    imgs = _t(synth.images(3, cfg))
    ref = oclip.encode_image(sd, cfg, imgs)
    got = eng.encode_image(imgs)
    cos = F.cosine_similarity(got.cpu(), ref, dim=-1)
    assert maxerr(got, ref) < 1e-3 * max(1.0, ref.abs().max().item()) and (1 - cos).abs().max().item() < 1e-5
    toks = _t(synth.captions(3, cfg))
    rg, rs = oclip.encode_text(sd, cfg, toks)
    g, s = eng.encode_text(toks)
    assert maxerr(s, rs) < 1e-3 * max(1.0, rs.abs().max().item())
    assert (1 - F.cosine_similarity(g.cpu(), rg, dim=-1)).abs().max().item() < 1e-5
    eng.close()


def test_zero_rows_fusion():
    eng, sd = fusion_engine(128)
    assert eng.index_fuse(torch.zeros(0, 128), torch.zeros(0, 13, 128)).shape == (0, 128)
    assert eng.dvr_fuse(torch.zeros(0, 128), torch.zeros(0, 13, 128), torch.zeros(0, 128), torch.zeros(0, 77, 128)).shape == (0, 128)
    with pytest.raises(ValueError):
        eng.index_fuse(torch.zeros(3, 128), torch.zeros(3, 12, 128))          # VisualSR needs exactly 13 patches


def test_batch_invariance_of_fusion_rows():
    """Every GEMM tile shape accumulates over k in the same order, so a row's result does not depend on the batch it
    travels in (what makes sharded gallery builds bit-identical to unsharded ones)."""
    d = 128
    eng, sd = fusion_engine(d)
    raw, loc = _t(synth.global_feats(2000, d, tag="bi")), _t(synth.local_feats(2000, d, tag="bil"))
    full = eng.index_fuse(raw, loc, normalize_input=True).cpu()
    for a, b in ((0, 1), (5, 70), (100, 1124), (1990, 2000)):
        assert torch.equal(eng.index_fuse(raw[a:b], loc[a:b], normalize_input=True).cpu(), full[a:b])


def test_modified_resnet_tower_tiny_and_rn50x4():
    """open_clip ModifiedResNet image tower (RN50x4 for BASELINE configs C1/C3): NHWC GEMM convolutions with the 3x3-window
    LDS-DMA loader, folded BatchNorm, fused ReLU / residual epilogues, attention pool -- against the CPU oracle."""
    for name, n, tol in (("tiny-resnet", 5, 2e-4), ("RN50x4", 2, 1e-3)):
        cfg, sd_np, eng = tower_engine(name, seed=8)
        sd = ofusion.as_torch(sd_np)
        imgs = _t(synth.images(n, cfg))
        ref = oclip.encode_image(sd, cfg, imgs)
        got = eng.encode_image(imgs)
        scale = max(1.0, ref.abs().max().item())
        assert maxerr(got, ref) < tol * scale, (name, maxerr(got, ref), scale)
        assert (1 - F.cosine_similarity(got.cpu(), ref, dim=-1)).abs().max().item() < 1e-5
        # batch invariance: one image alone gives the same row
        assert torch.equal(eng.encode_image(imgs[1:2]), got[1:2])
        toks = _t(synth.captions(3, cfg))
        rg, rs = oclip.encode_text(sd, cfg, toks)
        g, s = eng.encode_text(toks)
        assert maxerr(s, rs) < 1e-3 * max(1.0, rs.abs().max().item())
        eng.close()


@pytest.mark.parametrize("name,n", [("tiny", 5), ("tiny-hd64", 4), ("ViT-B-16", 3)])
def test_clip_towers_bf16_precision(name, n):
    """Perf mode (fern_set_precision(BF16)): bf16 operands on the token-level block GEMMs, fp32 accumulation.

    Checked two ways: (1) against the oracle evaluated with the SAME rounding points (only fp32 summation order and
    the occasional operand that lands on the other side of a bf16 rounding boundary differ); (2) against the fp32
    oracle, to state what the mode costs in accuracy (bf16 has 8 mantissa bits: ~4e-3 relative per operand)."""
    cfg, sd_np, eng = tower_engine(name, seed=11)
    sd = ofusion.as_torch(sd_np)
    imgs = _t(synth.images(n, cfg))
    toks = _t(synth.captions(n, cfg))
    fp32_img = eng.encode_image(imgs)
    eng.set_precision("bf16")
    assert eng.precision == "bf16"
    got = eng.encode_image(imgs)
    g, s = eng.encode_text(toks)
    # batch invariance survives the mode: a row does not depend on its batch
    assert torch.equal(eng.encode_image(imgs[1:2]), got[1:2])
    child = eng.fork()
    assert child.precision == "bf16" and torch.equal(child.encode_image(imgs), got)
    child.close()
    eng.set_precision("fp32")
    assert torch.equal(eng.encode_image(imgs), fp32_img)          # switching back restores the parity path bit for bit

    ref_b = oclip.encode_image(sd, cfg, imgs, precision="bf16")
    ref_f = oclip.encode_image(sd, cfg, imgs)
    rg_b, rs_b = oclip.encode_text(sd, cfg, toks, precision="bf16")
    rg_f, rs_f = oclip.encode_text(sd, cfg, toks)

    def cos_err(a, b):
        return (1 - F.cosine_similarity(a.cpu().double().flatten(-1 if a.dim() == 2 else 1), b.double().flatten(-1 if b.dim() == 2 else 1), dim=-1)).abs().max().item()

    # (1) same rounding points: tight
    assert cos_err(got, ref_b) < 2e-5 and cos_err(g, rg_b) < 2e-5
    assert maxerr(got, ref_b) < 5e-3 * max(1.0, ref_b.abs().max().item())
    assert maxerr(s, rs_b) < 5e-3 * max(1.0, rs_b.abs().max().item())
    # (2) cost of the mode against the fp32 statement: features stay within 1e-3 in cosine
    assert cos_err(got, ref_f) < 1e-3 and cos_err(g, rg_f) < 1e-3
    assert cos_err(got, ref_f) > 0 and not torch.equal(got, fp32_img)   # the mode really is a different precision
    eng.close()


@pytest.mark.parametrize("name,n", [("tiny-hd64", 4), ("ViT-B-16", 3)])
def test_clip_towers_fp8_precision(name, n):
    """BASELINE config 5's "fp8 MFMA encoder path" (fern_set_precision(FP8)): e4m3fn operands with per-token / per-channel
    scales on the token-level block GEMMs.  The kernels themselves are pinned in test_gpu_kernels.py (bit-exact quantiser,
    GEMM against exact arithmetic on the same bytes).  End to end: (1) vs the oracle restating the same quantisation points
    -- tiny arithmetic differences move values across e4m3 rounding boundaries (3 mantissa bits: one flipped element is a
    6 % change of it) and the flips compound over 11 layers, so the agreement is loose (measured 1.4e-4 ... 1.3e-3 in
    cosine) but the product must sit closer to its restatement than to fp32; (2) vs the fp32 oracle: the cost of the mode,
    reported not hidden -- cosine error of the features 1.3e-3 ... 4.2e-3 (bf16 mode: 1e-5)."""
    cfg, sd_np, eng = tower_engine(name, seed=11)
    sd = ofusion.as_torch(sd_np)
    imgs = _t(synth.images(n, cfg))
    toks = _t(synth.captions(n, cfg))
    fp32_img = eng.encode_image(imgs)
    eng.set_precision("fp8")
    assert eng.precision == "fp8"
    got = eng.encode_image(imgs)
    g, s = eng.encode_text(toks)
    assert torch.equal(eng.encode_image(imgs[1:2]), got[1:2])          # per-token scales: still batch-invariant
    eng.set_precision("fp32")
    assert torch.equal(eng.encode_image(imgs), fp32_img)

    ref_q = oclip.encode_image(sd, cfg, imgs, precision="fp8")
    ref_f = oclip.encode_image(sd, cfg, imgs)
    rg_q, _ = oclip.encode_text(sd, cfg, toks, precision="fp8")
    rg_f, _ = oclip.encode_text(sd, cfg, toks)

    def cos_err(a, b):
        return (1 - F.cosine_similarity(a.cpu().double(), b.double(), dim=-1)).abs().max().item()

    assert cos_err(got, ref_q) < 2e-3 and cos_err(g, rg_q) < 2e-3      # same quantisation points
    assert cos_err(got, ref_q) < cos_err(got, ref_f) and cos_err(g, rg_q) < cos_err(g, rg_f)
    assert cos_err(got, ref_f) < 1e-2 and cos_err(g, rg_f) < 1e-2      # the price of fp8, well above bf16's 1e-5
    assert cos_err(got, ref_f) > 1e-5
    eng.close()


@pytest.mark.parametrize("name,n", [("tiny-w256", 4), ("tiny-hd48", 4), ("ViT-B-16", 3)])
def test_clip_towers_mx8_precision(name, n):
    """BASELINE config 5 on the block-scaled MFMA (fern_set_precision(MX8)): e4m3fn operands with one E8M0 scale per 32-element
    block.  Kernels pinned in test_gpu_kernels.py (bit-exact quantiser, GEMM against exact arithmetic on the same bytes and
    scales).  End to end: (1) against the oracle restating the same quantisation points (e4m3 rounding flips compound over the
    layers, as in the per-row fp8 mode, so the agreement is loose but closer than to fp32); (2) against the fp32 oracle, the cost of
    the mode; (3) batch invariance and a clean return to fp32."""
    cfg, sd_np, eng = tower_engine(name, seed=11)
    sd = ofusion.as_torch(sd_np)
    imgs = _t(synth.images(n, cfg))
    toks = _t(synth.captions(n, cfg))
    fp32_img = eng.encode_image(imgs)
    eng.set_precision("mx8")
    assert eng.precision == "mx8"
    got = eng.encode_image(imgs)
    g, s = eng.encode_text(toks)
    assert torch.equal(eng.encode_image(imgs[1:2]), got[1:2])          # block scales are per token: still batch-invariant
    assert torch.equal(eng.encode_text(toks[2:3])[0], g[2:3])
    eng.set_precision("fp8")
    got8 = eng.encode_image(imgs)
    eng.set_precision("fp32")
    assert torch.equal(eng.encode_image(imgs), fp32_img)

    ref_q = oclip.encode_image(sd, cfg, imgs, precision="mx8")
    ref_f = oclip.encode_image(sd, cfg, imgs)
    rg_q, _ = oclip.encode_text(sd, cfg, toks, precision="mx8")
    rg_f, _ = oclip.encode_text(sd, cfg, toks)

    def cos_err(a, b):
        return (1 - F.cosine_similarity(a.cpu().double(), b.double(), dim=-1)).abs().max().item()

    print(f"mx8 {name}: vs restatement {cos_err(got, ref_q):.2e} / {cos_err(g, rg_q):.2e}, vs fp32 {cos_err(got, ref_f):.2e} / {cos_err(g, rg_f):.2e}, "
          f"per-row fp8 vs fp32 {cos_err(got8, ref_f):.2e}")
    assert cos_err(got, ref_q) < 2e-3 and cos_err(g, rg_q) < 2e-3      # same quantisation points
    assert cos_err(got, ref_q) < cos_err(got, ref_f) and cos_err(g, rg_q) < cos_err(g, rg_f)
    assert cos_err(got, ref_f) < 1e-2 and cos_err(g, rg_f) < 1e-2
    assert cos_err(got, ref_f) > 1e-5
    eng.close()


# Cosine-error bounds of the mixed modes against their own restatement.  Measured on an MI355X (tiny-w256 / tiny-hd48 / ViT-B-16):
# mx8img 2.7e-4 / 4.7e-7 / 8.1e-4, mx8mlp 7.7e-5 / 4.7e-7 / 4.0e-4 -- e4m3 rounding flips compounding over the layers, as in the
# mx8 and fp8 modes.  The bounds keep a margin of about 2.5x over the largest value.
MIXED_BOUNDS = {"mx8img": 2e-3, "mx8mlp": 1e-3}


@pytest.mark.parametrize("name,n", [("tiny-w256", 4), ("tiny-hd48", 4), ("ViT-B-16", 3)])
def test_clip_towers_mx8img_and_mx8mlp_precision(name, n):
    """The mixed modes (FERN_PREC_MX8_MLP; FERN_PREC_MX8_IMG, the c5 default) against oracle.clip's restatement of their own rounding
    points (_block_mixed: MX MLP half -- and for mx8img the MX attention half when head_dim % 32 == 0; tiny-hd48's head_dim 48 takes
    the bf16 attention half -- over the fp32 stream, the bf16 text tower).  (1) close to the restatement, closer than to fp32 and to
    the bf16 restatement; (2) the text features are the bf16 mode's; (3) batch invariance and a clean return to fp32."""
    cfg, sd_np, eng = tower_engine(name, seed=11)
    sd = ofusion.as_torch(sd_np)
    imgs = _t(synth.images(n, cfg))
    toks = _t(synth.captions(n, cfg))
    fp32_img = eng.encode_image(imgs)
    got, txt = {}, {}
    for mode in ("mx8img", "mx8mlp"):
        eng.set_precision(mode)
        assert eng.precision == mode
        got[mode] = eng.encode_image(imgs)
        txt[mode] = eng.encode_text(toks)
        assert torch.equal(eng.encode_image(imgs[1:2]), got[mode][1:2])      # block scales are per token: batch-invariant
        assert torch.equal(eng.encode_text(toks[2:3])[0], txt[mode][0][2:3])
    eng.set_precision("fp32")
    assert torch.equal(eng.encode_image(imgs), fp32_img)
    eng.close()

    ref = {m: oclip.encode_image(sd, cfg, imgs, precision=m) for m in ("mx8img", "mx8mlp", "bf16", "fp32")}
    rg_b, rs_b = oclip.encode_text(sd, cfg, toks, precision="bf16")

    def cos_err(a, b):
        return (1 - F.cosine_similarity(a.cpu().double().flatten(-1 if a.dim() == 2 else 1), b.double().flatten(-1 if b.dim() == 2 else 1), dim=-1)).abs().max().item()

    for mode, other in (("mx8img", "mx8mlp"), ("mx8mlp", "mx8img")):
        g, s = txt[mode]
        e_own, e_other = cos_err(got[mode], ref[mode]), cos_err(got[mode], ref[other])
        e_f, e_b = cos_err(got[mode], ref["fp32"]), cos_err(got[mode], ref["bf16"])
        print(f"{mode} {name}: vs own restatement {e_own:.2e}, vs {other} {e_other:.2e}, vs bf16 {e_b:.2e}, vs fp32 {e_f:.2e}; "
              f"text vs bf16 {cos_err(g, rg_b):.2e} / {cos_err(s, rs_b):.2e}")
        assert e_own < MIXED_BOUNDS[mode]
        assert e_own < e_f and e_own < e_b
        # e_other is reported, not asserted: on tiny-hd48 (head_dim 48) the two modes are the same computation, so there is no
        # separation to require; on the other towers it measured 2.4x - 16x
        # the text tower is the bf16 block: the bf16 test's bounds
        assert cos_err(g, rg_b) < 2e-5 and cos_err(s, rs_b) < 2e-5
        assert maxerr(s, rs_b) < 5e-3 * max(1.0, rs_b.abs().max().item())
    assert not torch.equal(got["mx8img"], fp32_img) and not torch.equal(got["mx8mlp"], fp32_img)


def test_mx8_precision_needs_widths_that_are_multiples_of_128():
    cfg, _, eng = tower_engine("tiny-hd64", seed=1)                              # ViT width 192
    with pytest.raises(FernError, match="multiples of 128"):
        eng.set_precision("mx8")
    assert eng.precision == "fp32"
    eng.close()


def test_fp8_precision_needs_widths_that_are_multiples_of_64():
    cfg, _, eng = tower_engine("tiny", seed=1)
    if cfg.v_width % 64 or cfg.t_width % 64 or cfg.v_mlp % 64 or cfg.t_mlp % 64:
        with pytest.raises(FernError, match="multiples of 64"):
            eng.set_precision("fp8")
    eng.close()


@pytest.mark.parametrize("d,b,t", [(128, 5, 77), (512, 9, 77), (640, 6, 77), (128, 3, 40)])
def test_dvr_fuse_reduced_precision(d, b, t):
    """In the reduced-precision modes (bf16 and fp8 alike) the two fusion BERT blocks run with bf16 operands / fp32
    accumulation and bf16 attention; cross attention, VisualSR and the combiners stay fp32.  (1) against the oracle's
    restatement of the same rounding points; (2) against the fp32 statement, to state what the mode costs."""
    eng, sd = fusion_engine(d)
    rg, rl = _t(synth.global_feats(b, d, tag="rg")), _t(synth.local_feats(b, d, tag="rl"))
    tg = _t(synth.global_feats(b, d, tag="tg"))
    ts = _t(synth._normal(42, f"tseq/{d}", (b, t, d)))
    fp32 = eng.dvr_fuse(rg, rl, tg, ts)
    ref_b = ofusion.dvr_fuse(sd, rl, ts, rg, tg, precision="bf16")
    ref_f = ofusion.dvr_fuse(sd, rl, ts, rg, tg)
    try:
        for prec in ("bf16", "fp8", "mx8"):
            eng.set_precision(prec)
            got = eng.dvr_fuse(rg, rl, tg, ts)
            assert torch.equal(eng.dvr_fuse(rg[1:2], rl[1:2], tg[1:2], ts[1:2]), got[1:2])      # batch-invariant
            assert maxerr(got, ref_b) < 5e-4                                                    # unit-norm features
            assert maxerr(got, ref_f) < 1e-2 and not torch.equal(got, fp32)
            assert abs(got.norm(dim=1).cpu() - 1).max().item() < 1e-5
    finally:
        eng.set_precision("fp32")
    assert torch.equal(eng.dvr_fuse(rg, rl, tg, ts), fp32)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp8", "mx8"])
def test_encoders_chunk_large_batches_without_changing_rows(precision):
    """Batches larger than the internal chunk (64 images, 256 captions, 256 fusion rows) are processed in pieces: every row
    must equal the row computed alone, in every precision mode (workspace reuse across chunks, scale buffers, bf16 copies)."""
    cfg = synth.CLIP_CONFIGS["tiny-w256" if precision == "mx8" else "tiny-hd64"]
    d = cfg.embed_dim
    eng = FernEngine("cuda:0")
    eng.load_tensors(synth.clip_state_dict(cfg, seed=8))
    eng.finalize_clip(cfg)
    eng.load_tensors(synth.fusion_state_dict(d, seed=9))
    eng.finalize_fusion(d)
    eng.set_precision(precision)
    n_img, n_txt = 150, 530
    imgs = _t(synth.images(n_img, cfg, 2))
    toks = _t(synth.captions(n_txt, cfg, 2, full_length=False))
    fi = eng.encode_image(imgs)
    g, s = eng.encode_text(toks)
    for i in (0, 63, 64, 65, 127, 128, 149):
        assert torch.equal(eng.encode_image(imgs[i:i + 1]), fi[i:i + 1]), i
    for i in (0, 255, 256, 257, 511, 512, 529):
        gi, si = eng.encode_text(toks[i:i + 1])
        assert torch.equal(gi, g[i:i + 1]) and torch.equal(si, s[i:i + 1]), i
    b = 300
    loc = _t(synth.local_feats(b, d, 3))
    fused = eng.dvr_fuse(fi[:1].expand(b, -1).contiguous() + g[:b] * 0.1, loc, g[:b], s[:b])
    for i in (0, 255, 256, 299):
        one = eng.dvr_fuse((fi[:1] + g[i:i + 1] * 0.1).contiguous(), loc[i:i + 1], g[i:i + 1], s[i:i + 1])
        assert torch.equal(one, fused[i:i + 1]), i
    assert torch.isfinite(fused).all()
    eng.close()


@pytest.mark.parametrize("cfg_name,b,precision", [(c, b, p) for c, b in [("ViT-B-16", 64), ("ViT-B-16", 5), ("tiny", 7)]
                                                    for p in ["fp32", "f32x3", "bf16", "mx8img"]] +
                         [("ViT-B-16", b, p) for b in (65, 130) for p in ("fp32", "mx8img")])
def test_encode_pair_is_bit_identical_to_the_two_encoder_calls(cfg_name, b, precision):
    """fern_encode_pair (round 6): both towers of a query batch walked layer by layer, the text layer's GEMMs riding in the image layer's
    launches (gemm.hip: gemm_f32_pair_kernel, once the image GEMM's tuned plan is a mixed plan -- the second call of a shape).  Same tiles,
    same k order: image features, text global and text seq equal fern_vit_encode_image + fern_text_encode BIT FOR BIT, on the first call
    (two launches per pair while the shapes are tuned), on later calls (one launch), with pairing switched off by a forced tile, and in a
    mode the library does not pair (bf16: the two calls).  b = 65 / 130: the pair path cuts batches above 64 into chunks of 64."""
    cfg, _, eng = tower_engine(cfg_name, seed=4)
    if precision in ("bf16", "mx8img") and cfg_name == "tiny":
        eng.close()
        pytest.skip("the tiny tower's widths are outside the reduced-precision modes")
    eng.set_precision(precision)
    imgs = torch.from_numpy(synth.images(b, cfg, 11)).cuda()
    toks = torch.from_numpy(synth.captions(b, cfg, 11)).cuda()
    ref_i = eng.encode_image(imgs)
    ref_g, ref_s = eng.encode_text(toks)
    for rep in range(3):                                   # 1st: shapes seen for the first time by the pair launcher; 2nd, 3rd: tuned plans
        pi, pg, ps = eng.encode_pair(imgs, toks)
        assert torch.equal(pi, ref_i) and torch.equal(pg, ref_g) and torch.equal(ps, ref_s), (cfg_name, b, precision, rep)
    if precision in ("fp32", "f32x3") and cfg_name == "ViT-B-16" and b == 64:
        # both forms of every pair, whatever the pair tuner chose on this box: flip each exported "pair ... 0|1" line, import, compare bits
        pairs = [ln for ln in eng.tuner_export().splitlines() if ln.startswith("pair ")]
        assert len(pairs) >= 3, pairs                      # QKV / out-proj / c_fc / c_proj of the ViT-B/16 + text layers (those whose image plan is a mixed plan)
        flipped = "\n".join(ln[:-1] + ("0" if ln.endswith("1") else "1") for ln in pairs) + "\n"
        eng.tuner_import(flipped)
        assert all(ln in eng.tuner_export() for ln in flipped.splitlines())
        pi, pg, ps = eng.encode_pair(imgs, toks)
        assert torch.equal(pi, ref_i) and torch.equal(pg, ref_g) and torch.equal(ps, ref_s), "one-launch and two-launch forms of a pair differ"
        eng.tuner_import("\n".join(pairs) + "\n")
    if precision == "mx8img" and b == 64:
        # the mixed mode's pairs (gemm_bf16.hip: launch_gemm_mxbf_pair): two launches / the 16-wave pair kernel / the 8-wave one, all three
        # forms of every pair whatever the pair tuner chose on this box
        pairs = [ln for ln in eng.tuner_export().splitlines() if ln.startswith("pairb ")]
        assert len(pairs) == 4, pairs                      # QKV / out-proj / c_fc / c_proj of the ViT-B/16 + text layers
        for choice in "012":
            forced = "\n".join(ln.rsplit(" ", 1)[0] + " " + choice for ln in pairs) + "\n"
            eng.tuner_import(forced)
            assert all(ln in eng.tuner_export() for ln in forced.splitlines())
            pi, pg, ps = eng.encode_pair(imgs, toks)
            assert torch.equal(pi, ref_i) and torch.equal(pg, ref_g) and torch.equal(ps, ref_s), f"pair form {choice} differs from the two calls"
        eng.tuner_import("\n".join(pairs) + "\n")
    pi, pg, ps = eng.encode_pair(imgs, toks, want_seq=False)      # global only: the pooled-row projection, as encode_text(want_seq=False) computes it
    assert ps is None and torch.equal(pi, ref_i) and torch.equal(pg, eng.encode_text(toks, want_seq=False)[0])
    if precision in ("fp32", "f32x3"):
        eng.tuner_force_config("f32" if precision == "fp32" else "f32x3", 0)      # a forced tile: the pair launcher makes two launches
        try:
            pi, pg, ps = eng.encode_pair(imgs, toks)
            assert torch.equal(pi, ref_i) and torch.equal(pg, ref_g) and torch.equal(ps, ref_s)
        finally:
            eng.tuner_force_config("f32" if precision == "fp32" else "f32x3", -1)
    with pytest.raises(ValueError):
        eng.encode_pair(imgs, toks[:-1])
    eng.close()


@pytest.mark.parametrize("precision", ["fp32", "mx8img"])
@pytest.mark.parametrize("v_layers,t_layers", [(4, 1), (2, 3)])
def test_encode_pair_walks_the_unpaired_tail_layers(v_layers, t_layers, precision):
    """Towers of unequal depth: fern_encode_pair pairs the layers both towers have and walks the deeper tower's remaining blocks alone
    (4 + 1: three full image blocks, one paired, an image tail of two; 2 + 3: one paired, a text tail of two), in the fp32 data flow and in
    the mixed mode (tiny-w256: widths that are multiples of 128, head_dim 64, so mx8img pairs).  Bit for bit the two encoder calls, on the
    first call (which tunes) and the second (which may take the one-launch form), with and without the seq output."""
    from dataclasses import replace
    cfg, _, eng = tower_engine(replace(synth.CLIP_CONFIGS["tiny-w256"], v_layers=v_layers, t_layers=t_layers), seed=4)
    eng.set_precision(precision)
    b = 3
    imgs = torch.from_numpy(synth.images(b, cfg, 11)).cuda()
    toks = torch.from_numpy(synth.captions(b, cfg, 11)).cuda()
    ref_i = eng.encode_image(imgs)
    ref_g, ref_s = eng.encode_text(toks)
    for rep in range(2):
        pi, pg, ps = eng.encode_pair(imgs, toks)
        assert torch.equal(pi, ref_i) and torch.equal(pg, ref_g) and torch.equal(ps, ref_s), rep
    pi, pg, ps = eng.encode_pair(imgs, toks, want_seq=False)
    assert ps is None and torch.equal(pi, ref_i) and torch.equal(pg, eng.encode_text(toks, want_seq=False)[0])
    eng.close()

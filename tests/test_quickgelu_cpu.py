"""CPU: the QuickGELU CLIP towers' oracle, fixture, arithmetic, configs, driver flags and ABI (no GPU needed).

Bounds.  Oracle against the in-tree statement run with hidden_act="quick_gelu": test_clip_oracle_matches_in_tree_statement's
(2e-5 on the tiny towers, 2e-4 at full size; measured 9.5e-7 image / 1.2e-6 text on tiny and tiny-hd64).  quick_gelu2
(csrc/gemm_epilogue.h) restated in float32, operation for operation, against float64 x * sigmoid(1.702 x) on [-30, 30]:
max |error| <= 1.5e-6 -- twice the 7.4e-7 measured with numpy's exp2 (the hardware's v_exp_f32 / v_rcp_f32 are 1-ulp
instructions: the same order); the error is absolute because the far negative tail loses RELATIVE accuracy (3.3e-6) to the
rounding of the exp2 argument, where the values themselves are below 1e-20.
"""
import numpy as np
import pytest
import torch

from fashionern_aaai2024_amd import _lib, synth
from oracle import clip as oclip, fusion as ofusion

import quickgelu_oracle as qo
from support import t

CLIP_SEED, INPUT_SEED = 5, 42
TOWERS = [("tiny", 5, 6, 2e-5), ("tiny-hd64", 5, 6, 2e-5), ("ViT-B-16", 2, 2, 2e-4)]


# ---- 1. patched oracle against the fixture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_img,n_txt,tol", TOWERS)
def test_patched_oracle_matches_in_tree_statement_with_quick_gelu(name, n_img, n_txt, tol):
    gold = qo.load_goldens()
    cfg = synth.CLIP_CONFIGS[name]
    sd = ofusion.as_torch(synth.clip_state_dict(cfg, seed=CLIP_SEED))
    with torch.no_grad(), qo.quick_gelu() as oc:
        img = oc.encode_image(sd, cfg, t(synth.images(n_img, cfg, INPUT_SEED)))
        err = np.abs(img.numpy() - gold[f"{name}_image"]).max()
        print(f"{name}: image max |d| {err:.2e}")
        assert err < tol
        for tag, full in (("full", True), ("ragged", False)):
            toks = t(synth.captions(n_txt, cfg, INPUT_SEED, full_length=full))
            g, s = oc.encode_text(sd, cfg, toks)
            es, eg = np.abs(s.numpy() - gold[f"{name}_text_{tag}_seq"]).max(), np.abs(g.numpy() - gold[f"{name}_text_{tag}_global"]).max()
            print(f"{name}: text {tag} max |d| seq {es:.2e} global {eg:.2e}")
            assert es < tol and eg < tol


def test_patch_is_scoped_and_leaves_the_fusion_oracle_alone():
    import torch.nn.functional as F
    x = torch.linspace(-4, 4, 101)
    assert oclip.F is F and ofusion.F is F
    with qo.quick_gelu() as oc:
        assert oc is oclip and oclip.F is not F and ofusion.F is F
        assert torch.equal(oclip.F.gelu(x), x * torch.sigmoid(1.702 * x))
        assert torch.equal(oclip.F.gelu(x, approximate="tanh"), x * torch.sigmoid(1.702 * x))
        assert torch.equal(oclip.F.linear(x[None], x[None]), F.linear(x[None], x[None]))      # everything else is forwarded
    assert oclip.F is F
    with pytest.raises(RuntimeError):      # restored when the body raises
        with qo.quick_gelu():
            raise RuntimeError("x")
    assert oclip.F is F


# ---- 2. the fixture discriminates -------------------------------------------------------------------------------------------------
def test_fixture_differs_from_the_gelu_fixture_everywhere():
    import os
    quick = qo.load_goldens()
    with np.load(os.path.join(qo.GOLD, "clip.npz")) as gelu:
        assert sorted(quick) == sorted(gelu.files)
        for k in sorted(quick):
            assert quick[k].shape == gelu[k].shape and quick[k].dtype == np.float32
            d = np.abs(quick[k] - gelu[k]).max()
            print(f"{k}: max |quick - gelu| {d:.2e}")
            assert d > 1e-3, k


# ---- 3. quick_gelu2's arithmetic --------------------------------------------------------------------------------------------------
def quick_gelu2_f32(x):
    """csrc/gemm_epilogue.h:quick_gelu2, one float32 operation per line of the kernel."""
    x = x.astype(np.float32)
    c = np.float32(-1.702) * np.float32(1.4426950408889634)      # folded by the compiler in float, like this
    with np.errstate(over="ignore"):
        w = x * c
        e = np.exp2(w)                                           # v_exp_f32; +inf for x << 0
        d = e + np.float32(1.0)
        r = np.float32(1.0) / d                                  # v_rcp_f32; 1 / inf = 0
    y = x * r
    assert y.dtype == np.float32
    return y


def test_quick_gelu2_restatement_against_float64():
    x = np.concatenate([np.linspace(-30, 30, 600001), np.linspace(-2, 2, 400001)]).astype(np.float32)
    ref = x.astype(np.float64) / (1.0 + np.exp(-1.702 * x.astype(np.float64)))
    y = quick_gelu2_f32(x)
    err = np.abs(y.astype(np.float64) - ref).max()
    print(f"quick_gelu2 fp32 vs float64 on [-30, 30]: max |error| {err:.2e}")
    assert err <= 1.5e-6
    # the limits: exp2 overflows to +inf for x << 0 (rcp -> 0, the product is -0) and underflows to 0 for x >> 0 (x * 1)
    far = quick_gelu2_f32(np.array([-1000.0, -80.0, 80.0, 1000.0, 0.0], dtype=np.float32))
    assert np.array_equal(far, np.array([-0.0, -0.0, 80.0, 1000.0, 0.0], dtype=np.float32)) and np.isfinite(far).all()


# ---- 4. configs -------------------------------------------------------------------------------------------------------------------
def test_resolve_clip_config_and_quickgelu_names():
    import dataclasses
    assert [f.name for f in dataclasses.fields(synth.ClipConfig)][-1] == "quick_gelu"
    for base in ("ViT-B-32", "ViT-B-16", "ViT-L-14", "ViT-L-14-336"):
        q, g = synth.resolve_clip_config(base + "-quickgelu"), synth.resolve_clip_config(base)
        assert q.quick_gelu and not g.quick_gelu and q.name == base + "-quickgelu"
        assert dataclasses.replace(q, name=base, quick_gelu=False) == g      # the same shapes
        assert synth.resolve_clip_config(base + "-quickgelu", force_quick_gelu=True) == q
    for name in ("ViT-B-16", "RN50x4"):
        plain, forced = synth.resolve_clip_config(name), synth.resolve_clip_config(name, force_quick_gelu=True)
        assert plain is synth.CLIP_CONFIGS[name] and not plain.quick_gelu
        assert forced.quick_gelu and dataclasses.replace(forced, quick_gelu=False) == plain
    inst = dataclasses.replace(synth.CLIP_CONFIGS["tiny"], name="mine")
    assert synth.resolve_clip_config(inst) is inst
    assert synth.resolve_clip_config(inst, True) == dataclasses.replace(inst, quick_gelu=True)
    assert all(not c.quick_gelu for n, c in synth.CLIP_CONFIGS.items() if not n.endswith("-quickgelu"))
    with pytest.raises(KeyError):
        synth.resolve_clip_config("no-such-tower")


@pytest.mark.parametrize("name", ["tiny", "tiny-resnet"])
def test_weights_do_not_depend_on_the_activation(name):
    a = synth.clip_state_dict(synth.resolve_clip_config(name), seed=CLIP_SEED)
    b = synth.clip_state_dict(synth.resolve_clip_config(name, force_quick_gelu=True), seed=CLIP_SEED)
    assert list(a) == list(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    cfg = synth.resolve_clip_config(name)
    assert np.array_equal(synth.images(2, cfg, INPUT_SEED), synth.images(2, synth.resolve_clip_config(name, True), INPUT_SEED))


# ---- 5. drivers -------------------------------------------------------------------------------------------------------------------
def test_driver_parsers_take_force_quick_gelu():
    from fashionern_aaai2024_amd.run import _cli, extract_patch
    for kind in ("fiq", "val", "cirr", "shoes", "200k"):
        assert _cli.build_parser(kind).parse_args([]).force_quick_gelu is False
        args = _cli.build_parser(kind).parse_args(["--force-quick-gelu", "--clip-model-name", "RN50x4"])
        assert args.force_quick_gelu is True and args.clip_model_name == "RN50x4"
    base = ["--images", "in", "--out", "out"]
    assert extract_patch.build_parser().parse_args(base).force_quick_gelu is False
    assert extract_patch.build_parser().parse_args(base + ["--force-quick-gelu"]).force_quick_gelu is True


# ---- 6. ABI -----------------------------------------------------------------------------------------------------------------------
def test_set_activation_validates_before_any_hip_call_and_abi_is_unchanged():
    lib = _lib.load()
    assert lib.fern_abi_version() == 3
    assert lib.fern_clip_set_activation(None, 1) == -1
    assert b"ctx is NULL" in lib.fern_last_error() and b"fern_clip_set_activation" in lib.fern_last_error()
    from fashionern_aaai2024_amd import engine
    assert (engine.EPI_BIAS_QUICKGELU, engine.ACT_GELU, engine.ACT_QUICK_GELU) == (4, 0, 1)
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib.os.path.dirname(_lib.os.path.abspath(_lib.__file__))), "include", "fern.h")).read()
    for text in ("FERN_EPI_BIAS_QUICKGELU = 4", "FERN_ACT_GELU = 0", "FERN_ACT_QUICK_GELU = 1", "#define FERN_ABI_VERSION 3"):
        assert text in hdr
    assert [n for n, _ in _lib.ClipConfigC._fields_][-3:] == ["r_layers", "r_width", "r_heads"]      # no field added to fern_clip_config

"""The ModifiedResNet tower's kernels one by one (include/fern.h: fern_conv3x3_nhwc, fern_conv1x1_nhwc, fern_stem_conv,
fern_avgpool_nhwc, fern_attnpool_tokens): each entry is the tower's own launcher behind an argument check, each reference is torch's
conv2d / avg_pool2d / indexing on the CPU in float64 (tests/resnet_refs.py) -- not the oracle's restatement of the tower.

Bounds.  Everything GEMM-shaped: the fp32 family's bound (gemm_refs.close: max abs error <= 2e-5 x max|ref|), and bit equality where
the arithmetic is exact (integer operands, one-tap weights, forced tiles, batch slices).  The pool and the token mean: derived from the
operation count (k^2 - 1 additions and a multiply: k^2 x 2^-23 x max|x|; HW additions and a multiply: HW x 2^-23 x max|x|)."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import gemm_refs
import resnet_refs as R
from fashionern_aaai2024_amd import synth
from fashionern_aaai2024_amd._lib import FernError
from fashionern_aaai2024_amd.engine import FernEngine
from oracle import clip as oclip
from oracle import fusion as ofusion

pytestmark = pytest.mark.gpu

# (b, H, W, cin, cout)
CONV3 = [
    (3, 1, 1, 16, 16),         # eight of nine taps outside the image for every pixel
    (2, 2, 2, 48, 80),         # RN50x4's padded stem width (three k tiles per tap), N = 80
    (3, 5, 5, 16, 96),         # M = 75: image boundaries inside one 32-row MFMA tile
    (7, 4, 4, 32, 32),         # tiny-resnet
    (2, 9, 9, 80, 80),         # RN50x4's last grid, M = 162: ragged second row tile
    (5, 7, 7, 160, 160),       # the 128x160 tile's width
    (1, 18, 18, 320, 320),
    (2, 3, 6, 16, 32),         # the loader's x / y roles on a non-square grid
]
CONV3_TILED = [(2, 2, 2, 48, 80), (3, 5, 5, 16, 96), (2, 9, 9, 80, 80), (5, 7, 7, 160, 160)]
CONV3_TILES = (8, 9, 10, 11, 14, 15)      # the six instantiations of the 3x3-window loader
CONV1 = [(162, 320, 80), (75, 96, 16), (245, 640, 160), (50, 80, 48), (8, 2560, 640)]      # (M, N, K)
STEM = [(3, 2, 16), (2, 10, 16), (1, 64, 32), (2, 34, 48), (2, 32, 48)]      # (b, S, cout_pad); 48: the per-pixel kernel, 578 / 512 pixels
POOL = [(3, 2, 16, 2), (2, 6, 48, 2), (2, 18, 80, 2), (1, 8, 32, 4)]         # (b, H, C, k)
TOKENS = [(3, 1, 64), (2, 4, 1024), (2, 81, 2560)]                           # (b, HW, C)


def _first_diff(got, want):
    """'' when equal, else the index and values of the first differing element and how many differ."""
    ne = (got != want).nonzero()
    if ne.numel() == 0:
        return ""
    i = tuple(ne[0].tolist())
    return f"{ne.shape[0]} elements differ, first at {i}: got {got[i].item()!r}, want {want[i].item()!r}"


def _conv3(engine, x, w4, bias):
    return engine.conv3x3_nhwc(x, R.conv3_rows(w4), bias).cpu()


# ---- 3x3 convolution through the window loader ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CONV3)
def test_conv3x3_against_fp64(engine, case):
    x, w4, bias, ref = R.conv3_case(*case)
    gemm_refs.close(_conv3(engine, x, w4, bias), ref)


@pytest.mark.parametrize("case", CONV3)
def test_conv3x3_is_exact_on_integer_data(engine, case):
    x, w4, bias, ref = R.conv3_case(*case, integer=True)
    got = _conv3(engine, x, w4, bias)
    assert torch.equal(got.double(), ref), _first_diff(got.double(), ref)


@pytest.mark.parametrize("case", CONV3)
def test_conv3x3_every_tap_reads_its_own_pixel(engine, case):
    """Weights that copy channel c from ONE tap: the output is the input shifted by that tap, exact zeros where the tap leaves the image."""
    b, H, W, cin, cout = case
    x = R.conv3_case(*case)[0].abs() + 0.5
    zero = torch.zeros(cout)
    for ky in range(3):
        for kx in range(3):
            got = _conv3(engine, x, R.tap_weights(cin, cout, ky, kx), zero)
            want = R.tap_shift(x, cout, ky, kx)
            assert torch.equal(got, want), f"tap (ky={ky}, kx={kx}) of {case}, index (b, y, x, c): {_first_diff(got, want)}"


@pytest.mark.parametrize("case", CONV3_TILED)
def test_conv3x3_every_tile_is_bit_identical(engine, case):
    x, w4, bias, ref = R.conv3_case(*case)
    free = _conv3(engine, x, w4, bias)
    gemm_refs.close(free, ref)
    try:
        for cfg in CONV3_TILES:
            engine.tuner_force_config("f32", cfg)
            got = _conv3(engine, x, w4, bias)
            assert torch.equal(got, free), f"tile {cfg} of {case}: {_first_diff(got, free)}"
    finally:
        engine.tuner_force_config("f32", -1)


@pytest.mark.parametrize("case", [c for c in CONV3 if c[0] > 1])
def test_conv3x3_batch_invariance(engine, case):
    x, w4, bias, _ = R.conv3_case(*case)
    full = _conv3(engine, x, w4, bias)
    for i in range(case[0]):
        alone = _conv3(engine, x[i:i + 1], w4, bias)
        assert torch.equal(alone, full[i:i + 1]), f"image {i} of {case}: {_first_diff(alone, full[i:i + 1])}"


def test_conv3x3_under_f32x3_and_back(engine):
    fp32 = [_conv3(engine, *R.conv3_case(*case)[:3]) for case in CONV3]
    try:
        engine.set_precision("f32x3")
        for case in CONV3:
            x, w4, bias, ref = R.conv3_case(*case)
            gemm_refs.close(_conv3(engine, x, w4, bias), ref)
    finally:
        engine.set_precision("fp32")
    for case, want in zip(CONV3, fp32):
        assert torch.equal(_conv3(engine, *R.conv3_case(*case)[:3]), want), case


# ---- 1x1 convolution: the bottleneck's three epilogues ----------------------------------------------------------------------------
def _conv1_forms(engine, a, w, bias, r):
    """bias | bias + ReLU | bias + residual + ReLU, on the device"""
    return (engine.conv1x1_nhwc(a, w, bias, relu=False), engine.conv1x1_nhwc(a, w, bias), engine.conv1x1_nhwc(a, w, bias, residual=r))


def _conv1_refs(base, r):
    return base, F.relu(base), F.relu(base + r.double())


@pytest.mark.parametrize("case", CONV1)
def test_conv1x1_three_epilogues_against_fp64(engine, case):
    a, w, bias, r, base = R.conv1_case(*case)
    for got, ref in zip(_conv1_forms(engine, a, w, bias, r), _conv1_refs(base, r)):
        gemm_refs.close(got, ref)


@pytest.mark.parametrize("case", CONV1)
def test_conv1x1_is_exact_on_integer_data(engine, case):
    a, w, bias, r, base = R.conv1_case(*case, integer=True)
    for form, (got, ref) in enumerate(zip(_conv1_forms(engine, a, w, bias, r), _conv1_refs(base, r))):
        got = got.cpu().double()
        assert torch.equal(got, ref), f"form {form} of {case}: {_first_diff(got, ref)}"


def _conv1_tiles(M, K):
    """Every tile of the fp32 family that takes the shape itself: 32-wide k tiles need K % 32 == 0, the small-M kernel M <= 128 and
    K % 64 == 0 (the launcher would put another tile in the place of one that does not fit)."""
    tiles = [c for c in (0, 1, 2, 3) if K % 32 == 0]
    if M <= 128 and K % 64 == 0:
        tiles.append(6)
    return tiles + [8, 9, 10, 11, 12, 13, 14, 15]


@pytest.mark.parametrize("case", CONV1)
def test_conv1x1_every_tile_is_bit_identical(engine, case):
    M, N, K = case
    a, w, bias, r, base = R.conv1_case(*case)
    a, w, bias, r = (t.cuda() for t in (a, w, bias, r))
    free = _conv1_forms(engine, a, w, bias, r)
    gemm_refs.close(free[2], F.relu(base + r.cpu().double()))
    tiles = _conv1_tiles(M, K)
    assert {8, 9, 10, 11, 14, 15} <= set(tiles)
    try:
        for cfg in tiles:
            engine.tuner_force_config("f32", cfg)
            for form, (got, want) in enumerate(zip(_conv1_forms(engine, a, w, bias, r), free)):
                assert torch.equal(got, want), f"tile {cfg}, form {form} of {case}: {_first_diff(got.cpu(), want.cpu())}"
    finally:
        engine.tuner_force_config("f32", -1)


# ---- stem convolution: the generic kernel and the one-thread-per-pixel kernel of cout_pad == 48 ----------------------------------
def _stem(engine, img, w4, bias):
    return engine.stem_conv(img, w4.reshape(w4.shape[0], 27), bias).cpu()


@pytest.mark.parametrize("case", STEM)
def test_stem_against_fp64_and_zero_channels(engine, case):
    img, w4, bias, ref = R.stem_case(*case)
    got = _stem(engine, img, w4, bias)
    assert got.shape == ref.shape
    gemm_refs.close(got, ref)
    pad = got[..., R.stem_zero_channels(case[2])]
    assert pad.numel() > 0 and torch.equal(pad, torch.zeros_like(pad))      # +0.0 exactly: what the next convolution's padded k reads


@pytest.mark.parametrize("case", STEM)
def test_stem_is_exact_on_integer_data(engine, case):
    img, w4, bias, ref = R.stem_case(*case, integer=True)
    got = _stem(engine, img, w4, bias).double()
    assert torch.equal(got, ref), _first_diff(got, ref)


@pytest.mark.parametrize("case", [c for c in STEM if c[2] == 48])
def test_stem_per_pixel_kernel_equals_the_generic_kernel(engine, case):
    """An output channel's fma chain does not depend on how many channels there are: the 48 operand rows zero-padded to 64 run the
    generic kernel, whose first 48 channels must be the per-pixel kernel's output bit for bit."""
    img, w4, bias, _ = R.stem_case(*case)
    px = _stem(engine, img, w4, bias)
    w64, b64 = torch.zeros(64, 3, 3, 3), torch.zeros(64)
    w64[:48], b64[:48] = w4, bias
    generic = _stem(engine, img, w64, b64)
    assert torch.equal(generic[..., :48], px), _first_diff(generic[..., :48], px)
    assert torch.equal(generic[..., 48:], torch.zeros_like(generic[..., 48:]))


# ---- average pool ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", POOL)
def test_avgpool_against_fp64(engine, case):
    b, H, C, k = case
    x, ref = R.avgpool_case(*case)
    got = engine.avgpool_nhwc(x, k).cpu()
    assert got.shape == ref.shape
    err = (got.double() - ref).abs().max().item()
    assert err <= k * k * 2.0 ** -23 * x.abs().max().item(), err


@pytest.mark.parametrize("case", POOL)
def test_avgpool_reads_the_right_elements(engine, case):
    x, ref = R.avgpool_case(*case, coded=True)
    got = engine.avgpool_nhwc(x, case[3]).cpu().double()
    assert torch.equal(got, ref), f"index (b, y, x, c): {_first_diff(got, ref)}"


# ---- attention-pool token builder -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TOKENS)
def test_attnpool_tokens(engine, case):
    b, HW, C = case
    x, pos, rows, mean = R.tokens_case(*case)
    T, T0 = engine.attnpool_tokens(x, pos)
    T, T0 = T.cpu(), T0.cpu()
    assert T.shape == (b, HW + 1, C) and T0.shape == (b, C)
    assert torch.equal(T[:, 1:], rows), f"index (b, token - 1, c): {_first_diff(T[:, 1:], rows)}"      # one fp32 add each
    err = (T[:, 0].double() - mean).abs().max().item()
    assert err <= HW * 2.0 ** -23 * x.abs().max().item(), err
    assert torch.equal(T0, T[:, 0])


# ---- what the entries refuse (before any launch) ------------------------------------------------------------------------------------
def test_entries_refuse_what_the_launchers_cannot_serve(engine):
    z = torch.zeros
    odd = z(2 * 2 * 16 + 1, device="cuda")[1:].reshape(1, 2, 2, 16)      # contiguous, 4 bytes off a 16-byte boundary
    refused = [
        ("cin % 16", lambda: engine.conv3x3_nhwc(z(1, 2, 2, 24), z(16, 216), z(16))),
        ("16-byte aligned", lambda: engine.conv3x3_nhwc(odd, z(16, 144), z(16))),
        ("cin % 16", lambda: engine.conv1x1_nhwc(z(4, 24), z(16, 24), z(16))),
        ("before the ReLU only", lambda: engine.conv1x1_nhwc(z(4, 16), z(16, 16), z(16), residual=z(4, 16), relu=False)),
        ("S % 2", lambda: engine.stem_conv(z(1, 3, 5, 5), z(16, 27), z(16))),
        ("cout_pad % 4", lambda: engine.stem_conv(z(1, 3, 4, 4), z(6, 27), z(6))),
        ("H % k", lambda: engine.avgpool_nhwc(z(1, 6, 6, 16), 4)),
        ("C % 4", lambda: engine.avgpool_nhwc(z(1, 4, 4, 6), 2)),
        ("C % 4", lambda: engine.attnpool_tokens(z(1, 4, 6), z(5, 6))),
        ("bad argument", lambda: engine.attnpool_tokens(z(1, 0, 16), z(1, 16))),
    ]
    for text, call in refused:
        with pytest.raises(FernError, match=text):
            call()
    assert engine.conv3x3_nhwc(z(0, 2, 2, 16), z(16, 144), z(16)).shape == (0, 2, 2, 16)      # nothing to do is not an error


# ---- one small tower that reaches RN50x4's own paths --------------------------------------------------------------------------------
def test_width_80_tower_against_the_oracle():
    """RN50x4 cut to 64 px and one bottleneck per stage: width 80, the stem padded 40 -> 48 (per-pixel stem kernel, conv_c = 48 / 80),
    N = 80 / 160 / 320 / 640, E = 2560 with 40 heads over 5 tokens -- at the tiny-resnet test's own bounds.
    Measured on MI355X: max abs error 1.8e-5 at max|ref| = 10.4 (bound 2.1e-3), 1 - cosine 1.2e-7 (bound 1e-5)."""
    cfg = dataclasses.replace(synth.CLIP_CONFIGS["RN50x4"], image_size=64, r_layers=(1, 1, 1, 1))
    sd_np = synth.clip_state_dict(cfg, seed=8)
    sd = ofusion.as_torch(sd_np)
    eng = FernEngine("cuda:0")
    try:
        eng.load_tensors(sd_np)
        eng.finalize_clip(cfg)
        imgs = torch.from_numpy(synth.images(5, cfg))
        ref = oclip.encode_image(sd, cfg, imgs)
        got = eng.encode_image(imgs).cpu()
        err = (got.double() - ref.double()).abs().max().item()
        scale = max(1.0, ref.abs().max().item())
        cos = (1 - F.cosine_similarity(got, ref, dim=-1)).abs().max().item()
        print(f"width-80 tower: max abs err {err:.3e}, max|ref| {ref.abs().max().item():.3e}, 1 - cos {cos:.3e}")
        assert err < 2e-4 * scale, (err, scale)
        assert cos < 1e-5, cos
        assert torch.equal(eng.encode_image(imgs[3:4]).cpu(), got[3:4])      # batch invariance of one row
    finally:
        eng.close()

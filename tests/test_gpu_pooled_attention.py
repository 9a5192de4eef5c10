"""The pooled single-query attention (fern_pooled_attention): one query per (image, head) over tokens whose K / V are never projected --
what the fp32 towers run in the last ViT block and in the ModifiedResNet's attention pool.  The reference is the PROJECTED form,
softmax(q (t Wk^T + bk)^T / sqrt(hd)) (t Wv^T + bv), in fp64 on the CPU with a non-zero key bias: the folded form takes no key bias
because a softmax drops it.

Tolerance of the kernel-level cases: 1e-5 x max|ref|.  fp32 rounding of either form is <= 7e-7 of the output scale at these shapes
(measured on the CPU against fp64), a wrong head mapping or a missing value bias is O(1)."""
import functools

import pytest
import torch

from fashionern_aaai2024_amd import synth
from oracle import clip as oclip, fusion as ofusion
from support import rand, tower_engine

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 64, 1),          # a single key
          (3, 17, 128, 4),        # hd 32
          (5, 10, 192, 3),        # hd 64, the tiny-hd64 tower
          (2, 10, 384, 8),        # hd 48
          (2, 82, 320, 4),        # hd 80
          (2, 197, 768, 12),      # the last ViT-B/16 block
          (2, 290, 256, 4)]       # more than 256 keys
REL = 1e-5


@functools.lru_cache(maxsize=None)
def _case(b, S, E, heads):
    """Operands of one shape: layer-normed-looking tokens, projection weights at the towers' scale, a NON-ZERO key bias."""
    q = rand(b, E, seed=1)
    t = rand(b, S, E, seed=2)
    wk, wv = rand(E, E, seed=3, scale=1.2 / E ** 0.5), rand(E, E, seed=4, scale=1.2 / E ** 0.5)
    bk, bv = rand(E, seed=5, scale=0.5), rand(E, seed=6, scale=0.5)
    return q, t, wk, wv, bk, bv


def _projected_ref(q, t, wk, wv, bk, bv, heads):
    """softmax(q (t Wk^T + bk)^T / sqrt(hd)) (t Wv^T + bv) per head, fp64."""
    q, t, wk, wv, bk, bv = (x.double() for x in (q, t, wk, wv, bk, bv))
    b, S, E = t.shape
    hd = E // heads
    k = (t @ wk.T + bk).reshape(b, S, heads, hd)
    v = (t @ wv.T + bv).reshape(b, S, heads, hd)
    s = torch.einsum("bhd,bjhd->bhj", q.reshape(b, heads, hd), k) / hd ** 0.5
    return torch.einsum("bhj,bjhd->bhd", torch.softmax(s, dim=-1), v).reshape(b, E)


def _check(got, ref, what):
    got = got.cpu()
    assert torch.isfinite(got).all(), what
    err, scale = (got.double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"{what}: max err {err:.3e}, max|ref| {scale:.3e}, ratio {err / scale:.2e}")
    assert err <= REL * scale, (what, err, scale)


@pytest.mark.parametrize("b,S,E,heads", SHAPES)
def test_entry_point_matches_the_projected_form(engine, b, S, E, heads):
    q, t, wk, wv, bk, bv = _case(b, S, E, heads)
    _check(engine.pooled_attention(q, t, wk, wv, bv, heads), _projected_ref(q, t, wk, wv, bk, bv, heads), (b, S, E, heads))


@pytest.mark.parametrize("b,S,E,heads", [(3, 17, 128, 4), (2, 197, 768, 12)])
def test_extreme_logits_stay_finite_and_exact(engine, b, S, E, heads):
    """q x 50: one key takes all the weight (the max subtraction).  +1e3 on every token: a huge score offset that the softmax drops."""
    q, t, wk, wv, bk, bv = _case(b, S, E, heads)
    _check(engine.pooled_attention(q * 50, t, wk, wv, bv, heads), _projected_ref(q * 50, t, wk, wv, bk, bv, heads), "q x 50")
    _check(engine.pooled_attention(q, t + 1e3, wk, wv, bv, heads), _projected_ref(q, t + 1e3, wk, wv, bk, bv, heads), "tokens + 1e3")


def test_rows_do_not_depend_on_the_batch(engine):
    q, t, wk, wv, bk, bv = _case(5, 10, 192, 3)
    full = engine.pooled_attention(q, t, wk, wv, bv, 3)
    for i in range(5):
        assert torch.equal(engine.pooled_attention(q[i:i + 1], t[i:i + 1], wk, wv, bv, 3), full[i:i + 1]), i


@pytest.mark.parametrize("name,b", [("tiny", 65), ("tiny-resnet", 129)])
def test_tower_rows_do_not_depend_on_the_batch_across_chunks(name, b):
    """b = 65 crosses the ViT walker's chunk of 64 images, b = 129 the ResNet walker's chunk of 128."""
    cfg, _, eng = tower_engine(name, 5)
    imgs = torch.from_numpy(synth.images(b, cfg, 21)).cuda()
    full = eng.encode_image(imgs)
    for i in (0, 1, 15, 16, 63, 64, b - 2, b - 1):
        assert torch.equal(eng.encode_image(imgs[i:i + 1]), full[i:i + 1]), (name, i)
    eng.close()


def _scale_key_bias(cfg, sd):
    """The key bias of the image tower's single-query attention x 100: the oracle adds it, the towers never read it."""
    if cfg.v_arch == "resnet":
        sd["visual.attnpool.k_proj.bias"] = sd["visual.attnpool.k_proj.bias"] * 100
    else:
        w = cfg.v_width
        bias = sd[f"visual.transformer.resblocks.{cfg.v_layers - 1}.attn.in_proj_bias"].copy()
        bias[w:2 * w] *= 100
        sd[f"visual.transformer.resblocks.{cfg.v_layers - 1}.attn.in_proj_bias"] = bias


@pytest.mark.parametrize("name", ["tiny", "tiny-resnet"])
def test_tower_with_a_large_key_bias_matches_the_oracle(name):
    cfg, sd_np, eng = tower_engine(name, 5, _scale_key_bias)
    imgs = torch.from_numpy(synth.images(5, cfg))
    ref = oclip.encode_image(ofusion.as_torch(sd_np), cfg, imgs)
    got = eng.encode_image(imgs).cpu()
    err, scale = (got - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    print(f"{name}: max err {err:.3e}, scale {scale:.3e}")
    assert err < 2e-4 * scale, (name, err, scale)
    eng.close()


def test_pair_path_is_bit_identical_to_the_two_encoder_calls():
    cfg, _, eng = tower_engine("tiny", 4)
    imgs = torch.from_numpy(synth.images(7, cfg, 11)).cuda()
    toks = torch.from_numpy(synth.captions(7, cfg, 11)).cuda()
    ref_i = eng.encode_image(imgs)
    ref_g, ref_s = eng.encode_text(toks)
    for rep in range(2):
        pi, pg, ps = eng.encode_pair(imgs, toks)
        assert torch.equal(pi, ref_i) and torch.equal(pg, ref_g) and torch.equal(ps, ref_s), rep
    eng.close()


def test_graph_replay_is_bit_identical_to_eager():
    """The three dispatches are captured with the rest of a lane's step (no allocation, no synchronisation between them)."""
    from fashionern_aaai2024_amd.clip_model import create_model
    from fashionern_aaai2024_amd.model import ERN
    from fashionern_aaai2024_amd.pipeline import ComposedQueryPipeline
    cfg = synth.CLIP_CONFIGS["tiny"]
    d = cfg.embed_dim
    clip = create_model(cfg, device="cuda:0", seed=3)
    eng = ERN(clip, d, "cuda:0", engine=clip.engine).init_random(4).engine
    gal = eng.index_fuse(torch.from_numpy(synth.global_feats(500, d, tag="pg")), torch.from_numpy(synth.local_feats(500, d, tag="pgl")), True)
    batches = [(torch.from_numpy(synth.images(9, cfg, 100 + j)).cuda(), torch.from_numpy(synth.captions(9, cfg, 100 + j)).cuda(),
                torch.from_numpy(synth.local_feats(9, d, 100 + j)).cuda()) for j in range(4)]
    eager = [eng.sim_topk(eng.dvr_fuse(eng.encode_image(im), lc, *eng.encode_text(tk)), gal, 20) for im, tk, lc in batches]
    pipe = ComposedQueryPipeline(eng, lanes=1, graphs=True)
    for _ in range(2):                                   # a lane captures its step at its third call: the later ones are replays
        for (rs, ri), (im, tk, lc) in zip(eager, batches):
            s, i = pipe.submit(im, tk, lc, gal, 20).wait()
            torch.cuda.current_stream().synchronize()
            assert torch.equal(i, ri) and torch.equal(s, rs)
    assert all(lg.graph is not None for d_ in pipe._lane_graphs for lg in d_.values())
    pipe.close()
    clip.engine.close()

"""GPU: parity at the FULL sizes of BASELINE.json's configs, through size-independent properties where the CPU oracle
would be too slow (sortedness, idempotence, shard/merge == global, gather == top-K scores, batch invariance), plus a
direct oracle comparison on a bounded slice.

C1  RN50x4-shaped D=640, 1k gallery, B=32 (fusion + rank; the RN50x4 image tower itself: tests/test_gpu_kernels.py, test_gpu_fusion.py)
C2  ViT-B/16 D=512, B=64 vs 46k gallery
C3  D=640, ~200k gallery sharded 8 ways, all-gather == unsharded
C4  CIRR-style: B=1024 queries, K=51 with the reference removed, 6 group members per query
C5  1M-row gallery: fp32 sweep, bf16 sweep, and the whole config end to end -- ViT-B/16 towers in the per-row fp8 mode AND in the
    block-scaled fp8 mode the bench times ("mx8") -> fusion -> 1M-row bf16 gallery sweep, ranking checked against the oracle on
    the features the encoder produced
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fashionern_aaai2024_amd import synth
from fashionern_aaai2024_amd.engine import FernEngine
from oracle import chain
from oracle import fusion as ofusion
from oracle import rank as orank

import support as S

pytestmark = pytest.mark.gpu


def fused_engine(d):
    return S.fusion_engine(d, seed=21)


def unit(n, d, tag):
    return torch.from_numpy(synth.unit_rows(n, d, tag=tag))


def assert_same_order_up_to_near_ties(q, g, idx, ref_idx, gap=2e-6):
    """The torch oracle sums in BLAS order, the HIP sweep in its own fixed order: the two rankings may differ only where the
    oracle's own fp64-checked scores of the swapped rows are closer than fp32 rounding (`gap`)."""
    rows = sorted(set((idx != ref_idx).nonzero()[:, 0].tolist()))
    S.assert_same_order_up_to_near_ties({r: q[r].double() @ g.double().T for r in rows}, idx, ref_idx, gap)


def check_sorted_and_consistent(eng, q, g, s, i):
    s_c, i_c = s.cpu(), i.cpu()
    assert (s_c[:, :-1] >= s_c[:, 1:]).all(), "scores must be sorted descending"
    ties = s_c[:, :-1] == s_c[:, 1:]
    assert (i_c[:, :-1][ties] < i_c[:, 1:][ties]).all(), "ties must be ordered by ascending index"
    assert (i_c >= 0).all() and (i_c < g.shape[0]).all()
    for row in range(min(4, q.shape[0])):
        assert len(set(i_c[row].tolist())) == i_c.shape[1], "an index may appear only once"
    # the reported score is the dot product of the reported row (independent kernel: wave-reduced gather)
    gs = eng.gather_scores(q, g, i).cpu()
    assert (gs - s_c).abs().max().item() < 1e-5


@pytest.mark.parametrize("precision", ["fp32", "f32x3"])
def test_c1_rn50x4_shape_fusion_and_rank(precision):
    d, n, b = 640, 1000, 32
    eng, sd = fused_engine(d)
    eng.set_precision(precision)
    raw, loc = torch.from_numpy(synth.global_feats(n, d, tag="c1")), torch.from_numpy(synth.local_feats(n, d, tag="c1l"))
    gal = eng.index_fuse(raw, loc, normalize_input=True)
    ref = ofusion.index_fuse(sd, F.normalize(raw, dim=-1), loc)
    assert (gal.cpu() - ref).abs().max().item() < 2e-5
    rg, rl = torch.from_numpy(synth.global_feats(b, d, tag="c1q")), torch.from_numpy(synth.local_feats(b, d, tag="c1ql"))
    tg, ts = torch.from_numpy(synth.global_feats(b, d, tag="c1t")), torch.from_numpy(synth._normal(1, "c1ts", (b, 77, d)))
    q = eng.dvr_fuse(rg, rl, tg, ts)
    qr = ofusion.dvr_fuse(sd, rl, ts, rg, tg)
    assert (q.cpu() - qr).abs().max().item() < 5e-5
    s, i = eng.sim_topk(q, gal, 50)
    rs, ri = orank.cosine_topk(qr, ref, 50)
    assert (s.cpu() - rs).abs().max().item() < 1e-3
    full = qr @ ref.T
    S.assert_same_order_up_to_near_ties(full, i, ri, gap=1e-5)       # only near-ties of the oracle itself may swap
    ps, pi = eng.sim_topk(q, eng.prepare_gallery(gal), 50)           # the prepared form (bf16 pre-filter + exact rescoring): same bits
    assert torch.equal(ps, s) and torch.equal(pi, i)
    eng.set_precision("fp32")


def test_c2_full_size_sweep_properties():
    eng, _ = fused_engine(512)
    q, g = unit(64, 512, "c2q").cuda(), unit(46000, 512, "c2g").cuda()
    s, i = eng.sim_topk(q, g, 50)
    check_sorted_and_consistent(eng, q, g, s, i)
    # idempotence: ranking only the returned rows reproduces the order
    for row in (0, 17, 63):
        sub = g[i[row].long()]
        s2, i2 = eng.sim_topk(q[row:row + 1], sub, 50)
        assert torch.equal(i2.cpu().flatten(), torch.arange(50, dtype=torch.int32))
        assert (s2.cpu().flatten() - s[row].cpu()).abs().max().item() < 1e-6
    rs, ri = orank.cosine_topk(q.cpu(), g.cpu(), 50)
    assert (s.cpu() - rs).abs().max().item() < 1e-5
    assert_same_order_up_to_near_ties(q.cpu(), g.cpu(), i.cpu(), ri)
    cs, ci = chain.chain_topk(q.cpu().numpy(), g.cpu().numpy(), 50)        # the sweep's own summation order: no tolerance at all
    assert np.array_equal(i.cpu().numpy(), ci) and np.array_equal(s.cpu().numpy().view(np.uint32), cs.view(np.uint32))
    ps, pi = eng.sim_topk(q, eng.prepare_gallery(g), 50)                    # the stage bench.py times: prepared gallery, same bits
    assert torch.equal(ps, s) and torch.equal(pi, i)


@pytest.mark.parametrize("precision", ["fp32", "f32x3"])
def test_c3_sharded_200k_gallery_matches_unsharded(precision):
    d, n, world = 640, 200_000, 8
    eng, sd = fused_engine(d)
    eng.set_precision(precision)
    raw = torch.from_numpy(synth.global_feats(n, d, tag="c3")).cuda()
    loc = torch.from_numpy(synth.local_feats(25_000, d, tag="c3l")).cuda().repeat(8, 1, 1)   # 6.6 GB of local feats: reuse a 25k block
    full = eng.index_fuse(raw, loc, normalize_input=True)
    assert abs(full.norm(dim=1).cpu() - 1).max().item() < 1e-5
    per = n // world
    shards = [eng.index_fuse(raw[r * per:(r + 1) * per], loc[r * per:(r + 1) * per], normalize_input=True) for r in range(world)]
    assert torch.equal(torch.cat(shards), full), "shard -> fuse -> all_gather must be bit-identical to the unsharded fuse"
    sel = torch.tensor([0, 1, 12_345, 99_999, 199_999])
    ref = ofusion.index_fuse(sd, F.normalize(raw[sel].cpu(), dim=-1), loc[sel].cpu())
    assert (full[sel].cpu() - ref).abs().max().item() < 2e-5
    q = unit(64, d, "c3q").cuda()
    s, i = eng.sim_topk(q, full, 50)
    check_sorted_and_consistent(eng, q, full, s, i)
    parts = [eng.sim_topk(q, shards[r], 50, idx_offset=r * per) for r in range(world)]
    ms, mi = eng.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(mi, i) and torch.equal(ms, s), "sharded ranking + merge must equal the single-GPU ranking"
    ps, pi = eng.sim_topk(q, eng.prepare_gallery(full), 50)
    assert torch.equal(ps, s) and torch.equal(pi, i), "prepared gallery (candidate-list form at this size) must rank identically"
    pparts = [eng.sim_topk(q, eng.prepare_gallery(shards[r]), 50, idx_offset=r * per) for r in range(world)]
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(parts, pparts)), "prepared shards (dense form) likewise"
    eng.set_precision("fp32")


def test_c4_cirr_1024_queries_subset_and_global():
    eng, _ = fused_engine(512)
    b, n, k = 1024, 21_552, 51
    q, g = unit(b, 512, "c4q").cuda(), unit(n, 512, "c4g").cuda()
    r = np.random.default_rng(4)
    ref_idx = torch.from_numpy(r.integers(0, n, size=b).astype(np.int32))
    members = torch.from_numpy(r.integers(0, n, size=(b, 6)).astype(np.int32))
    members[:, 0] = ref_idx                                  # the reference is one of the 6 img_set members
    s, i = eng.sim_topk(q, g, k, exclude_idx=ref_idx)
    assert not (i.cpu() == ref_idx[:, None]).any(), "the reference image must be removed from every ranking"
    check_sorted_and_consistent(eng, q, g, s, i)
    s_all, i_all = eng.sim_topk(q, g, k)
    # removing the reference == the unrestricted ranking with the reference deleted
    for row in range(0, b, 97):
        keep = i_all[row].cpu() != ref_idx[row]
        assert torch.equal(i_all[row].cpu()[keep][:k - 1], i[row].cpu()[: int(keep.sum().item())][:k - 1])
    ms = eng.gather_scores(q, g, members).cpu()
    rs = orank.gather_scores(q.cpu(), g.cpu(), members)
    assert (ms - rs).abs().max().item() < 1e-5
    rs51, ri51 = orank.cosine_topk(q[:64].cpu(), g.cpu(), k, exclude_idx=ref_idx[:64])
    assert (s[:64].cpu() - rs51).abs().max().item() < 1e-5
    assert_same_order_up_to_near_ties(q[:64].cpu(), g.cpu(), i[:64].cpu(), ri51)
    sub = slice(1000, 1024)                                                   # the last queries of the batch, exactly
    full = chain.chain_scores(q[sub].cpu().numpy(), g.cpu().numpy())
    full[np.arange(24), ref_idx[sub].numpy()] = -np.inf
    order = np.argsort(-full, axis=1, kind="stable")[:, :k]
    assert np.array_equal(i[sub].cpu().numpy(), order.astype(np.int32))
    assert np.array_equal(s[sub].cpu().numpy().view(np.uint32), np.take_along_axis(full, order, axis=1).view(np.uint32))
    pg = eng.prepare_gallery(g)                                               # prepared form, both the 1024-query and the per-GPU 128-query shape
    for lo, hi in ((0, b), (128, 256)):
        ps, pi = eng.sim_topk(q[lo:hi], pg, k, exclude_idx=ref_idx[lo:hi])
        assert torch.equal(ps, s[lo:hi]) and torch.equal(pi, i[lo:hi])
    assert torch.equal(eng.gather_scores(q, pg, members).cpu(), ms)


def test_c5_one_million_row_gallery():
    eng, _ = fused_engine(512)
    n = 1_000_000
    g = torch.from_numpy(synth.unit_rows(125_000, 512, tag="c5g")).cuda().repeat(8, 1)     # 2 GB; rows repeat every 125k
    g[125_000:] += torch.linspace(0, 1e-3, n - 125_000, device="cuda")[:, None]            # ... but are not identical
    q = unit(16, 512, "c5q").cuda()
    s, i = eng.sim_topk(q, g, 50)
    check_sorted_and_consistent(eng, q, g, s, i)
    rs, ri = orank.cosine_topk(q[:4].cpu(), g.cpu(), 50)
    assert (s[:4].cpu() - rs).abs().max().item() < 1e-4
    full = q[:4].cpu() @ g.cpu().T
    S.assert_same_order_up_to_near_ties(full, i[:4], ri, gap=1e-5)
    # sharded over 8 "ranks" with offsets
    per = n // 8
    parts = [eng.sim_topk(q, g[r * per:(r + 1) * per], 50, idx_offset=r * per) for r in range(8)]
    ms, mi = eng.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(mi, i) and torch.equal(ms, s)


def test_step_is_hipgraph_capturable():
    """After one warm-up call per shape (workspace growth, tile tuning) the launch functions only enqueue kernels, so a
    whole fuse -> rank sequence can be captured into a hipGraph and replayed with identical results."""
    d = 128
    eng, _ = fused_engine(d)
    b, n = 8, 3000
    rg, rl = torch.from_numpy(synth.global_feats(b, d, tag="gq")).cuda(), torch.from_numpy(synth.local_feats(b, d, tag="gql")).cuda()
    tg, ts = torch.from_numpy(synth.global_feats(b, d, tag="gt")).cuda(), torch.from_numpy(synth._normal(1, "gts", (b, 77, d))).cuda()
    gal = eng.index_fuse(torch.from_numpy(synth.global_feats(n, d, tag="gg")), torch.from_numpy(synth.local_feats(n, d, tag="ggl")), True)

    def step():
        q = eng.dvr_fuse(rg, rl, tg, ts)
        return eng.sim_topk(q, gal, 50)

    ref_s, ref_i = step()                       # warm-up: allocates workspaces, tunes tiles
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s, out_i = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_i, ref_i) and torch.equal(out_s, ref_s)
    rg.mul_(-1.0)                                # new inputs in the captured buffers -> new results on replay
    graph.replay()
    torch.cuda.synchronize()
    exp_s, exp_i = step()
    assert torch.equal(out_i, exp_i) and torch.equal(out_s, exp_s) and not torch.equal(exp_i, ref_i)


def test_pipeline_lanes_are_bit_identical_to_serial():
    """ComposedQueryPipeline: batches in flight on several HIP streams (forked contexts sharing one set of weights)."""
    from fashionern_aaai2024_amd.clip_model import create_model
    from fashionern_aaai2024_amd.model import ERN
    from fashionern_aaai2024_amd.pipeline import ComposedQueryPipeline
    cfg = synth.CLIP_CONFIGS["tiny"]
    d = cfg.embed_dim
    clip = create_model(cfg, device="cuda:0", seed=3)
    model = ERN(clip, d, "cuda:0", engine=clip.engine).init_random(4)
    eng = model.engine
    gal = eng.index_fuse(torch.from_numpy(synth.global_feats(5000, d, tag="pg")), torch.from_numpy(synth.local_feats(5000, d, tag="pgl")), True)
    batches = []
    for j in range(7):
        batches.append((torch.from_numpy(synth.images(9, cfg, 100 + j)).cuda(), torch.from_numpy(synth.captions(9, cfg, 100 + j)).cuda(),
                        torch.from_numpy(synth.local_feats(9, d, 100 + j)).cuda()))
    serial = []
    for im, tk, lc in batches:
        q = eng.dvr_fuse(eng.encode_image(im), lc, *eng.encode_text(tk))
        serial.append(eng.sim_topk(q, gal, 20))
    pipe = ComposedQueryPipeline(eng, lanes=3)
    # the first job of a (precision, shapes) key runs alone -- lanes drained before it, waited for -- so that the GEMM tuner's trials for its
    # shapes are not timed beside other lanes' kernels; later jobs of the key are asynchronous
    first = pipe.submit(*batches[0], gal, 20)
    assert all(st.query() for st in pipe.streams) and len(pipe._seen_jobs) == 1
    assert torch.equal(first.wait()[1], serial[0][1])
    pipe.submit(*batches[1], gal, 20)
    assert len(pipe._seen_jobs) == 1
    for _ in range(2):                                   # twice: lanes are reused with warm workspaces
        futures = [pipe.submit(im, tk, lc, gal, 20) for im, tk, lc in batches]
        for (rs, ri), fut in zip(serial, futures):
            s, i = fut.wait()
            torch.cuda.current_stream().synchronize()
            assert torch.equal(i, ri) and torch.equal(s, rs)
    # the PREPARED gallery (certified bf16 pre-filter + exact fp32 rescoring): same bits through the lanes, eager and (below) captured
    pgal = eng.prepare_gallery(gal)
    futures = [pipe.submit(im, tk, lc, pgal, 20) for im, tk, lc in batches]
    for (rs, ri), fut in zip(serial, futures):
        s, i = fut.wait()
        torch.cuda.current_stream().synchronize()
        assert torch.equal(i, ri) and torch.equal(s, rs)
    pipe.close()
    # the same stream of batches with every lane's step replayed from a hipGraph (captured at a lane's third call): identical
    # results for inputs the graph was not captured with, results of earlier replays not overwritten by later ones
    pipe = ComposedQueryPipeline(eng, lanes=3, graphs=True)
    for _ in range(3):
        futures = [pipe.submit(im, tk, lc, gal, 20) for im, tk, lc in batches]
        for (rs, ri), fut in zip(serial, futures):
            s, i = fut.wait()
            torch.cuda.current_stream().synchronize()
            assert torch.equal(i, ri) and torch.equal(s, rs)
    assert all(lg.graph is not None for d_ in pipe._lane_graphs for lg in d_.values())
    for _ in range(3):
        futures = [pipe.submit(im, tk, lc, pgal, 20) for im, tk, lc in batches]
        for (rs, ri), fut in zip(serial, futures):
            s, i = fut.wait()
            torch.cuda.current_stream().synchronize()
            assert torch.equal(i, ri) and torch.equal(s, rs)
    # a captured graph holds addresses inside its lane's workspace.  A later, bigger call on the same lane engines
    # (here: a 700-query batch -- 90 MB of candidate lists against the 64 MB first block -- eager on every lane) makes the
    # contexts re-allocate their workspaces; the old graphs must be noticed as stale and re-captured, never replayed.
    gens = [e.ws_generation() for e in pipe.engines]
    big_gal = eng.index_fuse(torch.from_numpy(synth.global_feats(60000, d, tag="pg2")), torch.from_numpy(synth.local_feats(60000, d, tag="pgl2")), True)
    big = (torch.from_numpy(synth.images(700, cfg, 300)).cuda(), torch.from_numpy(synth.captions(700, cfg, 300)).cuda(),
           torch.from_numpy(synth.local_feats(700, d, 300)).cuda())
    for _ in range(2 * len(pipe.engines)):
        pipe.submit(*big, big_gal, 50).wait()
    torch.cuda.synchronize()
    assert any(e.ws_generation() != g0 for e, g0 in zip(pipe.engines, gens)), "the bigger call was expected to move the workspaces"
    for _ in range(3):
        futures = [pipe.submit(im, tk, lc, gal, 20) for im, tk, lc in batches]
        for (rs, ri), fut in zip(serial, futures):
            s, i = fut.wait()
            torch.cuda.current_stream().synchronize()
            assert torch.equal(i, ri) and torch.equal(s, rs)
    assert all(lg.graph is None or lg.ws_generation == e.ws_generation() for e, d_ in zip(pipe.engines, pipe._lane_graphs) for lg in d_.values())
    with pytest.raises(ValueError):
        pipe.submit(*batches[0], eng.gallery_to_bf16(gal), 20, members=torch.zeros(9, 6, dtype=torch.int32, device="cuda"))
    pipe.close()
    clip.engine.close()


def _bf16_ref(q, g, k):
    """Oracle for the bf16 sweep: the same rounding of both operands, fp32 products, exact ranking (score desc, index asc)."""
    return orank.cosine_topk(q.bfloat16().float(), g.bfloat16().float(), k)


@pytest.mark.parametrize("b,n,d", [(64, 46000, 512), (5, 1000, 640), (64, 33, 64), (130, 5000, 128), (1, 100_000, 512)])
def test_bf16_gallery_sweep(b, n, d):
    eng, _ = fused_engine(512)
    q, g = unit(b, d, "bq"), unit(n, d, "bg")
    gb = eng.gallery_to_bf16(g)
    assert torch.equal(gb.cpu(), g.bfloat16()), "fp32 -> bf16 must be round-to-nearest-even"
    s, i = eng.sim_topk_bf16(q, gb, 50)
    rs, ri = _bf16_ref(q, g, 50)
    kk = min(50, n)
    assert (s.cpu()[:, :kk] - rs[:, :kk]).abs().max().item() < 2e-6          # same operands: only the fp32 summation order differs
    full = q.bfloat16().float() @ g.bfloat16().float().T
    S.assert_same_order_up_to_near_ties(full, i, ri, gap=2e-6)
    fs, fi = orank.cosine_topk(q, g, 50)                                       # vs fp32 truth: north_star's 1e-3 at the path's widths
    assert (s.cpu()[:, :kk] - fs[:, :kk]).abs().max().item() < (1e-3 if d >= 512 else 4e-3)


def test_bf16_sweep_exact_ties_and_one_million_rows():
    eng, _ = fused_engine(512)
    g = torch.Generator().manual_seed(5)
    q = torch.randint(-1, 2, (7, 64), generator=g).float() / 8          # exactly representable in bf16: exact products, many ties
    gal = torch.randint(-1, 2, (70_000, 64), generator=g).float() / 8
    ex = torch.tensor([1000, -1, 1005, 3, 2000, -1, 1001], dtype=torch.int32)
    s, i = eng.sim_topk_bf16(q, eng.gallery_to_bf16(gal), 51, idx_offset=1000, exclude_idx=ex)
    rs, ri = orank.cosine_topk(q, gal, 51, idx_offset=1000, exclude_idx=ex)
    assert torch.equal(i.cpu(), ri) and torch.equal(s.cpu(), rs)
    big = torch.from_numpy(synth.unit_rows(125_000, 512, tag="c5g")).cuda().repeat(8, 1)
    big[125_000:] += torch.linspace(0, 1e-3, 875_000, device="cuda")[:, None]
    qq = unit(64, 512, "c5q").cuda()
    bb = eng.gallery_to_bf16(big)
    s, i = eng.sim_topk_bf16(qq, bb, 50)
    s_c, i_c = s.cpu(), i.cpu()
    assert (s_c[:, :-1] >= s_c[:, 1:]).all() and (i_c >= 0).all() and (i_c < 1_000_000).all()
    rows = bb[i_c[:4].flatten().long().cuda()].float().cpu().view(4, 50, 512)
    got = (qq[:4].bfloat16().float().cpu().unsqueeze(1) * rows).sum(-1)
    assert (got - s_c[:4]).abs().max().item() < 2e-6


def test_mx8mlp_sits_between_bf16_and_mx8():
    """FERN_PREC_MX8_MLP (round 5): MX8 for the image tower's MLP pair, bf16 for LayerNorm-1 / QKV / attention / out-proj, fp32 residual
    stream; FERN_PREC_MX8_IMG (round 6): all four image-tower GEMMs block-scaled over the fp32 stream.  Both run the text tower on the
    bf16 block (round 6: equal to the bf16 mode's text features bit for bit).  Image features: bf16 <= mx8mlp <= mx8img < mx8 in distance
    from the fp32 mode's."""
    cfg = synth.CLIP_CONFIGS["ViT-B-16"]
    eng = FernEngine("cuda:0")
    eng.load_tensors(synth.clip_state_dict(cfg, seed=3))
    eng.finalize_clip(cfg)
    imgs = torch.from_numpy(synth.images(8, cfg, 5))
    toks = torch.from_numpy(synth.captions(8, cfg, 5))
    f32 = eng.encode_image(imgs), eng.encode_text(toks)[0]
    err = {}
    feats = {}
    for prec in ("bf16", "mx8mlp", "mx8img", "mx8"):
        eng.set_precision(prec)
        assert eng.precision == prec
        fi, ft = eng.encode_image(imgs), eng.encode_text(toks)[0]
        assert torch.isfinite(fi).all() and torch.isfinite(ft).all()
        feats[prec] = ft
        err[prec] = ((1 - F.cosine_similarity(fi, f32[0], dim=-1)).mean().item(), (1 - F.cosine_similarity(ft, f32[1], dim=-1)).mean().item())
    assert err["bf16"][0] <= err["mx8mlp"][0] <= err["mx8img"][0] < err["mx8"][0], err
    assert torch.equal(feats["mx8mlp"], feats["bf16"]) and torch.equal(feats["mx8img"], feats["bf16"]), "text tower of the mixed modes = the bf16 block"
    assert err["bf16"][1] < err["mx8"][1], err
    assert err["mx8mlp"][0] < 5e-3 and err["mx8img"][0] < 5e-3, err
    eng.close()


@pytest.mark.parametrize("precision", ["fp8", "mx8", "mx8mlp", "mx8img"])
def test_c5_fp8_encoder_with_bf16_similarity_end_to_end(precision):
    """BASELINE configs[4] as one path on one GPU's share: ViT-B/16 towers in an fp8 mode -- "fp8" (per-row scales) and "mx8"
    (block-scaled, the precision `bench.py --config c5` times: VERDICT r3 item 1b) -> fusion -> 1M-row bf16 gallery sweep + top-50
    (the 8-GPU form shards the gallery build and replicates this step; tests/test_distributed_cpu.py).
    The ranking is checked exactly against the oracle ON THE FEATURES THE fp8 ENCODER PRODUCED (same bf16 rounding of both
    operands); the encoder's own deviation is what test_clip_towers_{fp8,mx8}_precision bound (tests/test_gpu_fusion.py), and the
    fused queries must stay within the mode's documented distance of the fp32 mode's: cosine >= 1 - 2e-2 for the modes that put e4m3
    operands on the text tower / a bf16 residual stream under them ("fp8", "mx8"), >= 1 - 5e-3 (round 6) for the
    modes that keep Recall -- "mx8mlp" and "mx8img", the mode `bench.py --config c5` times."""
    cfg = synth.CLIP_CONFIGS["ViT-B-16"]
    eng = FernEngine("cuda:0")
    eng.load_tensors(synth.clip_state_dict(cfg, seed=3))
    eng.finalize_clip(cfg)
    eng.load_tensors(synth.fusion_state_dict(512, seed=21))
    eng.finalize_fusion(512)
    b = 8
    imgs = torch.from_numpy(synth.images(b, cfg, 5))
    toks = torch.from_numpy(synth.captions(b, cfg, 5))
    loc = torch.from_numpy(synth.local_feats(b, 512, 5))
    ref32 = eng.encode_image(imgs)
    tg32, ts32 = eng.encode_text(toks)
    fused32 = eng.dvr_fuse(ref32, loc, tg32, ts32)
    eng.set_precision(precision)
    assert eng.precision == precision
    ref = eng.encode_image(imgs)
    tg, ts = eng.encode_text(toks)
    fused = eng.dvr_fuse(ref, loc, tg, ts)
    assert torch.isfinite(fused).all() and (fused.norm(dim=-1) - 1).abs().max().item() < 1e-5
    assert not torch.equal(fused, fused32), "the mode was expected to change the towers' arithmetic"
    dist = (1 - F.cosine_similarity(fused, fused32, dim=-1)).max().item()
    assert dist < ({"mx8mlp": 5e-3, "mx8img": 5e-3}.get(precision, 2e-2)), (precision, dist)
    n = 1_000_000
    g = torch.from_numpy(synth.unit_rows(125_000, 512, tag="c5e")).cuda().repeat(8, 1)
    g[125_000:] += torch.linspace(0, 1e-3, n - 125_000, device="cuda")[:, None]
    gb = eng.gallery_to_bf16(g)
    s, i = eng.sim_topk_bf16(fused, gb, 50)
    rs, ri = _bf16_ref(fused.cpu(), gb.float().cpu(), 50)
    assert (s.cpu() - rs).abs().max().item() < 2e-6
    full = fused.cpu().bfloat16().float() @ gb.float().cpu().T
    S.assert_same_order_up_to_near_ties(full, i, ri, gap=2e-6)
    eng.close()


def test_c5_default_mode_keeps_recall_at_50_on_a_512_query_split():
    """the mode `bench.py --config c5` times must keep the metric BASELINE names.  bench.py's own quality leg
    (`retrieval_quality_leg`: gallery ENCODED under each mode, composed queries through that mode's towers and fusion, exact ranking,
    targets at uniform fp32 ranks 0..63) on a 512-query x 4 096-image split: Recall@50 of the c5 default statistically within 1 pp of
    the fp32 encoder's and top-50 overlap >= 0.93 (the 2 048-query table of the bench line: 0.942), while "mx8" -- rounds 2-5's default --
    is measurably further away."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    default = bench.WORKLOADS["c5"]["precision"]
    assert default == "mx8img"
    cfg = synth.CLIP_CONFIGS["ViT-B-16"]
    eng = FernEngine("cuda:0")
    eng.load_tensors(synth.clip_state_dict(cfg, seed=0))
    eng.finalize_clip(cfg)
    eng.load_tensors(synth.fusion_state_dict(512, seed=0))
    eng.finalize_fusion(512)
    q = bench.retrieval_quality_leg(torch, eng, cfg, 512, torch.device("cuda:0"), ["fp32", default, "mx8"], n_gallery=4096, queries=512)
    m = q["modes"]
    # delta Recall@50 is a difference of two boundary-flip counts: its standard error on this split is ~1 pp (reported by the leg), so
    # the assertion is "not below -1 pp by more than three standard errors"; the top-50 overlap is the stable statistic
    se = m[default]["delta_recall_at_50_se_pp"]
    assert 0 < se < 2.0 and m[default]["delta_recall_at_50_pp"] >= -1.0 - 3.0 * se and m[default]["top50_overlap"] >= 0.93, m
    assert m[default]["top50_overlap"] > m["mx8"]["top50_overlap"] + 0.02 and m[default]["top1_same"] > m["mx8"]["top1_same"], m
    eng.close()


@pytest.mark.parametrize("precision", ["bf16", "fp8", "mx8", "mx8mlp", "mx8img"])
def test_full_step_is_hipgraph_capturable_in_reduced_precision(precision):
    """encode -> fuse -> rank of the tiny towers in a reduced-precision mode: after a warm-up call (workspaces, bf16 / fp8 / mx8
    tile tuning) the whole step only enqueues kernels and replays from a hipGraph with identical results."""
    cfg = synth.CLIP_CONFIGS["tiny-w256" if precision in ("mx8", "mx8mlp", "mx8img") else "tiny-hd64"]
    d = cfg.embed_dim
    eng = FernEngine("cuda:0")
    eng.load_tensors(synth.clip_state_dict(cfg, seed=2))
    eng.finalize_clip(cfg)
    eng.load_tensors(synth.fusion_state_dict(d, seed=3))
    eng.finalize_fusion(d)
    eng.set_precision(precision)
    b = 6
    imgs = torch.from_numpy(synth.images(b, cfg, 1)).cuda()
    toks = torch.from_numpy(synth.captions(b, cfg, 1)).cuda()
    loc = torch.from_numpy(synth.local_feats(b, d, 1)).cuda()
    gal = torch.nn.functional.normalize(torch.randn(2000, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)), dim=-1)

    def step():
        tg, ts = eng.encode_text(toks)
        q = eng.dvr_fuse(eng.encode_image(imgs), loc, tg, ts)
        return eng.sim_topk(q, gal, 50)

    ref_s, ref_i = step()
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s, out_i = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_i, ref_i) and torch.equal(out_s, ref_s)
    imgs.mul_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    exp_s, exp_i = step()
    assert torch.equal(out_i, exp_i) and torch.equal(out_s, exp_s)
    eng.close()

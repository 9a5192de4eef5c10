"""Candidate ranking on the GPU (include/fern.h: fern_sim_topk_candidates; `FernEngine.sim_topk_candidates`): every query ranks the set
of gallery rows its own list names.

Oracle: tests/candidates_oracle.py -- oracle/chain.c scores, the set semantics in numpy, the key order of `make_keys`.  fp32 and prepared
forms: scores, indices and places bit-equal.  bf16 form: bit-equal to the filtered ranking (`sim_topk(row_filter=...)`), whose scores are
the bf16 sweep's.  Finite inputs only.

The shapes are the smallest at which each path can go wrong: D = 64 / 512 / 640 take rescore.h's ring (2, 8 and 10 deep), D = 96 / 160
have an odd number of 32-k steps (the per-lane chain); M = 1 / 6 / 33 are under one round, one round and a tail; M = 1500 / 4096 are more
lists than the 1000-row gallery has rows, so they hold duplicates, several rounds per wave, and the largest sort; K runs below and above M."""
import functools

import numpy as np
import pytest
import torch

from candidates_oracle import candidates_oracle
from framed import SENTINEL, Framed
from support import assert_same_bits, fresh_engine, gallery, ptr, unit

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR = -1             # FERN_ERR_ARG


@pytest.fixture(scope="module")
def eng():
    yield from fresh_engine()


@pytest.fixture(scope="module")
def oracle():
    return candidates_oracle()()


@functools.lru_cache(maxsize=None)
def _data(b, n, d):
    """(q, g) on the CPU, shared by every test of a shape and never changed."""
    return unit(b, d, 1000 + d + b), unit(n, d, 2000 + d)


def _lists(b, m, n, seed, lo=-3, hi=None):
    """int32 [b, m]: random entries in [lo, hi) -- a few negative, a few past the gallery."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, (n + 3) if hi is None else hi, (b, m), generator=g, dtype=torch.int32)


# ---- fp32 against the chain oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 50, 1024))
@pytest.mark.parametrize("M", (1, 6, 33, 1500, 4096))
@pytest.mark.parametrize("D", (64, 96, 160, 512, 640))
def test_fp32_equals_the_chain_oracle(eng, oracle, D, M, K):
    B, N = 7, 1000
    q, g = _data(B, N, D)
    cand = _lists(B, M, N, 7 * D + M)
    want = oracle.sim_topk_candidates(q, g, cand, K, places=True)
    got = eng.sim_topk_candidates(q.cuda(), g.cuda(), cand.cuda(), K, places=True)
    assert_same_bits(got, want, f"D={D} M={M} K={K}")
    if M >= 1500:
        assert all(len(set(row.tolist())) < M for row in cand)      # the lists hold duplicates


def test_prepared_gallery_ranks_from_its_fp32_rows(eng, oracle):
    B, N, D, M, K = 7, 1000, 512, 33, 50
    q, g = _data(B, N, D)
    cand = _lists(B, M, N, 5)
    pg = eng.prepare_gallery(g.cuda())
    assert_same_bits(eng.sim_topk_candidates(q.cuda(), pg, cand, K, places=True), oracle.sim_topk_candidates(q, g, cand, K, places=True), "prepared")


def test_lists_and_numpy_arrays_are_accepted(eng, oracle):
    B, N, D, M, K = 7, 1000, 64, 6, 6
    q, g = _data(B, N, D)
    cand = _lists(B, M, N, 6)
    want = oracle.sim_topk_candidates(q, g, cand, K)
    assert_same_bits(eng.sim_topk_candidates(q.cuda(), g.cuda(), cand.tolist(), K), want, "list")
    assert_same_bits(eng.sim_topk_candidates(q.cuda(), g.cuda(), cand.numpy().astype(np.int64), K), want, "numpy int64")


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
def test_tied_rows_come_in_index_order(eng, oracle):
    """40 gallery rows are copied to other indices and every list names both copies: a pair scores the same bits for every query."""
    B, N, D, K = 7, 1000, 512, 128
    q, g = _data(B, N, D)
    g = g.clone()
    src, dst = np.arange(40) * 7 + 3, 999 - np.arange(40) * 11
    g[dst] = g[src]
    rng = np.random.default_rng(3)
    cand = np.stack([rng.permutation(np.concatenate([src, dst, rng.integers(0, N, 20)])) for _ in range(B)]).astype(np.int32)
    want = oracle.sim_topk_candidates(q, g, cand, K, places=True)
    ws, wi = want[0].numpy(), want[1].numpy()
    tied = 0
    for b in range(B):
        for p in range(K - 1):
            if wi[b, p + 1] >= 0 and ws[b, p].view(np.int32) == ws[b, p + 1].view(np.int32):
                tied += 1
                assert wi[b, p] < wi[b, p + 1]
    assert tied >= 20 * B, f"only {tied} exactly tied neighbours inside the lists"
    got = eng.sim_topk_candidates(q.cuda(), g.cuda(), cand, K, places=True)
    assert_same_bits(got, want, "ties")
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    for b in range(B):
        for p in range(K - 1):
            if gi[b, p + 1] >= 0 and gs[b, p].view(np.int32) == gs[b, p + 1].view(np.int32):
                assert gi[b, p] < gi[b, p + 1]


# ---- cross-check against the filtered ranking, all three gallery forms -----------------------------------------------------------------
XB, XN, XD = 32, 3000, 512


@functools.lru_cache(maxsize=None)
def _cross():
    """(q, g, cand int32 [32, 400] padded with -1, tags uint32-as-int32 [N]: bit b set iff row n is in list b)."""
    q, g = _data(XB, XN, XD)
    rng = np.random.default_rng(11)
    cand = np.full((XB, 400), -1, dtype=np.int32)
    tags = np.zeros(XN, dtype=np.uint32)
    for b in range(XB):
        rows = rng.choice(XN, size=int(rng.integers(5, 401)), replace=False)
        cand[b, :len(rows)] = rows
        tags[rows] |= np.uint32(1 << b)
    return q, g, torch.from_numpy(cand), torch.from_numpy(tags.view(np.int32))


@pytest.mark.parametrize("K", (64, 200))
@pytest.mark.parametrize("form", ("fp32", "prepared", "bf16"))
def test_equals_the_filtered_ranking(eng, form, K):
    from fashionern_aaai2024_amd.engine import RowFilter
    q, g, cand, tags = _cross()
    gal = gallery(eng, g, form)
    bit = torch.tensor([1 << b for b in range(XB)], dtype=torch.int64)
    flt = RowFilter(tags.cuda(), bit, bit)
    want = eng.sim_topk(q.cuda(), gal, K, row_filter=flt)
    got = eng.sim_topk_candidates(q.cuda(), gal, cand.cuda(), K)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{form} K={K}"
    # ... with exclude_idx naming a listed row (each list's third entry)
    ex = cand[:, 2].clone()
    want = eng.sim_topk(q.cuda(), gal, K, exclude_idx=ex, row_filter=flt)
    got = eng.sim_topk_candidates(q.cuda(), gal, cand.cuda(), K, exclude_idx=ex)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{form} K={K} exclude"
    assert not bool((got[1] == ex.cuda()[:, None]).any())
    # ... and with a second tag field (bits 30-31: the row's category n % 3) so that the caller's filter and the list compose; the first
    # 30 queries only, whose list bits leave the field free
    nb = 30
    cat = (torch.arange(XN) % 3).to(torch.int64)
    both = ((tags.to(torch.int64) & 0x3FFFFFFF) | (cat << 30))
    want_cat = (torch.arange(nb) % 3).to(torch.int64)
    ref = RowFilter(both.cuda(), bit[:nb] | (3 << 30), bit[:nb] | (want_cat << 30))
    own = RowFilter((cat << 30).cuda(), 3 << 30, want_cat << 30)
    gal_q = q[:nb].cuda()
    want = eng.sim_topk(gal_q, gal, K, row_filter=ref)
    got = eng.sim_topk_candidates(gal_q, gal, cand[:nb].cuda(), K, row_filter=own)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{form} K={K} composed filters"


# ---- frames of shards ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("fp32", "bf16"))
def test_shards_merge_to_the_whole_gallery(eng, form):
    q, g, cand, _ = _cross()
    K, cut = 64, 1234
    whole = eng.sim_topk_candidates(q.cuda(), gallery(eng, g, form), cand.cuda(), K)
    halves = [eng.sim_topk_candidates(q.cuda(), gallery(eng, g[a:b].contiguous(), form), cand.cuda(), K, idx_offset=a)
              for a, b in ((0, cut), (cut, XN))]
    merged = eng.topk_merge(torch.stack([h[0] for h in halves]), torch.stack([h[1] for h in halves]))
    assert torch.equal(merged[0], whole[0]) and torch.equal(merged[1], whole[1])


# ---- query chunks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 65, 1100))
def test_query_chunks(eng, oracle, B):
    """CIRR's shape (six members per query, D = 640) below, at and past the 1024-query chunk."""
    N, D, M, K = 1000, 640, 6, 6
    q, g = _data(B, N, D)
    cand = _lists(B, M, N, 40 + B)
    ex = cand[:, 0].clone()
    want = oracle.sim_topk_candidates(q, g, cand, K, exclude_idx=ex, places=True)
    got = eng.sim_topk_candidates(q.cuda(), g.cuda(), cand.cuda(), K, exclude_idx=ex, places=True)
    assert_same_bits(got, want, f"B={B}")


# ---- framed outputs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("fp32", "bf16"))
@pytest.mark.parametrize("M,K", ((6, 50), (33, 5), (300, 7)))
def test_outputs_stay_inside_their_frames(eng, form, M, K):
    from fashionern_aaai2024_amd import _lib
    from fashionern_aaai2024_amd.engine import _stream
    B, N, D = 7, 1000, 512
    q, g = _data(B, N, D)
    gal = gallery(eng, g, form)
    cand = _lists(B, M, N, 70 + M).cuda()
    ref = eng.sim_topk_candidates(q.cuda(), gal, cand, K, places=True)
    fs, fi, fp = (Framed(B, K, K, torch.float32, SENTINEL, DEV), Framed(B, K, K, torch.int32, SENTINEL, DEV),
                  Framed(B, M, M, torch.int32, SENTINEL, DEV))
    qd = q.cuda()
    g32, g16 = (gal, None) if form == "fp32" else (None, gal)
    _lib.check(eng.lib.fern_sim_topk_candidates(eng._h, ptr(qd), ptr(g32), ptr(g16), B, N, D, ptr(cand), M, K, ptr(fs), ptr(fi), ptr(fp), 0, None, None,
                                                None, None, _stream()), "fern_sim_topk_candidates")
    torch.cuda.synchronize()
    for f, what in ((fs, "out_scores"), (fi, "out_idx"), (fp, "out_place")):
        f.assert_intact(f"{what} M={M} K={K}")
    assert_same_bits((fs.contiguous(), fi.contiguous(), fp.contiguous()), ref, f"framed {form} M={M} K={K}")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over,text", [
    (dict(M=0), "need 1<=M<=4096"), (dict(M=4097), "need 1<=M<=4096"), (dict(K=0), "need 1<=K<=1024"), (dict(K=1025), "need 1<=K<=1024"),
    (dict(tags=0x10000, mask=None), "mask or value is NULL"), (dict(cand=None), "NULL argument"),
    (dict(gallery=None, D=96), "a bf16-only gallery needs D % 64 == 0, D <= 768")])
def test_refusals_name_the_entry(eng, over, text):
    p = 0x10000                                          # never dereferenced: every call is refused before any launch
    a = dict(q=p, gallery=p, gallery_bf16=p, B=2, N=10, D=64, cand=p, M=6, K=5, out_scores=p, out_idx=p, out_place=None, idx_offset=0,
             exclude_idx=None, tags=None, mask=None, value=None, stream=None)
    a.update(over)
    assert eng.lib.fern_sim_topk_candidates(eng._h, *a.values()) == ERR
    assert eng.lib.fern_last_error().decode() == "fern_sim_topk_candidates: " + text


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", (False, True))
def test_pipeline_submit_with_candidates(graphs):
    """submit(candidates=...) equals the direct engine call, eager and replayed; a replayed graph sees the NEW lists of the same shape
    (they travel through the lane's static buffers); a bf16 gallery is accepted; candidates with items is refused."""
    from fashionern_aaai2024_amd import synth
    from fashionern_aaai2024_amd.clip_model import create_model
    from fashionern_aaai2024_amd.engine import ItemMap
    from fashionern_aaai2024_amd.model import ERN
    from fashionern_aaai2024_amd.pipeline import ComposedQueryPipeline
    cfg = synth.CLIP_CONFIGS["tiny"]
    d = cfg.embed_dim
    clip = create_model(cfg, device="cuda:0", seed=3)
    model = ERN(clip, d, "cuda:0", engine=clip.engine).init_random(4)
    e = model.engine
    n, b, m, k = 2_000, 9, 40, 50
    pg = e.prepare_gallery(e.index_fuse(torch.from_numpy(synth.global_feats(n, d, tag="cg")), torch.from_numpy(synth.local_feats(n, d, tag="cgl")), True))
    im, tk, lc = (torch.from_numpy(synth.images(b, cfg, 500)).cuda(), torch.from_numpy(synth.captions(b, cfg, 500)).cuda(),
                  torch.from_numpy(synth.local_feats(b, d, 500)).cuda())
    fq = e.dvr_fuse(e.encode_image(im), lc, *e.encode_text(tk))
    lists = [_lists(b, m, n, 900 + j).cuda() for j in range(3)]      # same shape, different contents
    ex = lists[0][:, 1].clone()
    pipe = ComposedQueryPipeline(e, lanes=1, graphs=graphs)
    for gal in (pg, pg.bf16):
        direct = [e.sim_topk_candidates(fq, gal, c, k, exclude_idx=ex, places=True) for c in lists]
        assert not torch.equal(direct[0][1], direct[1][1])
        for _ in range(2):                                           # graphs: eager twice, captured, then replayed with other lists
            futures = [pipe.submit(im, tk, lc, gal, k, exclude_idx=ex, candidates=c) for c in lists]
            for want, fut in zip(direct, futures):
                s, i = fut.wait()
                torch.cuda.current_stream().synchronize()
                assert_same_bits((s, i, fut.place), want, "pipeline")
    if graphs:
        assert all(lg.graph is not None for d_ in pipe._lane_graphs for lg in d_.values())
    with pytest.raises(ValueError):
        pipe.submit(im, tk, lc, pg, k, candidates=lists[0], items=ItemMap(torch.zeros(n, dtype=torch.int32)))
    assert pipe.submit(im, tk, lc, pg, k).place is None
    pipe.close()


# ---- CIRR driver -----------------------------------------------------------------------------------------------------------------------
def test_cirr_subset_ranks_from_candidate_places():
    """run/_common.recalls_cirr(subset="candidates") on the synthetic CIRR fixture: the 7-tuple of the default path (gathered member
    scores sorted on the host) on the fp32 gallery, the same tuple on the PreparedGallery and on the bf16 gallery.  The bf16 form ranks on
    bf16 scores: a subset rank may differ from the fp32 one only where two members' fp32 scores are a bf16 near-tie (closer than the
    bf16 score error bound 2^-8 * ||q|| * ||g|| <= 2^-8 on unit rows); any such pair is shown."""
    import json
    import os

    import synthetic_data as sdata
    from fashionern_aaai2024_amd import synth
    from fashionern_aaai2024_amd.model import ERN
    from fashionern_aaai2024_amd.run import _common, test_cirr
    from fashionern_aaai2024_amd.tokenizer import register_tokenizer
    from fashionern_aaai2024_amd.utils import extract_index_features
    meta = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "harness.json")))
    register_tokenizer("stub", sdata.stub_tokenizer)
    d, n, q = meta["d"], meta["n"], meta["q"]
    clip = sdata.StubCLIP(d).eval().to("cuda:0")
    model = ERN(clip, d, "cuda:0")
    model.load_state_dict(synth.fusion_state_dict(d, seed=meta["fusion_seed"]))
    gal = sdata.Gallery(n, d, seed=meta["gallery_seed"])
    rel = sdata.RelativeDataset(gal, q, "cirr", seed=meta["relative_seed"])
    feats, names, local = extract_index_features(sdata.ClassicDataset(gal), clip, 13, "cuda:0", d, num_workers=0)
    pred, refs, tgts, members = test_cirr.generate_cirr_val_predictions(clip, rel, model, names, feats, "cuda:0", d, meta["batch_size"], 0, "stub")
    pg = model.engine.prepare_gallery(_common.fuse_index(model, feats, local))
    default = _common.recalls_cirr(model, pred, pg.f32, names, refs, tgts, members)
    assert list(default) == meta["recalls"]["cirr"]
    assert _common.recalls_cirr(model, pred, pg.f32, names, refs, tgts, members, subset="gather") == default
    assert _common.recalls_cirr(model, pred, pg.f32, names, refs, tgts, members, subset="candidates") == default
    assert _common.recalls_cirr(model, pred, pg, names, refs, tgts, members, subset="candidates") == default
    with _common.cirr_subset("candidates"):
        assert _common.recalls_cirr(model, pred, pg, names, refs, tgts, members) == default
    got = _common.recalls_cirr(model, pred, pg.bf16, names, refs, tgts, members, subset="candidates")
    if got[:3] != default[:3]:      # show the member scores behind every differing subset rank
        row = {nm: i for i, nm in enumerate(names)}
        eng = model.engine
        lines = []
        for i in range(q):
            rows = [row[m] for m in members[i] if m in row and m != refs[i]]
            c = torch.tensor([rows], dtype=torch.int32)
            p32 = eng.sim_topk_candidates(pred[i:i + 1], pg.f32, c, len(rows), places=True)
            p16 = eng.sim_topk_candidates(pred[i:i + 1], pg.bf16, c, len(rows), places=True)
            j = rows.index(row[tgts[i]])
            if int(p32[2][0, j]) != int(p16[2][0, j]):
                lines.append(f"query {i}: fp32 place {int(p32[2][0, j])} scores {p32[0][0].tolist()} idx {p32[1][0].tolist()}; "
                             f"bf16 place {int(p16[2][0, j])} scores {p16[0][0].tolist()} idx {p16[1][0].tolist()}")
        raise AssertionError("bf16 subset ranks differ from fp32:\n" + "\n".join(lines))
    assert got == default

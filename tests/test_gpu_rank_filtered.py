"""Filtered ranking (include/fern.h: fern_sim_topk_filtered / fern_rank_count_filtered; `RowFilter`): every query ranks only the gallery
rows with (tags[n] & mask[b]) == value[b].

Oracle: oracle/chain.c scores on the CPU; ineligible, excluded and out-of-gallery entries set to -inf; a stable argsort (score descending,
index ascending) gives the order; places follow `places` of tests/support.py.  fp32 and prepared forms: scores and indices
bit-equal.  bf16 form: the ranking of the values `sweep_bf16_scores` returns, masked the same way.  Finite inputs only.

The shapes are the smallest at which each code path can go wrong (tiles select from 16 384 rows with a ragged last tile, the
row-walking dense select, a gallery smaller than K, the two-block sweep, one 64-query block per launch past 131 072 rows, the
1 024-query chunk, the register-heaviest and the generic sweep instantiation, the degenerate gallery)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import chain
from support import fresh_engine, int_unit, places, rand, same_bits, strategy_forms

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 50, 64, 65, 1000)
ONE = 0x80000000          # tag bit of the single row that filter kind 4 selects (the gallery's last row: the ragged last tile)


def _tags(n, interleaved):
    """uint32 [N]: bits 0-1 the category (three of them: contiguous segments, or n % 3), bits 2-30 the id of the row's group of six,
    bit 31 set on the last row only."""
    r = np.arange(n, dtype=np.int64)
    cat = r % 3 if interleaved else (r * 3) // max(n, 1)
    t = (cat | ((r // 6) << 2)).astype(np.uint32)
    if n:
        t[n - 1] |= np.uint32(ONE)
    return t


def _filters(b, n, shift=0):
    """uint32 (mask [B], value [B]): the kinds mixed over one batch, kind = (query + shift) % 6 --
    0 all-pass; 1 / 5 one category of three; 2 one group of six rows; 3 nothing (a value with bits outside its mask); 4 exactly one
    row, the gallery's last."""
    mask, value = np.zeros(b, dtype=np.uint32), np.zeros(b, dtype=np.uint32)
    groups = max(1, (n + 5) // 6)
    for q in range(b):
        kind = (q + shift) % 6
        if kind in (1, 5):
            mask[q], value[q] = 3, (q + kind) % 3
        elif kind == 2:
            mask[q], value[q] = 0x7FFFFFFC, ((7 * q + 1) % groups) << 2
        elif kind == 3:
            mask[q], value[q] = 1, 2
        elif kind == 4:
            mask[q], value[q] = ONE, ONE
    return mask, value


def _eligible(tags, mask, value):
    return (tags[None, :] & mask[:, None]) == value[:, None]


def _masked(scores, elig, idx_offset=0, exclude=None):
    s = np.where(elig, scores, -np.inf).astype(np.float32)
    if exclude is not None:
        for r, e in enumerate(exclude):
            if 0 <= e - idx_offset < s.shape[1]:
                s[r, e - idx_offset] = -np.inf
    return s


def _topk(masked, k, idx_offset=0):
    """(scores [B,k] f32, idx [B,k] int32) of masked scores: the first k places of the stable argsort (score descending, index
    ascending), taken per row from the rows at or above the k-th largest score; a place without an eligible row holds (-inf, -1)."""
    b, n = masked.shape
    sc = np.full((b, k), -np.inf, dtype=np.float32)
    idx = np.full((b, k), -1, dtype=np.int32)
    for r in range(b):
        row = masked[r]
        kk = min(k, n)
        if kk == 0:
            continue
        thr = np.partition(row, n - kk)[n - kk]
        cand = np.flatnonzero(row >= thr)                       # ascending index: a stable sort keeps ties in index order
        cand = cand[np.argsort(-row[cand], kind="stable")][:kk]
        sc[r, :kk] = row[cand]
        idx[r, :kk] = np.where(row[cand] == -np.inf, -1, cand + idx_offset)
    return sc, idx


def _row_filter(tags, mask, value, signed=False):
    from fashionern_aaai2024_amd.engine import RowFilter
    if signed:      # int32 tensors, taken as bits
        return RowFilter(torch.from_numpy(tags.view(np.int32)).cuda(), torch.from_numpy(mask.view(np.int32)).cuda(),
                         torch.from_numpy(value.view(np.int32)).cuda())
    return RowFilter(torch.from_numpy(tags).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(value).cuda())


@pytest.fixture(scope="module")
def eng():
    yield from fresh_engine()


def _call(eng, label, q, gal, k, **kw):
    """The public call a user of this form and depth makes."""
    if k > 64:
        return eng.sim_topk_deep(q, gal, k, **kw)
    return eng.sim_topk_bf16(q, gal, k, **kw) if label == "bf16" else eng.sim_topk(q, gal, k, **kw)


def _check_all_forms(eng, q, g, cases, ks=KS):
    """`cases`: [(name, tags, mask, value, idx_offset, exclude or None)].  Every form and depth against the masked oracle ranking."""
    exact = chain.chain_scores(q.numpy(), g.numpy())
    qd = q.cuda()
    bad, wants = [], {}
    try:
        for label, gal, strategy in strategy_forms(eng, g):
            if strategy:
                eng.set_rank_strategy(strategy)
            base = exact if label != "bf16" else eng.sweep_bf16_scores(qd, eng.prepare_gallery(g), tile_max=False).cpu().numpy()
            for name, tags, mask, value, off, ex in cases:
                if (label == "bf16", name) not in wants:       # one reference per case and score kind, shared by the forms
                    wants[(label == "bf16", name)] = _topk(_masked(base, _eligible(tags, mask, value), off, ex), max(ks), off)
                want = wants[(label == "bf16", name)]
                flt = _row_filter(tags, mask, value, signed=(off != 0))
                exd = None if ex is None else torch.from_numpy(ex)
                for k in ks:
                    got = _call(eng, label, qd, gal, k, idx_offset=off, exclude_idx=exd, row_filter=flt)
                    if not same_bits(got, (want[0][:, :k], want[1][:, :k])):
                        bad.append((label, name, k))
    finally:
        eng.set_rank_strategy("auto")
    assert not bad, bad


# (the nine smallest shapes of the code paths, and 65 x 1 000 x 512: the masked two-block sweep has no registers at D = 512 and runs two one-block passes)
SHAPES = [(8, 16_390, 64), (5, 3_000, 128), (64, 63, 128), (65, 1_000, 64), (65, 131_104, 64), (1_025, 1_000, 64), (3, 1_000, 640),
          (3, 1_000, 768), (1, 1, 64), (65, 1_000, 512)]


@pytest.mark.parametrize("B,N,D", SHAPES)
def test_mixed_filters_equal_the_masked_chain_ranking(eng, B, N, D):
    """Filters (a)-(e) mixed over the batch, tags once in contiguous segments and once interleaved, and (g) combined with exclude_idx
    and an idx_offset -- the excluded row is ineligible for some queries, eligible for others, the single eligible row for kind 4."""
    q, g = rand(B, D, seed=B + N), rand(N, D, seed=N + D, scale=D ** -0.5)
    off = 1_000
    cases = []
    for shift in range(0, 6 if B < 6 else 1, max(B, 1)):      # small batches: several passes, so that every kind is used
        m, v = _filters(B, N, shift)
        cases.append((f"segments/{shift}", _tags(N, False), m, v, 0, None))
        cases.append((f"interleaved/{shift}", _tags(N, True), m, v, 0, None))
        ex = np.array([off + (N - 1 if (r + shift) % 6 == 4 else (5 * r) % N) if r % 3 != 2 else -1 for r in range(B)], dtype=np.int32)
        cases.append((f"exclude+offset/{shift}", _tags(N, True), m, v, off, ex))
    # what the cases are about: the group filter leaves at most six rows (places 6.. unfilled at K = 50), kind 3 leaves none
    m, v = _filters(max(B, 6), N)
    el = _eligible(_tags(N, True), m, v).sum(axis=1)
    assert el[0] == N and el[2] <= 6 and el[3] == 0 and el[4] == min(N, 1)
    _check_all_forms(eng, q, g, cases)


@pytest.mark.parametrize("B,N,D", [(8, 16_390, 64), (65, 1_000, 64), (3, 1_000, 640), (1, 1, 64)])
def test_all_pass_filter_equals_the_unfiltered_call(eng, B, N, D):
    q, g = rand(B, D, seed=3 + N).cuda(), rand(N, D, seed=4 + N, scale=D ** -0.5)
    tags = _tags(N, True)
    zero = np.zeros(B, dtype=np.uint32)
    flt = _row_filter(tags, zero, zero)
    from fashionern_aaai2024_amd.engine import RowFilter
    scalar = RowFilter(torch.from_numpy(tags).cuda(), 0, 0)
    ex = torch.tensor([(3 * r) % N for r in range(B)], dtype=torch.int32)
    try:
        for label, gal, strategy in strategy_forms(eng, g):
            if strategy:
                eng.set_rank_strategy(strategy)
            for k in KS:
                for kw in ({}, {"idx_offset": 77, "exclude_idx": ex + 77}):
                    want = _call(eng, label, q, gal, k, **kw)
                    for f in (flt, scalar):
                        got = _call(eng, label, q, gal, k, row_filter=f, **kw)
                        assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (label, k)
    finally:
        eng.set_rank_strategy("auto")


@pytest.mark.parametrize("B,N,D", [(8, 16_390, 64), (5, 3_000, 128)])
def test_adversarial_gallery_whose_unfiltered_top_is_all_ineligible(eng, B, N, D):
    """(f) every ineligible row gets a component along the queries' directions, so the unfiltered top-K of every query consists of
    ineligible rows only; the filtered result is still the chain's ranking of the eligible ones."""
    q, g = rand(B, D, seed=11), rand(N, D, seed=12, scale=D ** -0.5)
    tags = _tags(N, True)
    mask, value = np.full(B, 3, dtype=np.uint32), np.zeros(B, dtype=np.uint32)      # category 0 of the interleaved three
    elig = _eligible(tags, mask, value)
    push = (q / q.norm(dim=1, keepdim=True)).sum(dim=0)
    g = g + torch.from_numpy(~elig[0]).float()[:, None] * 4.0 * push[None, :]
    kmax = 1000
    s = chain.chain_scores(q.numpy(), g.numpy())
    top = np.argsort(-s, axis=1, kind="stable")[:, :kmax]
    assert not np.take_along_axis(elig, top, axis=1).any()          # the unfiltered top-K is entirely ineligible ...
    assert (elig.sum(axis=1) >= kmax).all()                         # ... and K eligible rows exist
    _check_all_forms(eng, q, g, [("adversarial", tags, mask, value, 0, None)], ks=(50, 64, kmax))


@pytest.mark.parametrize("B,N,D", [(8, 16_390, 64), (5, 3_000, 128)])
def test_tie_heavy_galleries_run_the_fallbacks_filtered(eng, B, N, D):
    """Scores in multiples of 1/64 with thousands of ties: the select kernels have no room and the exact fallbacks rank -- filtered."""
    q, g = int_unit(B, D, seed=41), int_unit(N, D, seed=42)
    cat = (np.full(B, 3, dtype=np.uint32), (np.arange(B) % 3).astype(np.uint32))
    groups = (N + 5) // 6
    grp = (np.full(B, 0x7FFFFFFC, dtype=np.uint32), (((11 * np.arange(B) + 2) % groups) << 2).astype(np.uint32))
    cases = [("categories/segments", _tags(N, False), *cat, 0, None), ("categories/interleaved", _tags(N, True), *cat, 0, None),
             ("groups", _tags(N, True), *grp, 0, None)]
    _check_all_forms(eng, q, g, cases, ks=(50, 1000))


_CAP_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, torch
import test_gpu_rank_filtered as t
from fashionern_aaai2024_amd.engine import FernEngine
eng = FernEngine("cuda:0")
B, N, D = 5, 3000, 128
q, g = t.rand(B, D, seed=1), t.rand(N, D, seed=2, scale=D ** -0.5)
m, v = t._filters(B, N, 1)
t._check_all_forms(eng, q, g, [("interleaved", t._tags(N, True), m, v, 0, None), ("segments", t._tags(N, False), m, v, 0, None)], ks=(50, 65, 1000))
print("ok")
"""


def test_forced_deep_fallback_in_a_child_process():
    """FERN_RANK_DEEP_CAP=1: every query overflows the deep select kernel's capacity and is ranked by the gated exact fallback (after the
    gated, masked rewrite of its row in the prepared form)."""
    env = dict(os.environ, FERN_RANK_DEEP_CAP="1")
    r = subprocess.run([sys.executable, "-c", _CAP_CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


# ---- rank_of -----------------------------------------------------------------------------------------------------------------------
def _rank_targets(b, n, m, seed, place, elig):
    """[B,m] targets spread over the whole depth of the masked ranking, plus ineligible rows, -1 and an index past the gallery."""
    rng = np.random.default_rng(seed)
    order = np.argsort(place, axis=1)
    t = rng.integers(0, n, size=(b, m)).astype(np.int64)
    for r in range(b):
        ne = int(elig[r].sum())
        if ne:
            depth = np.linspace(0, ne - 1, m).astype(np.int64)
            t[r] = np.where(rng.random(m) < 0.7, order[r, depth], t[r])
        if r % 4 == 1:
            t[r, rng.integers(m)] = -1
        if r % 4 == 2:
            t[r, rng.integers(m)] = n + 3
    return t.astype(np.int32)


def _expected_ranks(place, t, elig):
    n = place.shape[1]
    ok = (t >= 0) & (t < n)
    safe = np.where(ok, t, 0)
    ok &= np.take_along_axis(elig, safe, axis=1)
    return np.where(ok, np.take_along_axis(place, safe, axis=1), -1).astype(np.int32)


@pytest.mark.parametrize("B,N,D", [(8, 16_390, 64), (65, 1_000, 64), (5, 3_000, 128)])
def test_rank_of_is_the_place_in_the_masked_ranking(eng, B, N, D):
    q, g = rand(B, D, seed=31 + N), rand(N, D, seed=32 + N, scale=D ** -0.5)
    pg = eng.prepare_gallery(g)
    tags = _tags(N, True)
    mask, value = _filters(B, N, 1)
    elig = _eligible(tags, mask, value)
    flt = _row_filter(tags, mask, value)
    exact = chain.chain_scores(q.numpy(), g.numpy())
    approx = eng.sweep_bf16_scores(q.cuda(), pg, tile_max=False).cpu().numpy()
    for label, gal, base in (("fp32", g.cuda(), exact), ("prepared", pg, exact), ("bf16", pg.bf16, approx)):
        place = places(_masked(base, elig))
        for m in (1, 8, 13):
            t = _rank_targets(B, N, m, seed=m, place=place, elig=elig)
            got = eng.rank_of(q.cuda(), gal, torch.from_numpy(t), row_filter=flt)
            want = _expected_ranks(place, t, elig)
            assert (want == -1).any() and (want >= 0).any()
            assert np.array_equal(got.cpu().numpy(), want), (label, m)
        flat = _rank_targets(B, N, 1, seed=5, place=place, elig=elig)
        assert np.array_equal(eng.rank_of(q.cuda(), gal, torch.from_numpy(flat[:, 0]), row_filter=flt).cpu().numpy(),
                              _expected_ranks(place, flat, elig)[:, 0])


@pytest.mark.parametrize("form", ["fp32", "bf16"])
def test_filtered_counts_of_two_shards_add_up(eng, form):
    from fashionern_aaai2024_amd.engine import RowFilter
    B, N, D, m = 8, 16_390, 64, 5
    q, g = rand(B, D, seed=51).cuda(), rand(N, D, seed=52, scale=D ** -0.5)
    gal = g.cuda() if form == "fp32" else eng.gallery_to_bf16(g)
    tags = torch.from_numpy(_tags(N, True).view(np.int32)).cuda()          # int32 bits: torch indexes and slices them on the device
    mask, value = (torch.from_numpy(a.view(np.int32)).cuda() for a in _filters(B, N, 1))
    t = torch.from_numpy(np.random.default_rng(9).integers(0, N, size=(B, m)).astype(np.int32))
    ex = torch.tensor([(13 * r) % N for r in range(B)], dtype=torch.int32)
    whole = eng.rank_of(q, gal, t, exclude_idx=ex, row_filter=RowFilter(tags, mask, value))
    keys = eng.rank_keys(q, gal, t)
    ok = ((tags[t.cuda().long()] & mask[:, None]) == value[:, None]) & (t.cuda() != ex.cuda()[:, None])
    keys = torch.where(ok, keys, torch.zeros_like(keys))
    cut = 7_001
    counts = sum(eng.rank_count(q, gal[a:b].contiguous(), keys, idx_offset=a, exclude_idx=ex, row_filter=RowFilter(tags[a:b], mask, value)).clamp(min=0)
                 for a, b in ((0, cut), (cut, N)))
    counts = torch.where(keys == 0, torch.full_like(counts, -1), counts)
    assert torch.equal(counts, whole)
    assert (whole >= 0).any() and (whole == -1).any()


# ---- merged gallery against per-category galleries ---------------------------------------------------------------------------------
def test_merged_filtered_gallery_equals_the_three_category_galleries():
    import synthetic_data as sdata
    from fashionern_aaai2024_amd import synth
    from fashionern_aaai2024_amd.engine import RowFilter
    from fashionern_aaai2024_amd.model import ERN
    from fashionern_aaai2024_amd.run import _common, test_fiq
    from fashionern_aaai2024_amd.tokenizer import register_tokenizer
    from fashionern_aaai2024_amd.utils import extract_index_features
    register_tokenizer("stub", sdata.stub_tokenizer)
    dev, d = "cuda:0", 128
    clip = sdata.StubCLIP(d).eval().to(dev)
    model = ERN(clip, d, dev)
    model.load_state_dict(synth.fusion_state_dict(d, seed=11))
    feats, locals_, names, preds, targets, per_recalls, per_top = [], [], [], [], [], [], []
    for c, n in enumerate((700, 900, 1_100)):
        gal = sdata.Gallery(n, d, seed=20 + c)
        rel = sdata.RelativeDataset(gal, 40, "fiq", seed=30 + c)
        f, nm, lc = extract_index_features(sdata.ClassicDataset(gal), clip, 13, dev, d, num_workers=0)
        p, t = test_fiq.generate_fiq_val_predictions(clip, rel, model, nm, f, dev, d, 16, 0, "stub")
        fused = _common.fuse_index(model, f, lc, prepared=True)
        per_recalls.append(_common.recalls_unique(model, p, fused, nm, t, (10, 50)))
        per_top.append(_common._ranked(model, p, fused, 50))
        feats.append(f); locals_.append(lc); names.append(nm); preds.append(p); targets.append(t)
    all_f, all_l, tags, starts = _common.merge_galleries(feats, locals_)
    assert list(starts) == [0, 700, 1_600, 2_700] and names[0][0] == names[1][0]      # names repeat across the categories
    merged = _common.fuse_index(model, all_f, all_l, prepared=True)
    assert _common.recalls_merged(model, preds, merged, tags, starts, names, targets, (10, 50)) == per_recalls
    value = torch.cat([torch.full((p.shape[0],), c, dtype=torch.int32) for c, p in enumerate(preds)])
    top = _common._ranked(model, torch.cat(preds), merged, 50, row_filter=RowFilter(tags.to(dev), -1, value.to(dev)))
    o = 0
    for c, p in enumerate(preds):
        assert np.array_equal(top[o:o + p.shape[0]] - starts[c], per_top[c]), c
        o += p.shape[0]


# ---- pipeline ----------------------------------------------------------------------------------------------------------------------
def test_pipeline_submit_with_a_row_filter_eager_and_replayed():
    from fashionern_aaai2024_amd import synth
    from fashionern_aaai2024_amd.clip_model import create_model
    from fashionern_aaai2024_amd.engine import RowFilter
    from fashionern_aaai2024_amd.model import ERN
    from fashionern_aaai2024_amd.pipeline import ComposedQueryPipeline
    cfg = synth.CLIP_CONFIGS["tiny"]
    d = cfg.embed_dim
    clip = create_model(cfg, device="cuda:0", seed=3)
    model = ERN(clip, d, "cuda:0", engine=clip.engine).init_random(4)
    e = model.engine
    n = 5_000
    gal = e.prepare_gallery(e.index_fuse(torch.from_numpy(synth.global_feats(n, d, tag="fg")), torch.from_numpy(synth.local_feats(n, d, tag="fgl")), True))
    tags = torch.from_numpy(_tags(n, True)).cuda()
    batches = []
    for j in range(3):                                      # a different mask / value batch per job
        m, v = _filters(9, n, j)
        batches.append((torch.from_numpy(synth.images(9, cfg, 300 + j)).cuda(), torch.from_numpy(synth.captions(9, cfg, 300 + j)).cuda(),
                        torch.from_numpy(synth.local_feats(9, d, 300 + j)).cuda(), RowFilter(tags, torch.from_numpy(m).cuda(), torch.from_numpy(v).cuda())))
    direct = []
    for im, tk, lc, flt in batches:
        fq = e.dvr_fuse(e.encode_image(im), lc, *e.encode_text(tk))
        direct.append(e.sim_topk(fq, gal, 50, row_filter=flt))
    assert not torch.equal(direct[0][1], direct[1][1])
    pipe = ComposedQueryPipeline(e, lanes=1, graphs=True)
    for _ in range(2):                                      # one lane, one key: eager twice, captured, then replayed with other filters
        futures = [pipe.submit(im, tk, lc, gal, 50, row_filter=flt) for im, tk, lc, flt in batches]
        for (ds, di), fut in zip(direct, futures):
            s, i = fut.wait()
            torch.cuda.current_stream().synchronize()
            assert torch.equal(i, di) and torch.equal(s, ds)
    assert all(lg.graph is not None for d_ in pipe._lane_graphs for lg in d_.values())
    pipe.close()

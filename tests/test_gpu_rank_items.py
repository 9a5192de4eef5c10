"""Item-level ranking (include/fern.h: fern_sim_topk_items, fern_item_rank; FernEngine.sim_topk_items / item_rank_of): the exact row
ranking with every row but the first of its item removed, on every gallery form -- fp32 and PreparedGallery (exact fp32-chain scores) and
bf16 (the bf16 similarity) -- plus the graph / pipeline plumbing above it.

Oracle: tests/items_oracle.py on oracle/chain.c scores (bf16 form: on the values `sweep_bf16_scores` returns).  Every comparison is bit
for bit: uint32 views of the scores, array_equal on indices, items and ranks."""
import functools

import numpy as np
import pytest
import torch

import items_oracle as io
from oracle import chain
from support import fresh_engine, gallery, int_unit, rand, same_bits

pytestmark = pytest.mark.gpu


def _runs(sizes, n_items, seed):
    """Contiguous runs of the given sizes; run r carries id perm[r] (ids play no part in the order, so they are shuffled)."""
    perm = np.random.default_rng(seed).permutation(n_items)
    assert len(sizes) == n_items
    return np.repeat(perm, sizes).astype(np.int32)


def _uneven_37():
    """1 000 rows, 37 items: ten singletons, a run that ends at row 59, one across row 64, one of 400 rows across 256, then 24 more."""
    sizes = [1] * 10 + [50, 10, 400] + [22] * 23 + [24]
    assert sum(sizes) == 1000
    return _runs(sizes, 37, seed=5)


def _even(n, g, seed):
    sizes = [n // g + (1 if r < n % g else 0) for r in range(g)]
    return _runs(sizes, g, seed)


# (B, N, D, K, G, layout, forms)
SHAPES = {
    "single": (1, 1, 128, 1, 1, lambda: np.zeros(1, np.int32), ("fp32", "prepared", "bf16")),
    "uneven": (3, 1000, 128, 64, 37, _uneven_37, ("fp32", "prepared", "bf16")),
    "identity": (65, 1000, 512, 65, 1000, lambda: np.arange(1000, dtype=np.int32), ("fp32", "prepared", "bf16")),
    "interleaved": (64, 5003, 512, 1024, 300, lambda: (np.arange(5003) % 300).astype(np.int32), ("fp32", "prepared", "bf16")),
    "chunked": (1025, 1000, 640, 10, 50, lambda: _even(1000, 50, 7), ("fp32",)),
    "large": (2, 46_001, 768, 1000, 9000, lambda: _even(46_001, 9000, 9), ("fp32", "bf16")),
}
CASES = [(name, form) for name, sh in SHAPES.items() for form in sh[6]]


@pytest.fixture(scope="module")
def eng():
    yield from fresh_engine()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(q, g, items, chain scores) of a shape: computed once, shared, never written to."""
    B, N, D, K, G, layout, _ = SHAPES[name]
    q, g = rand(B, D, seed=B + N), rand(N, D, seed=N + D, scale=D ** -0.5)
    s = chain.chain_scores(q.numpy(), g.numpy())
    s.setflags(write=False)
    return q, g, layout(), s


_bf16_scores = {}


def _scores(eng, name, form):
    """The [B, N] score matrix the form ranks on: the chain's, or the bf16 sweep's own values."""
    q, g, items, s = _case(name)
    if form != "bf16":
        return s
    if name not in _bf16_scores:
        _bf16_scores[name] = eng.sweep_bf16_scores(q.cuda(), eng.prepare_gallery(g.cuda()), tile_max=False).cpu().numpy()
    return _bf16_scores[name]


def _item_map(items, n_items):
    from fashionern_aaai2024_amd.engine import ItemMap
    return ItemMap(torch.from_numpy(np.asarray(items, dtype=np.int32)).cuda(), n_items)


@pytest.mark.parametrize("name,form", CASES)
def test_topk_items_equals_the_oracle(eng, name, form):
    B, N, D, K, G, _, _ = SHAPES[name]
    q, g, items, _ = _case(name)
    got = eng.sim_topk_items(q.cuda(), gallery(eng, g, form), _item_map(items, G), K)
    want = io.item_topk(io.masked_scores(_scores(eng, name, form)), items, G, K)
    assert same_bits(got, want)
    if name == "identity":                                   # every row its own item: the row ranking itself
        s, i = eng.sim_topk_deep(q.cuda(), gallery(eng, g, form), K)
        assert torch.equal(got[1], i) and torch.equal(got[0].view(torch.int32), s.view(torch.int32)) and torch.equal(got[2], i)


@pytest.mark.parametrize("name,form", [c for c in CASES if SHAPES[c[0]][1] <= 1024 and c[0] != "chunked"])
def test_small_galleries_equal_the_deduplicated_deep_list(eng, name, form):
    B, N, D, K, G, _, _ = SHAPES[name]
    q, g, items, _ = _case(name)
    gal = gallery(eng, g, form)
    s, i = (x.cpu().numpy() for x in eng.sim_topk_deep(q.cuda(), gal, N))
    ws = np.full((B, K), -np.inf, dtype=np.float32)
    wi = np.full((B, K), -1, dtype=np.int32)
    wt = np.full((B, K), -1, dtype=np.int32)
    for b in range(B):
        seen, o = set(), 0
        for sc, r in zip(s[b], i[b]):
            if r >= 0 and items[r] not in seen and o < K:
                seen.add(items[r])
                ws[b, o], wi[b, o], wt[b, o] = sc, r, items[r]
                o += 1
    assert same_bits(eng.sim_topk_items(q.cuda(), gal, _item_map(items, G), K), (ws, wi, wt))


# ---- contract cases at (3, 1 000, 128) -------------------------------------------------------------------------------------------
def test_k_beyond_the_items_is_padded(eng):
    q, g, items, s = _case("uneven")
    got = eng.sim_topk_items(q.cuda(), g.cuda(), _item_map(items, 37), 100)
    assert same_bits(got, io.item_topk(io.masked_scores(s), items, 37, 100))
    s_, i_, t_ = (x.cpu().numpy() for x in got)
    assert (i_[:, 37:] == -1).all() and (t_[:, 37:] == -1).all() and np.isneginf(s_[:, 37:]).all() and (i_[:, :37] >= 0).all()


def test_idx_offset_and_exclusions_move_the_representative(eng):
    q, g, items, s = _case("uneven")
    off = 7000
    plain = io.item_topk(io.masked_scores(s), items, 37, 37)
    big = int(items[100])                                    # the 400-row item
    best_of_big = [int(plain[1][b][list(plain[2][b]).index(big)]) for b in range(3)]
    single = int(items[3])                                   # a singleton item: row 3 is its only row
    ex = np.array([best_of_big[0] + off, 3 + off, -1], dtype=np.int32)
    got = eng.sim_topk_items(q.cuda(), g.cuda(), _item_map(items, 37), 37, idx_offset=off, exclude_idx=torch.from_numpy(ex))
    want = io.item_topk(io.masked_scores(s, off, ex), items, 37, 37, off)
    assert same_bits(got, want)
    i_, t_ = got[1].cpu().numpy(), got[2].cpu().numpy()
    rep0 = int(i_[0][list(t_[0]).index(big)]) - off
    assert rep0 != best_of_big[0] and items[rep0] == big     # represented by its next row
    assert single not in t_[1] and (t_[1] >= 0).sum() == 36 and single in t_[0]      # the singleton disappears for query 1 only
    assert np.array_equal(i_[2], plain[1][2] + off)


def _filter_case(items):
    from fashionern_aaai2024_amd.engine import RowFilter
    n = len(items)
    tags = ((items.astype(np.int64) % 2) | ((np.arange(n) % 2) << 1)).astype(np.int32)      # bit 0: item parity, bit 1: row parity
    mask = np.array([1, 2, 0], dtype=np.int32)               # query 0: whole (odd) items removed; query 1: half of every item's rows; query 2: all
    value = np.array([0, 2, 0], dtype=np.int32)
    elig = (tags[None, :] & mask[:, None]) == value[:, None]
    return RowFilter(torch.from_numpy(tags).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(value).cuda()), elig


@pytest.mark.parametrize("form", ["fp32", "bf16"])
def test_row_filter_removes_items_and_rows(eng, form):
    q, g, items, _ = _case("uneven")
    s = _scores(eng, "uneven", form)
    flt, elig = _filter_case(items)
    got = eng.sim_topk_items(q.cuda(), gallery(eng, g, form), _item_map(items, 37), 37, row_filter=flt)
    assert same_bits(got, io.item_topk(io.masked_scores(s, eligible=elig), items, 37, 37))
    t_ = got[2].cpu().numpy()
    assert (t_[0][t_[0] >= 0] % 2 == 0).all() and (t_[0] >= 0).sum() < 37
    assert (got[1].cpu().numpy()[1][t_[1] >= 0] % 2 == 1).all()      # odd rows only: singletons on even rows are gone too
    # mask = value = 0 is the unfiltered call
    from fashionern_aaai2024_amd.engine import RowFilter
    open_ = RowFilter(flt.tags, 0, 0)
    a = eng.sim_topk_items(q.cuda(), gallery(eng, g, form), _item_map(items, 37), 37, row_filter=open_)
    b = eng.sim_topk_items(q.cuda(), gallery(eng, g, form), _item_map(items, 37), 37)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_ids_outside_the_range_are_ignored(eng):
    q, g, items, s = _case("uneven")
    ids = items.copy()
    ids[::7] = -1
    ids[5::11] = 37
    ids[500:520] = 1 << 30
    got = eng.sim_topk_items(q.cuda(), g.cuda(), _item_map(ids, 37), 64)
    assert same_bits(got, io.item_topk(io.masked_scores(s), ids, 37, 64))
    i_ = got[1].cpu().numpy()
    assert not np.isin(i_[i_ >= 0] % 7, [0]).any()
    ranks = eng.item_rank_of(q.cuda(), g.cuda(), _item_map(ids, 37), torch.tensor([[-1, 37, 1 << 30, int(items[100])]] * 3, dtype=torch.int32))
    assert (ranks[:, :3].cpu().numpy() == -1).all() and (ranks[:, 3].cpu().numpy() >= 0).all()


@pytest.mark.parametrize("layout", ["interleaved", "contiguous"])
def test_all_ties_are_broken_by_row_index(eng, layout):
    N, D = 1000, 128
    g = int_unit(1, D, seed=3).repeat(N, 1)
    q = int_unit(3, D, seed=4)
    items = (np.arange(N) % 10 if layout == "interleaved" else np.arange(N) // 100).astype(np.int32)
    s, i, t = (x.cpu().numpy() for x in eng.sim_topk_items(q.cuda(), g.cuda(), _item_map(items, 10), 10))
    first = np.arange(10) if layout == "interleaved" else np.arange(10) * 100
    assert np.array_equal(i, np.tile(first, (3, 1))) and np.array_equal(t, items[i])
    assert np.array_equal(s.view(np.uint32), chain.chain_scores(q.numpy(), g[:1].numpy()).repeat(10, axis=1).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _flood():
    """30 000 copies of the best-scoring row, spread over 5 000 items (six rows each, interleaved), then 4 001 ordinary items: after the
    reduction 5 000 representatives tie at the top -- more than the select kernel collects -- so the radix fallback ranks them."""
    B, N, D = 2, 46_001, 768
    q, g = int_unit(B, D, seed=31), int_unit(N, D, seed=32)
    g[:30_000] = (q[0] + q[1]).sign() / 8.0
    items = np.concatenate([np.arange(30_000) % 5000, 5000 + (np.arange(N - 30_000) // 4)]).astype(np.int32)
    s = chain.chain_scores(q.numpy(), g.numpy())
    assert (s[:, :30_000].max(axis=1) > s[:, 30_000:].max(axis=1)).all()
    return q, g, items, s


@pytest.mark.parametrize("form", ["fp32", "bf16"])
def test_tie_flood_reaches_the_fallback(eng, form):
    q, g, items, s = _flood()
    G, K = 5000 + 4001, 1000
    if form == "bf16":                                       # operands in {-1, 0, 1} / 8 are exact in bf16: the sweep's values still tie
        s = eng.sweep_bf16_scores(q.cuda(), eng.prepare_gallery(g.cuda()), tile_max=False).cpu().numpy()
    got = eng.sim_topk_items(q.cuda(), gallery(eng, g, form), _item_map(items, G), K)
    assert same_bits(got, io.item_topk(io.masked_scores(s), items, G, K))
    assert np.array_equal(got[1].cpu().numpy(), np.tile(np.arange(K), (2, 1)))
    ranks = eng.item_rank_of(q.cuda(), gallery(eng, g, form), _item_map(items, G), torch.tensor([[4999, 0, 5000]] * 2, dtype=torch.int32))
    assert np.array_equal(ranks.cpu().numpy(), io.item_ranks(io.masked_scores(s), items, G, [[4999, 0, 5000]] * 2))
    assert ranks[0, 0] == 4999 and ranks[0, 1] == 0


# ---- ranks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("uneven", "fp32"), ("uneven", "bf16"), ("interleaved", "fp32"), ("interleaved", "prepared"), ("interleaved", "bf16")])
def test_item_rank_is_the_place_in_the_full_item_list(eng, name, form):
    B, N, D, K, G, _, _ = SHAPES[name]
    q, g, items, _ = _case(name)
    gal, im = gallery(eng, g, form), _item_map(items, G)
    _, _, t = eng.sim_topk_items(q.cuda(), gal, im, G)
    targets = torch.arange(G, dtype=torch.int32).repeat(B, 1)
    ranks = eng.item_rank_of(q.cuda(), gal, im, targets).cpu().numpy()
    t = t.cpu().numpy()
    assert (t >= 0).all()
    assert np.array_equal(np.take_along_axis(ranks, t.astype(np.int64), axis=1), np.tile(np.arange(G, dtype=np.int32), (B, 1)))


@pytest.mark.parametrize("m", [1, 5])
def test_item_rank_equals_the_oracle(eng, m):
    B, N, D, K, G, _, _ = SHAPES["interleaved"]
    q, g, items, s = _case("interleaved")
    t = np.random.default_rng(m).integers(-2, G + 2, size=(B, m)).astype(np.int32)
    t[0, 0], t[1, 0] = -1, G                                  # ids outside [0, G), whatever the draw
    off = 300
    ex = np.array([off + (13 * r) % N if r % 2 else -1 for r in range(B)], dtype=np.int32)
    want = io.item_ranks(io.masked_scores(s, off, ex), items, G, t)
    got = eng.item_rank_of(q.cuda(), g.cuda(), _item_map(items, G), torch.from_numpy(t), idx_offset=off, exclude_idx=torch.from_numpy(ex))
    assert np.array_equal(got.cpu().numpy(), want) and (want >= 0).any() and (want == -1).any()
    flat = eng.item_rank_of(q.cuda(), g.cuda(), _item_map(items, G), torch.from_numpy(t[:, 0].copy()), idx_offset=off, exclude_idx=torch.from_numpy(ex))
    assert flat.shape == (B,) and np.array_equal(flat.cpu().numpy(), want[:, 0])


def test_empty_and_filtered_out_target_items_have_no_rank(eng):
    q, g, items, s = _case("uneven")
    flt, elig = _filter_case(items)
    t = np.tile(np.arange(40, dtype=np.int32), (3, 1))       # ids 37 .. 39 are out of range
    im = _item_map(items, 37)
    got = eng.item_rank_of(q.cuda(), g.cuda(), im, torch.from_numpy(t), row_filter=flt).cpu().numpy()
    assert np.array_equal(got, io.item_ranks(io.masked_scores(s, eligible=elig), items, 37, t))
    assert (got[0, 1:37:2] == -1).all() and (got[0, 0:37:2] >= 0).all() and (got[:, 37:] == -1).all()
    wide = _item_map(items, 45)                              # items 37 .. 44 exist but own no row
    got = eng.item_rank_of(q.cuda(), g.cuda(), wide, torch.tensor([[40, 44, 45]] * 3, dtype=torch.int32)).cpu().numpy()
    assert (got == -1).all()


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_on_new_queries_and_exclusions(eng):
    B, N, D, K, G, _, _ = SHAPES["interleaved"]
    _, g, items, _ = _case("interleaved")
    g, im = g.cuda(), _item_map(items, G)
    q = rand(B, D, seed=61).cuda()
    ex = torch.tensor([(3 * r) % N for r in range(B)], dtype=torch.int32).cuda()
    eng.sim_topk_items(q, g, im, K, exclude_idx=ex)          # one eager call: the workspace exists
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = eng.sim_topk_items(q, g, im, K, exclude_idx=ex)
    for seed in (63, 64):
        q.copy_(rand(B, D, seed=seed))
        ex.copy_(torch.tensor([(seed * r + 1) % N for r in range(B)], dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        # a table that was not zeroed inside the graph would keep the previous replay's representatives
        want = eng.sim_topk_items(q, g, im, K, exclude_idx=ex)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, want))
        s = chain.chain_scores(q.cpu().numpy(), g.cpu().numpy())
        assert same_bits(out, io.item_topk(io.masked_scores(s, 0, ex.cpu().numpy()), items, G, K))


def test_pipeline_submit_with_items_eager_and_replayed():
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
    n = 5_000
    gal = e.prepare_gallery(e.index_fuse(torch.from_numpy(synth.global_feats(n, d, tag="fg")), torch.from_numpy(synth.local_feats(n, d, tag="fgl")), True))
    items = ItemMap((torch.arange(n, dtype=torch.int32) // 3).cuda())
    assert items.n_items == 1667
    batches = [(torch.from_numpy(synth.images(9, cfg, 300 + j)).cuda(), torch.from_numpy(synth.captions(9, cfg, 300 + j)).cuda(),
                torch.from_numpy(synth.local_feats(9, d, 300 + j)).cuda()) for j in range(3)]
    direct = []
    for im, tk, lc in batches:
        fq = e.dvr_fuse(e.encode_image(im), lc, *e.encode_text(tk))
        direct.append(e.sim_topk_items(fq, gal, items, 50))
    assert not torch.equal(direct[0][1], direct[1][1])
    pipe = ComposedQueryPipeline(e, lanes=1, graphs=True)
    assert pipe.submit(*batches[0], gal, 50).item is None    # a row-level job carries no items
    for _ in range(2):                                      # one lane, one key: eager twice, captured, then replayed
        futures = [pipe.submit(im, tk, lc, gal, 50, items=items) for im, tk, lc in batches]
        for (ds, di, dt), fut in zip(direct, futures):
            s, i = fut.wait()
            torch.cuda.current_stream().synchronize()
            assert torch.equal(i, di) and torch.equal(s, ds) and torch.equal(fut.item, dt)
            assert torch.equal(fut.item, torch.where(i >= 0, i // 3, torch.full_like(i, -1)))
    assert all(lg.graph is not None for d_ in pipe._lane_graphs for lg in d_.values() if lg.calls > 2)
    pipe.close()


def test_argument_errors_are_refused_with_a_message(eng):
    from fashionern_aaai2024_amd._lib import FernError
    lib, h = eng.lib, eng._h
    p = 0x1000                                               # never dereferenced: every call below is refused before any HIP call
    topk = lambda k, g, items=p, g32=p, g16=None, d=128: lib.fern_sim_topk_items(h, p, g32, g16, 2, 10, d, k, items, g, p, p, p, 0, None, None, None, None, None)      # noqa: E731
    for k in (0, 1025):
        assert topk(k, 5) == -1 and b"fern_sim_topk_items: need 1<=K<=1024" in lib.fern_last_error()
    assert topk(5, 0) == -1 and b"fern_sim_topk_items: need G >= 1" in lib.fern_last_error()
    assert topk(5, 5, items=None) == -1 and b"fern_sim_topk_items: items is NULL" in lib.fern_last_error()
    assert topk(5, 5, g32=None, g16=p, d=640 + 32) == -1 and b"a bf16-only gallery needs D % 64 == 0, D <= 768" in lib.fern_last_error()
    rank = lambda g, items=p, m=1: lib.fern_item_rank(h, p, p, None, 2, 10, 128, items, g, p, m, 0, None, p, None, None, None, None)      # noqa: E731
    assert rank(0) == -1 and b"fern_item_rank: need G >= 1" in lib.fern_last_error()
    assert rank(5, items=None) == -1 and b"fern_item_rank: items is NULL" in lib.fern_last_error()
    assert rank(5, m=0) == -1 and b"fern_item_rank: need m >= 1" in lib.fern_last_error()
    q, g = rand(2, 128, seed=1).cuda(), rand(10, 128, seed=2).cuda()
    with pytest.raises(FernError, match="fern_sim_topk_items"):
        eng.sim_topk_items(q, g, _item_map(np.zeros(10, np.int32), 1), 1025)
    with pytest.raises(ValueError, match="gallery has 10 rows"):
        eng.sim_topk_items(q, g, _item_map(np.zeros(9, np.int32), 1), 5)
    with pytest.raises(FernError, match="workspace budget"):      # one query's table alone is past the budget
        eng.item_rank_of(q, g, _item_map(np.zeros(10, np.int32), 200_000_000), torch.zeros(2, dtype=torch.int32))

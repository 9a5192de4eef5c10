"""Ranking pages (include/fern.h: fern_rank_select / fern_sim_topk_from / fern_sim_topk_page; FernEngine.rank_select / sim_topk_from /
rank_page): the rows at places [offset, offset + K) of a query's ranking at any depth, the key at a place, and result lists continued from
a cursor, on every gallery form.

Oracle: oracle/chain.c scores ranked by a stable argsort (score descending, gallery index ascending), with the rows that take no place
(the excluded row, ineligible rows) removed.  Finite inputs only.  Every comparison is array_equal on indices and on score BITS."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import chain
from rank_oracle import make_keys
from support import assert_same_bits, int_unit, rand

pytestmark = pytest.mark.gpu

ALL = -1                     # the cursor ~0 as int64 bits: everything is eligible


def _rankings(scores, idx_offset=0, exclude=None, eligible=None):
    """Per query (scores, global indices) of its whole ranking: stable argsort of `scores` [B,N], then the excluded row (global index)
    and the ineligible rows (`eligible` bool [B,N]) removed."""
    out = []
    order = np.argsort(-scores, axis=1, kind="stable")
    for b in range(scores.shape[0]):
        o = order[b]
        keep = np.ones(len(o), dtype=bool)
        if eligible is not None:
            keep &= eligible[b, o]
        if exclude is not None:
            keep &= (o + idx_offset) != exclude[b]
        o = o[keep]
        out.append((scores[b, o].astype(np.float32), (o + idx_offset).astype(np.int32)))
    return out


def _slice(rankings, offsets, k):
    """The expected (scores, idx) [B,k] of places [offsets[b], offsets[b] + k): -inf / -1 past the end, a negative offset counts as 0."""
    b = len(rankings)
    s = np.full((b, k), -np.inf, dtype=np.float32)
    i = np.full((b, k), -1, dtype=np.int32)
    for r, (rs, ri) in enumerate(rankings):
        lo = max(int(offsets[r]), 0)
        part = slice(lo, lo + k)
        s[r, :len(rs[part])] = rs[part]
        i[r, :len(ri[part])] = ri[part]
    return s, i


def _same(got, want):
    """(scores, idx) of a call, tensors or arrays, against the oracle's arrays: float32 / int32, bit for bit."""
    assert want[0].dtype == np.float32 and want[1].dtype == np.int32
    assert_same_bits(tuple(got[:2]), tuple(want[:2]))


def _keys_at(rankings, places):
    """uint64 [B,m]: the ranking key of the row at each place; 0 for a place < 0 or past the end."""
    out = np.zeros(places.shape, dtype=np.uint64)
    for r, (rs, ri) in enumerate(rankings):
        for j, p in enumerate(places[r]):
            if 0 <= p < len(ri):
                out[r, j] = make_keys(rs[p:p + 1], ri[p:p + 1])[0]
    return out


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _offsets(n, k):
    return [0, 1, 63, 64, 1000, 1023, 1024, n - k - 1, n - 1, n, n + 5]


@pytest.fixture(scope="module")
def eng(engine):
    return engine


# ---- pages against oracle slices -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D", [(5, 3000, 128), (3, 1001, 64), (2, 1, 128), (4, 63, 128)])
def test_pages_equal_oracle_slices(eng, B, N, D):
    q, g = rand(B, D, seed=B + N), rand(N, D, seed=N + D, scale=D ** -0.5)
    ranks = _rankings(chain.chain_scores(q.numpy(), g.numpy()))
    qd, gd = q.cuda(), g.cuda()
    for k in (1, 50, 64, 1024):
        for off in _offsets(N, k):
            _same(eng.rank_page(qd, gd, off, k), _slice(ranks, [off] * B, k))
        per_query = np.array([(_offsets(N, k)[(3 * r + 1) % 11]) for r in range(B)], dtype=np.int32)      # one call, another offset per query
        _same(eng.rank_page(qd, gd, torch.from_numpy(per_query), k), _slice(ranks, per_query, k))
    s, i = eng.rank_page(qd, gd, N - 1, 64)
    assert (i[:, 1:] == -1).all() and torch.isneginf(s[:, 1:]).all() and (i[:, 0] >= 0).all()      # unfilled slots are exactly -inf / -1


# ---- tie-heavy data ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D", [(5, 3000, 128), (3, 1000, 64)])
def test_tie_heavy_pages_and_selects_split_runs_by_index(eng, B, N, D):
    q, g = int_unit(B, D, seed=41), int_unit(N, D, seed=42)
    ranks = _rankings(chain.chain_scores(q.numpy(), g.numpy()))
    offsets = [1, 63, 64, 500, N // 2 + 1, 999, N - 51]
    # the data is what the test is about: at most page boundaries the score at place `offset` is shared with another row
    shared = [(ranks[b][0] == ranks[b][0][off]).sum() > 1 for b in range(B) for off in offsets]
    assert sum(shared) * 2 >= len(shared)
    qd, gd = q.cuda(), g.cuda()
    for off in offsets:
        for k in (50, 1024):
            _same(eng.rank_page(qd, gd, off, k), _slice(ranks, [off] * B, k))
    places = np.array([offsets + [0, N - 1, N, -1]] * B, dtype=np.int32)
    got = eng.rank_select(qd, gd, torch.from_numpy(places))
    assert np.array_equal(_u64(got), _keys_at(ranks, places))
    back = eng.rank_count(qd, gd, got).cpu().numpy()
    assert np.array_equal(back, np.where((places >= 0) & (places < N), places, -1))


def test_a_tie_flood_pages_through_the_capacity_free_fallback(eng):
    """9000 identical rows: every score ties, the ranking is the index order, and a page whose ceiling leaves more than the select
    kernel's 4096 collected rows eligible (offsets 0, 1000, 4000) is ranked by the radix fallback UNDER the ceiling; the deeper ones
    (6000, 8990) fit the kernel's capacity again."""
    from fashionern_aaai2024_amd.engine import next_from
    B, N, D = 2, 9000, 64
    q = int_unit(B, D, seed=61)
    g = int_unit(1, D, seed=62).repeat(N, 1)
    ranks = _rankings(chain.chain_scores(q.numpy(), g.numpy()))
    assert all(np.array_equal(r[1], np.arange(N)) for r in ranks)
    qd, gd = q.cuda(), g.cuda()
    for off in (0, 1000, 4000, 6000, 8990):
        for k in (64, 1024):
            _same(eng.rank_page(qd, gd, off, k), _slice(ranks, [off] * B, k))
    first = eng.rank_page(qd, gd, 1000, 1024)
    _same(eng.sim_topk_from(qd, gd, 1024, next_from(*first)), _slice(ranks, [2024] * B, 1024))
    places = np.array([[0, 1, 4095, 4096, 8999, 9000, -1, 5000]] * B, dtype=np.int32)
    assert np.array_equal(_u64(eng.rank_select(qd, gd, torch.from_numpy(places))), _keys_at(ranks, places))


# ---- rank_select is the inverse of the ranks ----------------------------------------------------------------------------------------------
def _spread_places(b, n, m, seed):
    rng = np.random.default_rng(seed)
    p = np.linspace(0, n - 1, m).astype(np.int64)[None, :].repeat(b, axis=0)
    p = np.where(rng.random((b, m)) < 0.5, p, rng.integers(0, n, size=(b, m)))
    for r in range(b):
        p[r, rng.integers(m)] = (-1, n, n + 3, p[r, 0])[r % 4]
    return p.astype(np.int32)


@pytest.mark.parametrize("B,N,D", [(5, 3000, 128), (1025, 300, 64)])
def test_rank_select_inverts_rank_keys_and_rank_count(eng, B, N, D):
    q, g = rand(B, D, seed=3 + B), rand(N, D, seed=5 + N, scale=D ** -0.5)
    ranks = _rankings(chain.chain_scores(q.numpy(), g.numpy()))
    qd, gd = q.cuda(), g.cuda()
    for m in (1, 3, 8, 13):
        places = _spread_places(B, N, m, seed=m)
        got = eng.rank_select(qd, gd, torch.from_numpy(places))
        assert got.dtype == torch.int64 and tuple(got.shape) == (B, m)
        assert np.array_equal(_u64(got), _keys_at(ranks, places)), m
        inside = (places >= 0) & (places < N)
        rows = np.array([[ranks[r][1][p] if ok else -1 for p, ok in zip(places[r], inside[r])] for r in range(B)], dtype=np.int32)
        assert np.array_equal(_u64(got), _u64(eng.rank_keys(qd, gd, torch.from_numpy(rows)))), m      # bit for bit the row's own key; 0 past the end
        assert np.array_equal(eng.rank_count(qd, gd, got).cpu().numpy(), np.where(inside, places, -1)), m
    flat = _spread_places(B, N, 1, seed=77)
    got = eng.rank_select(qd, gd, torch.from_numpy(flat[:, 0]))
    assert tuple(got.shape) == (B,) and np.array_equal(_u64(got), _keys_at(ranks, flat)[:, 0])


# ---- cursors ---------------------------------------------------------------------------------------------------------------------------
def test_cursor_pages_concatenate_to_the_whole_ranking(eng):
    from fashionern_aaai2024_amd.engine import next_from
    B, N, D, K = 3, 2500, 128, 1024
    q, g = rand(B, D, seed=8), rand(N, D, seed=9, scale=D ** -0.5)
    ranks = _rankings(chain.chain_scores(q.numpy(), g.numpy()))
    qd, gd = q.cuda(), g.cuda()
    cursor = torch.full((B,), ALL, dtype=torch.int64)
    filled = []
    for page in range(4):
        s, i = eng.sim_topk_from(qd, gd, K, cursor)
        _same((s, i), _slice(ranks, [page * K] * B, K))
        filled.append(int((i[0] >= 0).sum()))
        cursor = next_from(s, i)
    assert filled == [1024, 1024, 452, 0] and (cursor == 0).all()
    for k in (1, 64, 1024):
        deep = eng.sim_topk_deep(qd, gd, k)
        want = (deep[0].cpu().numpy(), deep[1].cpu().numpy())
        _same(eng.sim_topk_from(qd, gd, k, torch.full((B,), ALL, dtype=torch.int64)), want)
        _same(eng.rank_page(qd, gd, 0, k), want)
        _same(want, _slice(ranks, [0] * B, k))
    s, i = eng.sim_topk_from(qd, gd, 64, torch.zeros(B, dtype=torch.int64))
    assert (i == -1).all() and torch.isneginf(s).all()


def test_ranking_to_depth_on_the_engine(eng):
    from fashionern_aaai2024_amd.run._common import ranking_to_depth
    B, N, D = 3, 1300, 64
    q, g = int_unit(B, D, seed=71), int_unit(N, D, seed=72)
    ranks = _rankings(chain.chain_scores(q.numpy(), g.numpy()))
    got = ranking_to_depth(eng, q.cuda(), g.cuda(), 1500)
    assert got.dtype == np.int32 and got.shape == (B, 1500)
    assert np.array_equal(got, _slice(ranks, [0] * B, 1500)[1])          # two cursor pages, -1 past the 1300 rows
    ex = np.array([ranks[0][1][0], -1, ranks[2][1][1100]], dtype=np.int32)
    cut = ranking_to_depth(eng, q.cuda(), eng.prepare_gallery(g.cuda()), 1200, page=500, exclude_idx=ex)
    assert np.array_equal(cut, _slice(_rankings(chain.chain_scores(q.numpy(), g.numpy()), exclude=ex), [0] * B, 1200)[1])


# ---- a ceiling whose index is foreign to the call ----------------------------------------------------------------------------------------
def test_a_global_cursor_continues_the_list_on_every_shard(eng):
    from fashionern_aaai2024_amd.engine import next_from
    B, N, D, K, CUT = 6, 701, 64, 100, 351
    q, g = int_unit(B, D, seed=51), int_unit(N, D, seed=52)
    ranks = _rankings(chain.chain_scores(q.numpy(), g.numpy()))
    qd, gd = q.cuda(), g.cuda()
    first = eng.sim_topk_deep(qd, gd, K)
    cursor = next_from(*first)
    whole = eng.sim_topk_from(qd, gd, K, cursor)
    _same(whole, _slice(ranks, [K] * B, K))
    owner = 0xFFFFFFFF - ((_u64(cursor) + np.uint64(1)) & np.uint64(0xFFFFFFFF)).astype(np.int64)      # the row the cursor was taken from
    assert ((owner >= 0) & (owner < N)).all()
    assert (owner < CUT).any() and (owner >= CUT).any()      # the cursor row belongs to only one of the two calls, and to each for some query
    lo = eng.sim_topk_from(qd, gd[:CUT].contiguous(), K, cursor, idx_offset=0)
    hi = eng.sim_topk_from(qd, gd[CUT:].contiguous(), K, cursor, idx_offset=CUT)
    merged = eng.topk_merge(torch.stack([lo[0], hi[0]]), torch.stack([lo[1], hi[1]]))
    _same(merged, (whole[0].cpu().numpy(), whole[1].cpu().numpy()))


# ---- exclude_idx, idx_offset, row_filter -------------------------------------------------------------------------------------------------
def test_exclusion_offset_and_row_filter(eng):
    from fashionern_aaai2024_amd.engine import RowFilter, next_from
    B, N, D, OFF = 5, 3000, 128, 1000
    q, g = rand(B, D, seed=21), rand(N, D, seed=22, scale=D ** -0.5)
    rng = np.random.default_rng(23)
    tags = (rng.integers(0, 3, size=N) | (rng.integers(0, 16, size=N) << 4)).astype(np.int32)      # a three-valued field below other bits
    mask = np.array([3, 3, 0, 3, 3], dtype=np.int32)
    value = np.array([0, 1, 0, 2, 4], dtype=np.int32)                 # query 2 accepts every row, query 4 no row: value outside mask
    eligible = (tags[None, :] & mask[:, None]) == value[:, None]
    assert eligible[2].all() and not eligible[4].any() and all(0 < eligible[b].sum() < N for b in (0, 1, 3))
    scores = chain.chain_scores(q.numpy(), g.numpy())
    plain = _rankings(scores, OFF)
    ex = np.array([plain[0][1][0], -1, plain[2][1][40], OFF + N + 2, plain[4][1][3]], dtype=np.int32)      # global indices
    ranks = _rankings(scores, OFF, exclude=ex, eligible=eligible)
    assert [len(r[1]) for r in ranks][4] == 0 and len(ranks[2][1]) == N - 1
    rf = RowFilter(torch.from_numpy(tags), torch.from_numpy(mask), torch.from_numpy(value))
    kw = dict(idx_offset=OFF, exclude_idx=torch.from_numpy(ex), row_filter=rf)
    qd, gd = q.cuda(), g.cuda()
    for off in (0, 70, 900, 1024):
        for k in (64, 1024):
            _same(eng.rank_page(qd, gd, off, k, **kw), _slice(ranks, [off] * B, k))
    cursor = torch.full((B,), ALL, dtype=torch.int64)
    for page in range(4):
        s, i = eng.sim_topk_from(qd, gd, 1024, cursor, **kw)
        _same((s, i), _slice(ranks, [page * 1024] * B, 1024))
        cursor = next_from(s, i)
    places = np.array([[0, 1, 39, 40, 41, 500, 998, 999, 1000, 1500, 2998, 2999, -1]] * B, dtype=np.int32)
    got = eng.rank_select(qd, gd, torch.from_numpy(places), **kw)
    assert np.array_equal(_u64(got), _keys_at(ranks, places))
    count = eng.rank_count(qd, gd, got, **kw).cpu().numpy()
    lens = np.array([len(r[1]) for r in ranks])[:, None]
    assert np.array_equal(count, np.where((places >= 0) & (places < lens), places, -1))
    # exclusion and offset without a filter
    ranks = _rankings(scores, OFF, exclude=ex)
    kw.pop("row_filter")
    _same(eng.rank_page(qd, gd, 1990, 1024, **kw), _slice(ranks, [1990] * B, 1024))
    assert np.array_equal(_u64(eng.rank_select(qd, gd, torch.from_numpy(places), **kw)), _keys_at(ranks, places))


# ---- gallery forms ----------------------------------------------------------------------------------------------------------------------
def test_bf16_and_prepared_gallery_forms(eng):
    from fashionern_aaai2024_amd.engine import next_from
    B, N, D = 4, 3001, 128
    q, g = rand(B, D, seed=31), rand(N, D, seed=32, scale=D ** -0.5)
    pg = eng.prepare_gallery(g.cuda())
    qd = q.cuda()
    approx = eng.sweep_bf16_scores(qd, pg, tile_max=False).cpu().numpy()      # the bf16 form ranks exactly these values
    ranks = _rankings(approx)
    places = np.array([[0, 7, 1023, 1024, 2000, 3000, 3001]] * B, dtype=np.int32)
    for off in (0, 1000, 2990):
        for k in (50, 1024):
            _same(eng.rank_page(qd, pg.bf16, off, k), _slice(ranks, [off] * B, k))
    assert np.array_equal(_u64(eng.rank_select(qd, pg.bf16, torch.from_numpy(places))), _keys_at(ranks, places))
    first = eng.sim_topk_deep(qd, pg.bf16, 1024)
    _same(eng.sim_topk_from(qd, pg.bf16, 1024, next_from(*first)), _slice(ranks, [1024] * B, 1024))
    # a PreparedGallery ranks on its fp32 rows: the fp32 tensor's bits
    exact = _rankings(chain.chain_scores(q.numpy(), g.numpy()))
    for gal in (g.cuda(), pg):
        _same(eng.rank_page(qd, gal, 1500, 1024), _slice(exact, [1500] * B, 1024))
        assert np.array_equal(_u64(eng.rank_select(qd, gal, torch.from_numpy(places))), _keys_at(exact, places))


# ---- argument refusals -------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_name_the_function(eng):
    from fashionern_aaai2024_amd._lib import FernError
    q, g = rand(2, 64, seed=1).cuda(), rand(10, 64, seed=2).cuda()
    cursor = torch.full((2,), ALL, dtype=torch.int64)
    for k in (0, 1025):
        with pytest.raises(FernError, match=r"\(-1\): fern_sim_topk_page: need 1<=K<=1024"):
            eng.rank_page(q, g, 0, k)
        with pytest.raises(FernError, match=r"\(-1\): fern_sim_topk_from: need 1<=K<=1024"):
            eng.sim_topk_from(q, g, k, cursor)
    places = torch.zeros((2, 1), dtype=torch.int32, device="cuda")
    keys = torch.zeros((2, 1), dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    assert eng.lib.fern_rank_select(eng._h, p(q), p(g), None, 2, 10, 64, p(places), 0, 0, None, p(keys), None, None, None, None) == -1
    assert b"fern_rank_select: need m >= 1" in eng.lib.fern_last_error()
    q48, g48 = rand(2, 48, seed=1).cuda(), rand(10, 48, seed=2).cuda()
    with pytest.raises(FernError, match=r"\(-1\): fern_sim_topk_page: the fp32 form needs D % 32 == 0"):
        eng.rank_page(q48, g48, 0, 5)
    with pytest.raises(FernError, match=r"\(-1\): fern_rank_select: the fp32 form needs D % 32 == 0"):
        eng.rank_select(q48, g48, places)
    with pytest.raises(FernError, match=r"\(-1\): fern_sim_topk_from: the fp32 form needs D % 32 == 0"):
        eng.sim_topk_from(q48, g48, 5, cursor)
    q1k, g1k = rand(2, 1024, seed=1).cuda(), rand(10, 1024, seed=2).cuda().bfloat16()
    with pytest.raises(FernError, match=r"\(-1\): fern_sim_topk_page: a bf16-only gallery needs D % 64 == 0, D <= 768"):
        eng.rank_page(q1k, g1k, 0, 5)
    with pytest.raises(FernError, match=r"\(-1\): fern_rank_select: a bf16-only gallery needs D % 64 == 0, D <= 768"):
        eng.rank_select(q1k, g1k, places)

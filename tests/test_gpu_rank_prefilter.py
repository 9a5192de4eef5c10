"""The fp32-gallery ranking stage as a CERTIFIED bf16 pre-filter + exact fp32 rescoring (fern_gallery_prepare /
fern_sim_topk_prefiltered; FernEngine.prepare_gallery + sim_topk), through the C ABI.

Reference semantics are fern_sim_topk's: `distances = 1 - q @ g.T; argsort(distances)[:, :K]` on the fp32 gallery
(run/test/test_fiq.py:49-50).  The contract of the pre-filter is that NOTHING about the result depends on the bf16 scores: the
scores returned are the exact fp32 fma-chain scores (oracle/chain.c), the ordering is the chain's, bit for bit -- including on
galleries built so that the bf16 ranking is wrong (rows inside the margin), on ties, with exclusions, and when the candidates do
not fit and the exact pass takes over."""
import numpy as np
import pytest
import torch

from oracle import chain
from oracle import rank as orank
from support import fresh_engine, int_unit, rand, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["auto", "lists", "dense"])
def engine(request):
    """Every test of this file runs under each form of the stage (include/fern.h: fern_rank_strategy): the cost model's pick, the
    candidate-list form and the dense form (which falls back to the lists beyond its size limit) -- all must give the same bits."""
    eng = request.getfixturevalue("_session_engine")
    eng.set_rank_strategy(request.param)
    yield eng
    eng.set_rank_strategy("auto")


@pytest.fixture(scope="module")
def _session_engine():
    yield from fresh_engine()


@pytest.mark.parametrize("B,N,D", [(3, 1000, 64), (64, 9001, 640), (130, 3000, 128), (1, 70_000, 512), (64, 46_000, 512), (5, 40, 64), (2, 7, 1024),
                                   (9, 200_003, 128)])
def test_prefiltered_ranking_is_bit_identical_to_the_fma_chain(engine, B, N, D):
    """Random operands at the shapes of test_sim_topk_bit_identical_to_the_fma_chain plus BASELINE C2's (64 x 46 000 x 512) and
    galleries smaller than K: same bits as the sequential fp32 fma chain, same ranking -- and the same as the plain fp32 stage."""
    q, g = rand(B, D, seed=B + N), rand(N, D, seed=N + D, scale=D ** -0.5)
    pg = engine.prepare_gallery(g)
    s, i = engine.sim_topk(q, pg, 50)
    cs, ci = chain.chain_topk(q.numpy(), g.numpy(), 50)
    m = min(N, 50)                                         # fewer rows than K: the tail is (-inf, -1)
    assert same_bits((s[:, :m], i[:, :m]), (cs, ci))
    assert (i[:, m:].cpu() == -1).all() and torch.isinf(s[:, m:].cpu()).all()
    s0, i0 = engine.sim_topk(q, g, 50)
    assert torch.equal(s, s0) and torch.equal(i, i0)


def test_prepare_reports_the_norms_that_certify_the_margin(engine):
    """meta = {max ||g - bf16(g)||, max ||bf16(g)||, max ||g||}; with them |exact - bf16 score| <= eps_b of include/fern.h for every
    (query, row) -- checked against the actual errors of the bf16 operands in float64."""
    d = 512
    q, g = rand(32, d, seed=5, scale=0.7), rand(20_000, d, seed=6, scale=d ** -0.5)
    g[17] *= 9.0                                           # one long row sets the maxima
    pg = engine.prepare_gallery(g)
    gb = g.bfloat16().float()
    assert torch.equal(pg.bf16.cpu().view(torch.int16), g.bfloat16().view(torch.int16))
    want = torch.stack([(g - gb).norm(dim=1).max(), gb.norm(dim=1).max(), g.norm(dim=1).max()])
    meta = pg.meta.cpu()
    assert torch.allclose(meta[:3], want, rtol=1e-5) and meta[3] == 0
    qb = q.bfloat16().float()
    err = (q.double() @ g.double().T - qb.double() @ gb.double().T).abs()                    # [32, 20000]
    eps = q.double().norm(dim=1) * meta[0].double() + (q - qb).double().norm(dim=1) * meta[1].double()
    assert (err.max(dim=1).values <= eps).all()
    assert err.max() > 1e-3 * eps.max()                   # ... and the bound is a bound on something (Cauchy-Schwarz is ~sqrt(D) loose on random rows)


@pytest.mark.parametrize("near", [400, 3000])
def test_rows_inside_the_margin_are_rescored_not_trusted(engine, near):
    """`near` gallery rows score within ~1e-4 of each other for every query (they are the query direction plus a little noise),
    far inside the bf16 error (~1e-3): the bf16 ranking of them is scrambled -- asserted -- and only the exact rescoring can order
    them.  400 rows fit the rescoring kernel; 3000 exceed its 1024 survivors and take the exact pass.  Result = the chain's, bit for bit."""
    d, n, k = 512, 30_000, 50
    base = torch.nn.functional.normalize(rand(1, d, seed=77), dim=-1)
    q = torch.nn.functional.normalize(base + 0.02 * rand(8, d, seed=78) * d ** -0.5, dim=-1)
    g = torch.nn.functional.normalize(rand(n, d, seed=79), dim=-1)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(80))[:near]
    g[rows] = torch.nn.functional.normalize(base + 0.03 * rand(near, d, seed=81) * d ** -0.5, dim=-1)
    cs, ci = chain.chain_topk(q.numpy(), g.numpy(), k)
    approx = (q.bfloat16().float() @ g.bfloat16().float().T).topk(k, dim=1).indices
    scrambled = sum(set(a.tolist()) != set(b.tolist()) for a, b in zip(approx, torch.from_numpy(ci.astype(np.int64))))
    assert scrambled >= 6, "the case must be one where the bf16 scores pick the wrong rows"
    s, i = engine.sim_topk(q, engine.prepare_gallery(g), k)
    assert same_bits((s, i), (cs, ci))


@pytest.mark.parametrize("n", [1, 63, 1025, 65_537])
def test_all_scores_equal_only_the_index_breaks_ties(engine, n):
    d, k = 64, 50
    q = int_unit(3, d, 5)
    g = int_unit(1, d, 6).repeat(n, 1)
    rs, ri = orank.cosine_topk(q, g, k)
    s, i = engine.sim_topk(q, engine.prepare_gallery(g), k)
    engine.sync()
    assert torch.equal(i.cpu(), ri) and torch.equal(s.cpu(), rs)


def test_exclusion_offsets_and_large_batches(engine):
    """CIRR's shape (BASELINE C4): B crosses the 1024-query plan chunk and the 128-query sweep blocks, K = 51, one excluded
    gallery index per query, idx_offset of a gallery shard."""
    n, d = 21_552, 64
    q, g = rand(1300, d, seed=51), rand(n, d, seed=52, scale=d ** -0.5)
    ex = torch.randint(0, n, (1300,), generator=torch.Generator().manual_seed(3), dtype=torch.int32) + 7000
    pg = engine.prepare_gallery(g)
    s, i = engine.sim_topk(q, pg, 51, idx_offset=7000, exclude_idx=ex)
    s0, i0 = engine.sim_topk(q, g, 51, idx_offset=7000, exclude_idx=ex)
    engine.sync()
    assert torch.equal(s, s0) and torch.equal(i, i0)
    assert not (i.cpu() == ex[:, None]).any()
    cs, ci = chain.chain_topk(q[:40].numpy(), g.numpy(), 52)            # the chain's top-52 minus the excluded row = the top-51
    for b in range(40):
        keep = [(sc, ix + 7000) for sc, ix in zip(cs[b], ci[b]) if ix + 7000 != int(ex[b])][:51]
        assert [x for _, x in keep] == i[b].cpu().tolist()
        assert np.array_equal(np.array([x for x, _ in keep], np.float32).view(np.uint32), s[b].cpu().numpy().view(np.uint32))


def test_large_dense_gallery_with_exclusions_spread_over_the_row(engine):
    """A gallery beyond the three register-held batches of the dense kernel (49 152 rows: the streaming path), the excluded row of each
    query is its best row, spread over the whole row range; N is not a multiple of anything."""
    n, d, k = 150_001, 64, 50
    q, g = rand(7, d, seed=61), rand(n, d, seed=62, scale=d ** -0.5)
    ex_rows = [0, 37_000, 49_151, 49_152, 75_001, 120_000, 150_000]
    for b, row in enumerate(ex_rows):
        g[row] = q[b] * 3.0
    ex = torch.tensor(ex_rows, dtype=torch.int32)
    s, i = engine.sim_topk(q, engine.prepare_gallery(g), k, exclude_idx=ex)
    s0, i0 = engine.sim_topk(q, g, k, exclude_idx=ex)
    assert torch.equal(s, s0) and torch.equal(i, i0) and not (i.cpu() == ex[:, None]).any()
    s, i = engine.sim_topk(q, engine.prepare_gallery(g), k)                  # ... and without the exclusion those rows rank first
    assert i[:, 0].cpu().tolist() == ex_rows


def test_excluded_row_is_the_best_row_and_a_sampled_row(engine):
    from test_gpu_rank_fused import plan, sample_row                     # the plain plan's sample; the pre-filter's is denser at this N
    n, d, k = 70_000, 64, 5
    q, g = int_unit(6, d, 31), int_unit(n, d, 32)
    s_rows = max(n // 32, min(n, 4096))
    r = n // s_rows
    ex_rows = [sample_row(c, r) for c in (0, 17, 500, s_rows - 1, 3, 9)]
    for b, row in enumerate(ex_rows):
        g[row] = torch.sign(q[b]) / 8.0 + (q[b] == 0) * 0.125
    ex = torch.tensor(ex_rows, dtype=torch.int32)
    rs, ri = orank.cosine_topk(q, g, k, exclude_idx=ex)
    s, i = engine.sim_topk(q, engine.prepare_gallery(g), k, exclude_idx=ex)
    assert torch.equal(i.cpu(), ri) and torch.equal(s.cpu(), rs)
    assert plan(n)[0] <= s_rows


def test_rows_of_very_different_lengths(engine):
    """Un-normalised operands: the margin scales with the longest gallery row, so short rows' scores sit deep inside it."""
    n, d, k = 20_000, 128, 50
    q = rand(9, d, seed=91) * 3.7
    g = rand(n, d, seed=92) * torch.logspace(-1, 1.3, n)[torch.randperm(n, generator=torch.Generator().manual_seed(93))][:, None]
    cs, ci = chain.chain_topk(q.numpy(), g.numpy(), k)
    s, i = engine.sim_topk(q, engine.prepare_gallery(g), k)
    assert same_bits((s, i), (cs, ci))


def test_prepared_gallery_is_refilled_in_place_and_feeds_the_pipeline_entry_points(engine):
    d = 64
    g1, g2, q = rand(5000, d, seed=1, scale=0.1), rand(5000, d, seed=2, scale=0.1), rand(4, d, seed=3)
    pg = engine.prepare_gallery(g1)
    pg2 = engine.prepare_gallery(g2, out=pg)
    assert pg2.bf16.data_ptr() == pg.bf16.data_ptr() and pg2.meta.data_ptr() == pg.meta.data_ptr()
    s, i = engine.sim_topk(q, pg2, 10)
    s0, i0 = engine.sim_topk(q, g2, 10)
    assert torch.equal(s, s0) and torch.equal(i, i0)
    idx = torch.tensor([[0, 5, 4999, -1]] * 4, dtype=torch.int32)
    assert torch.equal(engine.gather_scores(q, pg2, idx), engine.gather_scores(q, g2, idx))
    s, i = engine.sim_topk(q, engine.prepare_gallery(g2[:0]), 10)        # an empty shard
    assert (i.cpu() == -1).all()


# ---- dense form on the sweep's tile maxima (galleries of >= 16 384 rows, one 64-query block per sweep) ---------------------------------
@pytest.mark.parametrize("B,N,D", [(64, 46_000, 512), (5, 16_411, 640), (64, 100_001, 64), (3, 31, 128)])
def test_sweep_scores_are_the_bf16_products_and_tile_maxima_the_maxima_of_32_rows(_session_engine, B, N, D):
    """fern_sweep_bf16_scores: every approximate score is the bf16 operands' dot product (fp32 accumulation: compared with float64 of
    the same rounded operands), inside the certified eps_b of the exact score; tile_max[b][t] is bit for bit the largest of
    scores[b][32 t : 32 t + 32] -- the dense form reads those instead of the rows."""
    eng = _session_engine
    q, g = rand(B, D, seed=3 * B + N), rand(N, D, seed=N - D, scale=D ** -0.5)
    pg = eng.prepare_gallery(g)
    scores, tmax = eng.sweep_bf16_scores(q, pg)
    scores, tmax = scores.cpu(), tmax.cpu()
    ref = (q.bfloat16().double() @ g.bfloat16().double().T)
    assert (scores.double() - ref).abs().max() < 1e-5 * max(1.0, float(ref.abs().max()))
    pad = torch.full((B, (-N) % 32), -float("inf"))
    want = torch.cat([scores, pad], dim=1).view(B, -1, 32).max(dim=2).values
    assert torch.equal(tmax, want)
    meta = pg.meta.cpu().double()
    eps = q.double().norm(dim=1) * meta[0] + (q - q.bfloat16().float()).double().norm(dim=1) * meta[1]
    exact = q.double() @ g.double().T
    assert ((scores.double() - exact).abs().max(dim=1).values <= eps * 1.01 + 1e-6).all()


@pytest.mark.parametrize("B,N,D", [(5, 300_017, 64), (70, 140_000, 64), (1, 16_384, 64), (33, 262_145, 64), (7, 20_011, 768), (66, 17_000, 192)])
def test_tile_maxima_form_beyond_one_register_batch_and_with_split_query_blocks(engine, B, N, D):
    """N / 32 beyond the 8 192 tile maxima a workgroup holds in registers (the re-reading instance); 65..128 queries on a gallery of
    >= 131 072 rows (the sweep runs one 64-query block per launch so that it can leave tile maxima); the smallest gallery of the form;
    excluded rows = each query's best row, in tiles spread over the whole gallery; D = 768 / 192: the sweep's generic form (queries in
    LDS, no compile-time D), the second with more than 64 queries.  Bits of the fp32 stage, every time."""
    q, g = rand(B, D, seed=B + N), rand(N, D, seed=N + D, scale=D ** -0.5)
    ex_rows = [(b * 7919 * 31 + 5) % N for b in range(B)]
    for b, row in enumerate(ex_rows):
        g[row] = q[b] * 2.0
    ex = torch.tensor(ex_rows, dtype=torch.int32)
    pg = engine.prepare_gallery(g)
    for exclude in (ex, None):
        s, i = engine.sim_topk(q, pg, 50, exclude_idx=exclude)
        s0, i0 = engine.sim_topk(q, g, 50, exclude_idx=exclude)
        assert torch.equal(s, s0) and torch.equal(i, i0)
    assert i[:, 0].cpu().tolist() == ex_rows
    nq = min(B, 6)
    cs, ci = chain.chain_topk(q[:nq].numpy(), g.numpy(), 50)
    assert same_bits((s[:nq], i[:nq]), (cs, ci))


def test_more_listed_tiles_than_the_kernel_holds_takes_the_exact_ranking(engine):
    """6 000 rows within 1e-4 of each other spread over ~2 700 of the gallery's 3 125 tiles: every wave lists more than its 512 tiles and
    the query is ranked exactly behind the bound it had reached -- the chain's result, bit for bit."""
    d, n, k, near = 128, 100_000, 50, 6000
    base = torch.nn.functional.normalize(rand(1, d, seed=7), dim=-1)
    q = torch.nn.functional.normalize(base + 0.02 * rand(4, d, seed=8) * d ** -0.5, dim=-1)
    g = torch.nn.functional.normalize(rand(n, d, seed=9), dim=-1)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(10))[:near]
    g[rows] = torch.nn.functional.normalize(base + 0.03 * rand(near, d, seed=11) * d ** -0.5, dim=-1)
    assert len(set((rows // 32).tolist())) > 2048
    cs, ci = chain.chain_topk(q.numpy(), g.numpy(), k)
    s, i = engine.sim_topk(q, engine.prepare_gallery(g), k)
    assert same_bits((s, i), (cs, ci))


def test_gallery_past_the_inline_exact_limit_sends_floods_to_the_gated_exact_pass(engine):
    """300 000 x 128 fp32 = 154 MB: beyond what one workgroup may stream by itself, so a query without room (all rows equal: every tile is
    listed) is flagged for the gated exact-pass launch instead; ties break by index."""
    d, k, n = 128, 50, 300_000
    q = int_unit(3, d, 5)
    g = int_unit(1, d, 6).repeat(n, 1)
    g[123_456] = torch.sign(q[1]) / 8.0 + (q[1] == 0) * 0.125           # one row stands out for query 1
    rs, ri = orank.cosine_topk(q, g, k)
    s, i = engine.sim_topk(q, engine.prepare_gallery(g), k)
    assert torch.equal(i.cpu(), ri) and torch.equal(s.cpu(), rs)


def test_non_finite_rows_leave_no_certificate_and_the_stage_falls_back_to_the_exact_ranking(engine):
    """An inf / NaN gallery row makes the margin non-finite: nothing is certified, every query takes the exact ranking -- the same bits as
    the fp32 stage on that gallery."""
    n, d, k = 40_000, 64, 50
    q, g = rand(6, d, seed=1), rand(n, d, seed=2, scale=d ** -0.5)
    g[777, 3] = float("inf")
    pg = engine.prepare_gallery(g)
    s, i = engine.sim_topk(q, pg, k)
    s0, i0 = engine.sim_topk(q, g, k)
    assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))


def test_prepared_shards_with_offsets_merge_to_the_unsharded_ranking(engine):
    """The multi-GPU layout (distributed.sharded_topk): every rank ranks its own PREPARED shard of the gallery with its row
    offset and the queries' global exclusions, the per-shard top-K lists are merged (fern_topk_merge).  Shards of very different sizes
    take different forms of the stage (row walk, tile maxima, lists) -- the merged result is the unsharded fp32 ranking, bit for bit."""
    n, d, k = 120_000, 128, 50
    q, g = rand(40, d, seed=71), rand(n, d, seed=72, scale=d ** -0.5)
    ex = torch.randint(0, n, (40,), generator=torch.Generator().manual_seed(7), dtype=torch.int32)
    for b in range(40):
        g[int(ex[b])] = q[b] * 1.5                                     # the excluded row would rank first
    cuts = [0, 700, 9_000, 60_000, n]                                  # 700 / 8 300 / 51 000 / 60 000 rows
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        parts.append(engine.sim_topk(q, engine.prepare_gallery(g[lo:hi].contiguous()), k, idx_offset=lo, exclude_idx=ex))
    ms, mi = engine.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    s0, i0 = engine.sim_topk(q, g, k, exclude_idx=ex)
    assert torch.equal(ms, s0) and torch.equal(mi, i0) and not (mi.cpu() == ex[:, None]).any()


@pytest.mark.parametrize("k", [1, 2, 63, 64])
def test_smallest_and_largest_k_with_exclusions(engine, k):
    """K = 1 and K = 64 (the ABI's limits) with an excluded best row: the tile-maxima bound needs ceil((K + 1) / 4) tiles per wave."""
    n, d = 33_000, 64
    q, g = rand(9, d, seed=5 + k), rand(n, d, seed=6 + k, scale=d ** -0.5)
    ex_rows = [(b * 3671 + 11) % n for b in range(9)]
    for b, row in enumerate(ex_rows):
        g[row] = q[b] * 2.0
    ex = torch.tensor(ex_rows, dtype=torch.int32)
    pg = engine.prepare_gallery(g)
    for exclude in (ex, None):
        s, i = engine.sim_topk(q, pg, k, exclude_idx=exclude)
        s0, i0 = engine.sim_topk(q, g, k, exclude_idx=exclude)
        assert torch.equal(s, s0) and torch.equal(i, i0)
    cs, ci = chain.chain_topk(q.numpy(), g.numpy(), k)
    assert same_bits((s, i), (cs, ci)) and i[:, 0].cpu().tolist() == ex_rows

"""Ranking pages without a GPU: the C ABI entry points fern_rank_select / fern_sim_topk_from / fern_sim_topk_page (header, library,
ctypes table, argument checks), the torch helpers engine.ranking_keys / engine.next_from against the numpy key definition,
distributed.rank_from_sharded over gloo and run/_common.ranking_to_depth, the last two on a TEST-ONLY stub engine that ranks by the
key definition of include/fern.h."""
import os
import re

import numpy as np
import torch
import torch.distributed as dist

import gloo
from rank_oracle import RankOracle, make_keys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NAMES = (("fern_rank_select", 16), ("fern_sim_topk_from", 17), ("fern_sim_topk_page", 17))


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def test_page_entry_points_are_declared_exported_and_typed():
    from fashionern_aaai2024_amd import _lib
    header = open(os.path.join(ROOT, "include", "fern.h")).read()
    lib = _lib.load()
    for name, nargs in NAMES:
        assert re.search(rf"FERN_API int {name}\(", header)
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert "run/test/test_fiq.py:49-50" in header
    assert re.search(r"#define FERN_ABI_VERSION 3\b", header)
    assert lib.fern_abi_version() == 3


def test_page_argument_errors_name_the_function():
    from fashionern_aaai2024_amd import _lib
    lib = _lib.load()
    p = 0x1000                                           # never dereferenced: every call below is refused before any HIP call
    assert lib.fern_rank_select(None, p, p, None, 2, 10, 64, p, 1, 0, None, p, None, None, None, None) == -1
    assert b"fern_rank_select: ctx is NULL" in lib.fern_last_error()
    assert lib.fern_sim_topk_from(None, p, p, None, 2, 10, 64, 5, p, p, p, 0, None, None, None, None, None) == -1
    assert b"fern_sim_topk_from: ctx is NULL" in lib.fern_last_error()
    assert lib.fern_sim_topk_page(None, p, p, None, 2, 10, 64, 5, p, p, p, 0, None, None, None, None, None) == -1
    assert b"fern_sim_topk_page: ctx is NULL" in lib.fern_last_error()
    # the other refusals come first: a NULL context hides none of them
    for k in (0, 1025):
        assert lib.fern_sim_topk_from(None, p, p, None, 2, 10, 64, k, p, p, p, 0, None, None, None, None, None) == -1
        assert b"fern_sim_topk_from: need 1<=K<=1024" in lib.fern_last_error()
        assert lib.fern_sim_topk_page(None, p, p, None, 2, 10, 64, k, p, p, p, 0, None, None, None, None, None) == -1
        assert b"fern_sim_topk_page: need 1<=K<=1024" in lib.fern_last_error()
    assert lib.fern_rank_select(None, p, p, None, 2, 10, 64, p, 0, 0, None, p, None, None, None, None) == -1
    assert b"fern_rank_select: need m >= 1" in lib.fern_last_error()
    assert lib.fern_rank_select(None, p, p, None, 2, 10, 48, p, 1, 0, None, p, None, None, None, None) == -1
    assert b"fern_rank_select: the fp32 form needs D % 32 == 0" in lib.fern_last_error()
    assert lib.fern_sim_topk_page(None, p, None, p, 2, 10, 1024, 5, p, p, p, 0, None, None, None, None, None) == -1
    assert b"fern_sim_topk_page: a bf16-only gallery needs D % 64 == 0, D <= 768" in lib.fern_last_error()
    assert lib.fern_sim_topk_from(None, p, None, None, 2, 10, 64, 5, p, p, p, 0, None, None, None, None, None) == -1
    assert b"fern_sim_topk_from: gallery and gallery_bf16 are both NULL" in lib.fern_last_error()


# ---- ranking_keys / next_from ------------------------------------------------------------------------------------------------------
def _result(b, k, filled, seed):
    """A top-K result (scores, idx) [b, k] whose first filled[r] places of row r hold rows, the rest -inf / -1."""
    rng = np.random.default_rng(seed)
    s = np.sort(rng.standard_normal((b, k)).astype(np.float32), axis=1)[:, ::-1].copy()
    s[:, 0] = np.float32(0.0)                             # both signs and a zero
    s = np.sort(s, axis=1)[:, ::-1].copy()
    i = rng.integers(0, 2 ** 31 - 1, size=(b, k)).astype(np.int32)
    for r in range(b):
        s[r, filled[r]:] = -np.inf
        i[r, filled[r]:] = -1
    return s, i


def test_ranking_keys_equal_the_numpy_key_definition():
    from fashionern_aaai2024_amd.engine import ranking_keys
    s, i = _result(4, 9, [9, 9, 4, 0], seed=1)
    s[1, :3] = [np.float32(3.5), np.float32(-0.0), np.float32(-2.25)]
    i[1, :3] = [0, 2 ** 31 - 2, 7]
    want = np.where(i >= 0, make_keys(s, np.where(i >= 0, i, 0).astype(np.int64)), np.uint64(0))
    got = ranking_keys(torch.from_numpy(s), torch.from_numpy(i))
    assert got.dtype == torch.int64 and tuple(got.shape) == (4, 9)
    assert np.array_equal(got.numpy().view(np.uint64), want)
    assert (got[3] == 0).all() and (got[2, 4:] == 0).all() and (got[0] != 0).all()


def test_next_from_on_full_partial_and_empty_pages():
    from fashionern_aaai2024_amd.engine import next_from
    s, i = _result(3, 6, [6, 2, 0], seed=2)
    keys = make_keys(s, np.where(i >= 0, i, 0).astype(np.int64))
    got = next_from(torch.from_numpy(s), torch.from_numpy(i))
    assert got.dtype == torch.int64 and tuple(got.shape) == (3,)
    g = got.numpy().view(np.uint64)
    assert g[0] == keys[0, 5] - np.uint64(1)              # a full page: the key of its last place, minus 1
    assert g[1] == keys[1, 1] - np.uint64(1)              # a partly filled page: the last FILLED place
    assert g[2] == 0                                      # no filled place: the cursor that makes nothing eligible


# ---- the oracle engine (tests/rank_oracle.py: `sim_topk_from` by the key definition) ---------------------------------------------------
def _case():
    """Operands in {-1, 0, 1} / 8: every dot product is exact in fp32 in any order, so a shard's scores are the whole gallery's bit for
    bit and ties abound.  Ragged: 701 rows over two ranks are 351 + 350."""
    n, d, b = 701, 32, 4
    g = torch.Generator().manual_seed(9)
    gallery = torch.randint(-1, 2, (n, d), generator=g).float() / 8
    q = torch.randint(-1, 2, (b, d), generator=g).float() / 8
    return gallery, q


def _stable_ranking(q, gallery):
    s = (q @ gallery.T).numpy()
    return np.argsort(-s, axis=1, kind="stable").astype(np.int32)


PAGE = 256      # 701 rows: pages of 256, 256, 189 rows, then an empty one


def _follow(fn, b):
    from fashionern_aaai2024_amd.engine import next_from
    cursor = torch.full((b,), -1, dtype=torch.int64)
    pages = []
    for _ in range(4):
        s, i = fn(cursor)
        pages.append(i.numpy())
        cursor = next_from(s, i)
    return np.concatenate(pages, axis=1)


def _worker(rank, world, out_dir):
    from fashionern_aaai2024_amd import distributed as fd
    gallery, q = _case()
    eng = RankOracle()
    start, stop, _ = fd.shard_rows(gallery.shape[0], rank, world)
    ex = torch.tensor([3, -1, 400, 700], dtype=torch.int32)
    got = _follow(lambda c: fd.rank_from_sharded(eng, q, gallery[start:stop], start, PAGE, c), q.shape[0])
    excl = _follow(lambda c: fd.rank_from_sharded(eng, q, gallery[start:stop], start, PAGE, c, exclude_idx=ex), q.shape[0])
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), got=got, excl=excl)


def test_sharded_cursor_pages_equal_the_unsharded_ranking(tmp_path):
    gloo.spawn(2, _worker, str(tmp_path))
    gallery, q = _case()
    order = _stable_ranking(q, gallery)
    n = gallery.shape[0]
    s = (q @ gallery.T).numpy()
    # the data is what the test is about: most page boundaries fall inside a run of equal scores
    cut = [s[b, order[b, p - 1]] == s[b, order[b, p]] for b in range(q.shape[0]) for p in (PAGE, 2 * PAGE)]
    assert sum(cut) * 2 >= len(cut)
    ex = np.array([3, -1, 400, 700])
    for rank in range(2):
        got = np.load(tmp_path / f"r{rank}.npz")
        assert got["got"].shape == (q.shape[0], 4 * PAGE)
        assert np.array_equal(got["got"][:, :n], order)
        assert (got["got"][:, n:] == -1).all()
        for b in range(q.shape[0]):
            want = order[b][order[b] != ex[b]]
            assert np.array_equal(got["excl"][b, :len(want)], want)
            assert (got["excl"][b, len(want):] == -1).all()


def test_rank_from_sharded_makes_no_collective_in_a_world_of_one():
    from fashionern_aaai2024_amd import distributed as fd
    assert not (dist.is_available() and dist.is_initialized())
    gallery, q = _case()
    eng = RankOracle()
    got = _follow(lambda c: fd.rank_from_sharded(eng, q, gallery, 0, PAGE, c), q.shape[0])
    n = gallery.shape[0]
    assert np.array_equal(got[:, :n], _stable_ranking(q, gallery)) and (got[:, n:] == -1).all()


# ---- ranking_to_depth ------------------------------------------------------------------------------------------------------------
def test_ranking_to_depth_fills_cursor_pages_past_1024():
    from fashionern_aaai2024_amd.run._common import ranking_to_depth
    g = torch.Generator().manual_seed(11)
    gallery = torch.randint(-1, 2, (1700, 32), generator=g).float() / 8
    q = torch.randint(-1, 2, (3, 32), generator=g).float() / 8
    eng = RankOracle()
    order = _stable_ranking(q, gallery)
    got = ranking_to_depth(eng, q, gallery, 1500)
    assert got.dtype == np.int32 and got.shape == (3, 1500)
    assert np.array_equal(got, order[:, :1500])
    small = ranking_to_depth(eng, q, gallery[:40], 100, page=16)      # past N the entries are -1
    assert np.array_equal(small[:, :40], _stable_ranking(q, gallery[:40])) and (small[:, 40:] == -1).all()
    ex = np.array([order[0, 0], -1, order[2, 5]], dtype=np.int32)
    cut = ranking_to_depth(eng, q, gallery, 1100, page=1024, exclude_idx=ex)
    for b in range(3):
        assert np.array_equal(cut[b], order[b][order[b] != ex[b]][:1100])

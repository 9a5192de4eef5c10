"""Item-level ranking without a GPU: the C ABI entry points (header, library, ctypes table, argument checks), `ItemMap`'s rules,
`run/_common.recalls_items` and the 200k driver flag on the TEST-ONLY oracle engine (tests/items_oracle.py), and
`distributed.rank_items_sharded` / `item_rank_of_sharded` over gloo in worlds of two and three."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

import gloo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
META = json.load(open(os.path.join(HERE, "golden", "harness.json")))


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def test_item_entry_points_are_declared_exported_and_typed():
    from fashionern_aaai2024_amd import _lib
    header = open(os.path.join(ROOT, "include", "fern.h")).read()
    lib = _lib.load()
    for name, nargs in (("fern_sim_topk_items", 19), ("fern_item_rank", 18), ("fern_item_keys", 18), ("fern_item_count", 18)):
        assert re.search(rf"FERN_API int {name}\(", header)
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert "run/test/test_200k.py:52-60" in header and "dataloader/fashion200k_patch.py:282-290" in header
    assert lib.fern_abi_version() == 3 and "#define FERN_ABI_VERSION 3" in header
    assert "items.hip" in __import__("fashionern_aaai2024_amd.build", fromlist=["SOURCES"]).SOURCES


def test_item_argument_errors_name_the_function():
    from fashionern_aaai2024_amd import _lib
    lib = _lib.load()
    p = 0x1000                                           # never dereferenced: every call below is refused before any HIP call
    topk = lambda ctx=p, k=5, g=5, items=p, g32=p, g16=None, d=128, n=10: lib.fern_sim_topk_items(      # noqa: E731
        ctx, p, g32, g16, 2, n, d, k, items, g, p, p, p, 0, None, None, None, None, None)
    assert topk(ctx=None) == -1 and b"fern_sim_topk_items: ctx is NULL" in lib.fern_last_error()
    for k in (0, 1025):
        assert topk(k=k) == -1 and b"fern_sim_topk_items: need 1<=K<=1024" in lib.fern_last_error()
    assert topk(g=0) == -1 and b"fern_sim_topk_items: need G >= 1" in lib.fern_last_error()
    assert topk(items=None) == -1 and b"fern_sim_topk_items: items is NULL" in lib.fern_last_error()
    assert topk(g32=None) == -1 and b"gallery and gallery_bf16 are both NULL" in lib.fern_last_error()
    assert topk(d=48) == -1 and b"the fp32 form needs D % 32 == 0" in lib.fern_last_error()
    assert topk(g32=None, g16=p, d=640 + 32) == -1 and b"a bf16-only gallery needs D % 64 == 0, D <= 768" in lib.fern_last_error()
    assert topk(g=150_000_000) == -1 and b"exceed the 1.1 GB workspace budget" in lib.fern_last_error()      # one query's table
    assert topk(n=300_000_000) == -1 and b"exceed the 1.1 GB workspace budget" in lib.fern_last_error()      # one query's score row
    for name in ("fern_item_rank", "fern_item_keys", "fern_item_count"):
        call = lambda ctx=p, g=5, m=1, items=p, fn=getattr(lib, name): fn(ctx, p, p, None, 2, 10, 128, items, g, p, m, 0, None, p, None, None, None, None)      # noqa: E731
        assert call(ctx=None) == -1 and f"{name}: ctx is NULL".encode() in lib.fern_last_error()
        assert call(g=0) == -1 and f"{name}: need G >= 1".encode() in lib.fern_last_error()
        assert call(m=0) == -1 and f"{name}: need m >= 1".encode() in lib.fern_last_error()
        assert call(items=None) == -1 and f"{name}: items is NULL".encode() in lib.fern_last_error()


# ---- ItemMap ---------------------------------------------------------------------------------------------------------------------
def test_item_map_validation_rows_and_default_count():
    from fashionern_aaai2024_amd.engine import ItemMap
    m = ItemMap(torch.tensor([4, 4, 0, 9, -1, 2]))
    assert m.items.dtype == torch.int32 and m.n_items == 10              # max id + 1, computed once at construction
    assert ItemMap(torch.tensor([4, 4, 0], dtype=torch.int32), 3).n_items == 3      # a smaller count is allowed: id 4 then belongs to no item
    assert ItemMap(torch.zeros(0, dtype=torch.int32)).n_items == 1
    sl = m.rows(1, 4)
    assert sl.items.tolist() == [4, 0, 9] and sl.n_items == 10            # a shard: global ids, the global count
    assert m.resolve(6, "cpu").tolist() == [4, 4, 0, 9, -1, 2] and m.resolve(6, "cpu").is_contiguous()
    with pytest.raises(ValueError, match="gallery has 7 rows"):
        m.resolve(7, "cpu")
    with pytest.raises(ValueError, match="integer"):
        ItemMap(torch.zeros(3))
    with pytest.raises(ValueError, match=r"\[N\]"):
        ItemMap(torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        ItemMap(torch.tensor([1 << 31]))
    with pytest.raises(ValueError, match="n_items"):
        ItemMap(torch.tensor([0, 1]), 0)


# ---- the oracle itself, on a list small enough to write down -------------------------------------------------------------------------
def _handmade():
    """Seven rows, four names.  Query 0 scores the rows 7 6 5 4 3 2 1 (in row order), query 1 scores them 1 2 3 7 4 5 6."""
    names = ["a", "a", "a", "b", "c", "c", "d"]
    gallery = torch.zeros(7, 32)
    gallery[:, 0] = torch.tensor([7., 6., 5., 4., 3., 2., 1.]) / 8
    gallery[:, 1] = torch.tensor([1., 2., 3., 7., 4., 5., 6.]) / 8
    q = torch.zeros(2, 32)
    q[0, 0] = q[1, 1] = 1.0
    return names, gallery, q


def test_oracle_restates_the_definition():
    import items_oracle as io
    from fashionern_aaai2024_amd.engine import ItemMap, RowFilter
    names, gallery, q = _handmade()
    eng = io.items_oracle()()
    items = ItemMap(torch.tensor([0, 0, 0, 1, 2, 2, 3]))
    s, i, t = eng.sim_topk_items(q, gallery, items, 5)
    assert i.tolist() == [[0, 3, 4, 6, -1], [3, 6, 5, 2, -1]] and t.tolist() == [[0, 1, 2, 3, -1], [1, 3, 2, 0, -1]]
    assert s[0].tolist()[:4] == [7 / 8, 4 / 8, 3 / 8, 1 / 8] and s[0, 4] == float("-inf")
    assert eng.item_rank_of(q, gallery, items, torch.tensor([[3, 0, 4], [0, 1, -1]])).tolist() == [[3, 0, -1], [3, 0, -1]]
    # the excluded row hands its item to the next row; a filtered-out item takes no place; idx_offset moves indices only
    s, i, t = eng.sim_topk_items(q, gallery, items, 4, idx_offset=100, exclude_idx=torch.tensor([100, 103]),
                                 row_filter=RowFilter(torch.tensor([0, 0, 0, 1, 0, 0, 0]), torch.tensor([0, 1]), torch.tensor([0, 0])))
    assert i.tolist() == [[101, 103, 104, 106], [106, 105, 102, -1]] and t.tolist() == [[0, 1, 2, 3], [3, 2, 0, -1]]


# ---- run/_common.recalls_items -----------------------------------------------------------------------------------------------------
def test_recalls_items_counts_items_where_the_row_metrics_count_rows():
    import items_oracle as io
    from fashionern_aaai2024_amd.run import _common
    names, gallery, q = _handmade()
    model = types.SimpleNamespace(engine=io.items_oracle()())
    rows, distinct = _common.items_of_names(names)
    assert rows.tolist() == [0, 0, 0, 1, 2, 2, 3] and distinct == ["a", "b", "c", "d"]
    predicted = torch.cat([q, q[:1]])
    targets = ["b", "a", "nowhere"]
    # row level: "b" sits behind the three rows of "a" (place 3); query 1's best "a" row is behind b, d, c, c (place 4 of 0-based rows)
    row_places = _common.target_ranks(model, predicted, gallery, np.array([[3, -1, -1], [0, 1, 2], [-1, -1, -1]]))
    assert np.where(row_places >= 0, row_places, 99).min(axis=1).tolist() == [3, 4, 99]
    # item level: "a" is ONE item in front of "b" (place 1); b, d, c are three items in front of "a" (place 3)
    res = _common.recalls_items(model, predicted, gallery, names, targets, (1, 2, 4))
    assert res["recall@1"] == 0.0 and res["recall@2"] == _common._pct(1, 3) and res["recall@4"] == _common._pct(2, 3)
    assert res["median_rank"] == 3.0                         # places 2 and 4, counted from 1, over the queries that have a target item
    row = _common.retrieval_metrics(row_places, (1, 2, 4))
    assert row["recall@2"] == 0.0 and row["recall@4"] == _common._pct(1, 3) and row["median_rank"] == 4.5


def test_item_level_flag_is_offered_by_the_200k_driver_only():
    from fashionern_aaai2024_amd.run._cli import build_parser
    assert build_parser("200k").parse_args(["--item-level"]).item_level is True
    assert build_parser("200k").parse_args([]).item_level is False
    with pytest.raises(SystemExit):
        build_parser("fiq").parse_args(["--item-level"])


def test_200k_item_metrics_on_the_duplicate_name_fixture():
    """The 200k fixture of the harness tests (duplicate gallery names): item-level recalls can only be >= the any-hit row recalls, and the
    item places are the oracle's."""
    import items_oracle as io
    import synthetic_data as sdata
    from fashionern_aaai2024_amd import synth
    from fashionern_aaai2024_amd.model import ERN
    from fashionern_aaai2024_amd.run import rank_metrics, test_200k
    from fashionern_aaai2024_amd.tokenizer import register_tokenizer
    from fashionern_aaai2024_amd.utils import extract_index_features
    register_tokenizer("stub", sdata.stub_tokenizer)
    d = META["d"]
    clip = sdata.StubCLIP(d).eval()
    model = ERN(clip, d, "cpu", engine=io.items_oracle()())
    model.load_state_dict(synth.fusion_state_dict(d, seed=META["fusion_seed"]))
    gal = sdata.Gallery(META["n"], d, seed=META["gallery_seed"], dup_names=True)
    rel = sdata.RelativeDataset(gal, META["q"], "200k", seed=META["relative_seed"])
    feats, names, local = extract_index_features(sdata.ClassicDataset(gal), clip, 13, "cpu", d, num_workers=0)
    row = test_200k.compute_200k_val_metrics(rel, clip, feats, local, names, model, "cpu", d, META["batch_size"], 0, "stub")
    item = rank_metrics.compute_200k_item_metrics(rel, clip, feats, local, names, model, "cpu", d, META["batch_size"], 0, "stub")
    assert list(row) == META["recalls"]["200k"]
    assert len(set(names)) < len(names)
    assert item["recall@10"] >= row[0] and item["recall@50"] >= row[1] and 1.0 <= item["median_rank"] <= len(set(names))


# ---- worlds of two and three over gloo ---------------------------------------------------------------------------------------------
def _sharded_case():
    """Operands in {-1, 0, 1} / 8: every dot product is exact in fp32 in any summation order, so a shard's scores are the whole gallery's
    bit for bit (and ties abound).  702 rows = 18 blocks of 39 rows, every block four items of 1, 5, 13 and 20 rows: the shard boundaries
    of two ranks (351) and of three (234, 468) fall between items.  Ids ascend with the rows; every 17th row belongs to no item; ids
    72 .. 79 own no row.  `split`: runs of 40 rows, which straddle every one of those boundaries."""
    from fashionern_aaai2024_amd.engine import ItemMap, RowFilter
    n, d, b = 702, 32, 6
    g = torch.Generator().manual_seed(5)
    gallery = torch.randint(-1, 2, (n, d), generator=g).float() / 8
    q = torch.randint(-1, 2, (b, d), generator=g).float() / 8
    ids = np.repeat(np.arange(72), [1, 5, 13, 20] * 18)
    ids[3::17] = -1
    rows = torch.arange(n)
    tags = ((rows % 3) | ((rows % 7 != 0).long() << 2)).to(torch.int32)
    flt = (tags, torch.tensor([7, 7, 7, 4, 0, 1], dtype=torch.int32), torch.tensor([4, 5, 6, 4, 0, 2], dtype=torch.int32))
    targets = torch.tensor([[0, 35, 71], [36, 4, -1], [5, 40, 72], [71, 79, 8], [5, 36, 12], [65, 2, 80]], dtype=torch.int32)
    ex = torch.tensor([6, -1, 350, 699, 5, 400], dtype=torch.int32)
    return gallery, q, ItemMap(torch.from_numpy(ids), 80), ItemMap(torch.arange(n) // 40, 80), targets, ex, flt, RowFilter


def _worker(rank, world, out_dir):
    import items_oracle as io
    from fashionern_aaai2024_amd import distributed as fd
    gallery, q, items, split, targets, ex, (tags, mask, value), RowFilter = _sharded_case()
    eng = io.items_oracle()()
    start, stop, _ = fd.shard_rows(gallery.shape[0], rank, world)
    shard, im, flt = gallery[start:stop], items.rows(start, stop), RowFilter(tags[start:stop], mask, value)
    out = {}
    out["s"], out["i"], out["t"] = fd.rank_items_sharded(eng, q, shard, start, im, 50)
    out["fs"], out["fi"], out["ft"] = fd.rank_items_sharded(eng, q, shard, start, im, 100, exclude_idx=ex, row_filter=flt)
    out["ranks"] = fd.item_rank_of_sharded(eng, q, shard, start, im, targets)
    out["franks"] = fd.item_rank_of_sharded(eng, q, shard, start, im, targets, exclude_idx=ex, row_filter=flt)
    out["flat"] = fd.item_rank_of_sharded(eng, q, shard, start, im, targets[:, 0])
    out["local"] = eng.item_rank_of(q, shard, im, targets, idx_offset=start)      # what this shard alone knows
    raised = []
    for fn, last in ((fd.rank_items_sharded, 50), (fd.item_rank_of_sharded, targets)):
        try:
            fn(eng, q, shard, start, split.rows(start, stop), last)
            raised.append(0)
        except ValueError as e:
            raised.append(int("every item's rows inside one shard" in str(e)))
    out["raised"] = torch.tensor(raised)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), **{k: v.numpy() for k, v in out.items()})


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_item_ranking_equals_the_unsharded_result(tmp_path, world):
    import items_oracle as io
    gloo.spawn(world, _worker, str(tmp_path))
    gallery, q, items, split, targets, ex, (tags, mask, value), RowFilter = _sharded_case()
    eng = io.items_oracle()()
    flt = RowFilter(tags, mask, value)
    want = dict(zip("sit", eng.sim_topk_items(q, gallery, items, 50)))
    want.update(zip(("fs", "fi", "ft"), eng.sim_topk_items(q, gallery, items, 100, exclude_idx=ex, row_filter=flt)))
    want["ranks"] = eng.item_rank_of(q, gallery, items, targets)
    want["franks"] = eng.item_rank_of(q, gallery, items, targets, exclude_idx=ex, row_filter=flt)
    want["flat"] = want["ranks"][:, 0]
    ranks = want["ranks"].numpy()
    none = np.zeros(ranks.shape, dtype=bool)
    none[2, 2] = none[3, 1] = none[5, 2] = none[1, 2] = True      # 72, 79: items without rows; 80, -1: no item
    assert (ranks[none] == -1).all() and (ranks[~none] >= 0).all()
    held = np.unique(items.items.numpy()[items.items.numpy() >= 0]).size
    assert (want["ft"][5] == -1).all() and (want["franks"][5] == -1).all() and (want["ft"][4] >= 0).sum() == held
    local = []
    for rank in range(world):
        got = np.load(tmp_path / f"r{rank}.npz")
        for k, w in want.items():
            assert np.array_equal(got[k], w.numpy()), (rank, k)
        assert got["raised"].tolist() == [1, 1]              # an item that straddles a shard boundary is refused on every rank
        local.append(got["local"])
    # a shard that does not own a target item knows nothing of it (-1), yet its items are counted: the places are not the owner's alone
    owners = (np.stack(local) >= 0).sum(axis=0)
    assert (owners[ranks >= 0] == 1).all() and (owners[ranks < 0] == 0).all()
    own_place = np.stack(local).max(axis=0)
    assert (ranks >= own_place).all() and (ranks > own_place).any()


def test_sharded_item_helpers_make_no_collective_in_a_world_of_one():
    import items_oracle as io
    from fashionern_aaai2024_amd import distributed as fd
    assert not (dist.is_available() and dist.is_initialized())
    gallery, q, items, split, targets, ex, (tags, mask, value), RowFilter = _sharded_case()
    eng = io.items_oracle()()
    got = fd.rank_items_sharded(eng, q, gallery, 0, items, 50, exclude_idx=ex)
    assert all(torch.equal(a, b) for a, b in zip(got, eng.sim_topk_items(q, gallery, items, 50, exclude_idx=ex)))
    assert torch.equal(fd.item_rank_of_sharded(eng, q, gallery, 0, split, targets), eng.item_rank_of(q, gallery, split, targets))

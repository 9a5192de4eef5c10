"""Live gallery without a GPU: the three C ABI entry points (header, library, ctypes table, argument checks), `SlotTable`'s bookkeeping,
the row-filter composition with the store's live bit, `distributed.route_rows` and the drivers' --incremental-index flag."""
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def test_live_entry_points_are_declared_exported_and_typed():
    from fashionern_aaai2024_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "fern.h")).read()
    lib = _lib.load()
    for name, nargs in (("fern_gallery_upsert", 12), ("fern_gallery_move", 11), ("fern_scatter_u32", 7)):
        assert re.search(rf"FERN_API int {name}\(", header)
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert lib.fern_abi_version() == 3 and "#define FERN_ABI_VERSION 3" in header
    assert "live.hip" in build.SOURCES and "row_ops.h" in build.HEADERS
    for phrase in ("ORDERING CONTRACT", "meta is NOT reset", "DISJOINT", "Duplicate slots within one call"):
        assert phrase in header, phrase


def test_live_argument_errors_name_the_function():
    from fashionern_aaai2024_amd import _lib
    lib = _lib.load()
    p = 0x1000                                           # never dereferenced: every call below is refused before any HIP call
    err = lib.fern_last_error

    def upsert(ctx=p, ld=64, g=p, gb=p, meta=p, d=64, m=3, rows=p, normalize=0):
        return lib.fern_gallery_upsert(ctx, rows, ld, p, m, g, gb, meta, 100, d, normalize, None)
    assert upsert(ctx=None) == -1 and b"fern_gallery_upsert: ctx is NULL" in err()
    assert upsert(ld=60) == -1 and b"fern_gallery_upsert: need ld >= D" in err()
    assert upsert(ld=66) == -1 and b"fern_gallery_upsert: need ld >= D and ld % 4 == 0" in err()
    assert upsert(d=62, ld=64) == -1 and b"fern_gallery_upsert: D must be a multiple of 4" in err()
    assert upsert(g=None, gb=None, meta=None) == -1 and b"fern_gallery_upsert: give gallery, gallery_bf16 or both" in err()
    assert upsert(gb=None) == -1 and b"fern_gallery_upsert: meta belongs to the prepared form" in err()
    assert upsert(g=None) == -1 and b"fern_gallery_upsert: meta belongs to the prepared form" in err()
    assert upsert(rows=None) == -1 and b"fern_gallery_upsert: bad argument" in err()
    assert upsert(m=-1) == -1 and b"fern_gallery_upsert: bad argument" in err()
    assert upsert(d=1284, ld=1284, normalize=1) == -1 and b"fern_gallery_upsert: normalize needs D <= 1280" in err()

    def move(ctx=p, g=p, gb=p, d=64, m=3, src=p):
        return lib.fern_gallery_move(ctx, src, p, m, g, gb, None, None, 100, d, None)
    assert move(ctx=None) == -1 and b"fern_gallery_move: ctx is NULL" in err()
    assert move(g=None, gb=None) == -1 and b"fern_gallery_move: give gallery, gallery_bf16 or both" in err()
    assert move(d=6) == -1 and b"fern_gallery_move: D must be a multiple of 4" in err()
    assert move(src=None) == -1 and b"fern_gallery_move: bad argument" in err()

    def scatter(ctx=p, src=p, dst=p, m=3):
        return lib.fern_scatter_u32(ctx, src, p, m, dst, 100, None)
    assert scatter(ctx=None) == -1 and b"fern_scatter_u32: ctx is NULL" in err()
    assert scatter(dst=None) == -1 and b"fern_scatter_u32: bad argument" in err()
    assert scatter(m=-2) == -1 and b"fern_scatter_u32: bad argument" in err()


def test_the_package_exports_the_host_classes():
    import fashionern_aaai2024_amd as pkg
    from fashionern_aaai2024_amd import live_gallery
    assert pkg.LiveGallery is live_gallery.LiveGallery and pkg.SlotTable is live_gallery.SlotTable
    with pytest.raises(AttributeError):
        pkg.no_such_name


# ---- SlotTable -------------------------------------------------------------------------------------------------------------------
def test_slot_table_hands_out_the_lowest_free_slot_first():
    from fashionern_aaai2024_amd.live_gallery import SlotTable
    t = SlotTable(10)
    assert t.allocate(4).tolist() == [0, 1, 2, 3] and t.allocate(0).tolist() == [] and (t.n, t.n_live) == (4, 4)
    t.release([2, 0])
    assert (t.n, t.n_live) == (4, 2) and t.is_live([0, 1, 2, 3]).tolist() == [False, True, False, True]
    got = t.allocate(4)                                  # the two holes, lowest first, before fresh slots
    assert got.dtype == np.int32 and got.tolist() == [0, 2, 4, 5] and (t.n, t.n_live) == (6, 6)
    t.release([5, 1, 3])
    assert t.allocate(1).tolist() == [1] and t.allocate(2).tolist() == [3, 5] and t.live_slots().tolist() == list(range(6))


def test_a_full_table_raises_and_stays_as_it_was():
    from fashionern_aaai2024_amd.live_gallery import SlotTable
    t = SlotTable(5)
    t.allocate(4)
    t.release([1])
    before = (t.n, t.n_live, t.live_slots().tolist())
    with pytest.raises(RuntimeError, match="full"):
        t.allocate(3)                                    # two are free, three are wanted: nothing is handed out
    assert (t.n, t.n_live, t.live_slots().tolist()) == before
    assert t.allocate(2).tolist() == [1, 4]
    with pytest.raises(RuntimeError, match="full"):
        t.allocate(1)


def test_slots_that_are_not_live_and_duplicates_raise_and_change_nothing():
    from fashionern_aaai2024_amd.live_gallery import SlotTable
    t = SlotTable(8)
    t.allocate(5)
    t.release([3])
    before = (t.n, t.n_live, t.live_slots().tolist())
    with pytest.raises(KeyError, match="slot 3 is not live"):
        t.release([0, 3])
    with pytest.raises(KeyError, match="slot 6 is not live"):
        t.check_live([6])
    with pytest.raises(ValueError, match="given twice"):
        t.release([1, 1])
    with pytest.raises(ValueError, match="given twice"):
        t.check_live([2, 4, 2])
    with pytest.raises(IndexError):
        t.release([8])
    with pytest.raises(IndexError):
        t.check_live([-1])
    assert (t.n, t.n_live, t.live_slots().tolist()) == before
    assert t.check_live([4, 0]).tolist() == [4, 0]


def test_plan_compact_moves_the_highest_live_slots_into_the_lowest_holes():
    from fashionern_aaai2024_amd.live_gallery import SlotTable
    t = SlotTable(16)
    t.allocate(10)
    t.release([1, 4, 5, 8])                              # live: 0 2 3 6 7 9 -> n_live 6
    src, dst = t.plan_compact()
    assert src.tolist() == [9, 7, 6] and dst.tolist() == [1, 4, 5]
    assert not set(src.tolist()) & set(dst.tolist())
    assert t.n == 10 and t.live_slots().tolist() == [0, 2, 3, 6, 7, 9]      # a plan changes nothing
    t.apply_compact(src, dst)
    assert (t.n, t.n_live) == (6, 6) and t.live_slots().tolist() == [0, 1, 2, 3, 4, 5]
    assert t.allocate(2).tolist() == [6, 7]              # the old holes above n_live are ordinary free slots again
    src, dst = t.plan_compact()
    assert src.size == 0 and dst.size == 0
    with pytest.raises(ValueError):
        t.apply_compact([7], [9])                        # not a plan of this table
    rng = np.random.default_rng(0)
    for _ in range(20):                                  # random churn: the plan always leaves the live rows as [0, n_live)
        t = SlotTable(64)
        t.allocate(int(rng.integers(1, 65)))
        live = t.live_slots()
        t.release(rng.choice(live, size=int(rng.integers(0, live.size + 1)), replace=False))
        src, dst = t.plan_compact()
        assert (np.diff(src) < 0).all() and (np.diff(dst) > 0).all() and not set(src.tolist()) & set(dst.tolist())
        t.apply_compact(src, dst)
        assert t.live_slots().tolist() == list(range(t.n_live)) and t.n == t.n_live


def test_slot_offset_makes_every_slot_global():
    from fashionern_aaai2024_amd.live_gallery import SlotTable
    t = SlotTable(6, slot_offset=1000)
    assert t.allocate(4).tolist() == [1000, 1001, 1002, 1003]
    t.release([1001])
    with pytest.raises(IndexError):
        t.release([1])                                   # a local index is not a slot of this table
    assert t.allocate(2).tolist() == [1001, 1004]
    t.release([1000, 1002])
    src, dst = t.plan_compact()
    assert src.tolist() == [1004, 1003] and dst.tolist() == [1000, 1002] and t.n == 5
    with pytest.raises(ValueError):
        SlotTable(10, slot_offset=(1 << 31) - 5)


# ---- the live bit ----------------------------------------------------------------------------------------------------------------
def test_filter_composition_adds_the_live_bit_and_refuses_a_collision():
    from fashionern_aaai2024_amd.engine import RowFilter
    from fashionern_aaai2024_amd.live_gallery import check_user_tags, compose_filter
    live = 1 << 31
    assert compose_filter(0, 0, 31) == (live, live)
    assert compose_filter(3, 2, 31) == (live | 3, live | 2)
    m, v = compose_filter(torch.tensor([3, 0, 0x7FFFFFFC]), torch.tensor([1, 0, 8]), 31)
    assert m.tolist() == [live | 3, live, live | 0x7FFFFFFC] and v.tolist() == [live | 1, live, live | 8]
    m, v = compose_filter(torch.tensor([3, 12], dtype=torch.int32), 1, 4)      # another bit; tensor and scalar mixed
    assert m.tolist() == [19, 28] and v == 17
    for mask, value in ((live, 0), (0, live), (-1, 0), (torch.tensor([1, live]), 0), (0, torch.tensor([-(1 << 31)], dtype=torch.int32))):
        with pytest.raises(ValueError, match="live bit"):
            compose_filter(mask, value, 31)
    with pytest.raises(ValueError, match="live bit"):
        compose_filter(16, 0, 4)
    # the composed filter does what it says: live rows that pass the caller's filter, and only those
    tags = torch.tensor([live | 1, 1, live | 2, 2, live | 1, 0], dtype=torch.int64)
    f = RowFilter(tags, *compose_filter(3, 1, 31))
    t, mk, vl = f.resolve(1, 6, "cpu")
    assert ((t & mk[0]) == vl[0]).tolist() == [True, False, False, False, True, False]
    f = RowFilter(tags, *compose_filter(0, 0, 31))
    t, mk, vl = f.resolve(1, 6, "cpu")
    assert ((t & mk[0]) == vl[0]).tolist() == [True, False, True, False, True, False]
    assert check_user_tags([0, 5, 0x7FFFFFFF], 31).tolist() == [0, 5, 0x7FFFFFFF]
    assert check_user_tags(np.array([-2], dtype=np.int32), 0).tolist() == [0xFFFFFFFE]
    for bad in ([1, live], np.array([-1], dtype=np.int32)):
        with pytest.raises(ValueError, match="live bit"):
            check_user_tags(bad, 31)
    with pytest.raises(ValueError):
        check_user_tags([1 << 32], 31)


# ---- sharding --------------------------------------------------------------------------------------------------------------------
def test_route_rows_partitions_an_update_by_owning_shard():
    from fashionern_aaai2024_amd.distributed import route_rows, shard_rows
    n, world = 1001, 3
    bounds = [shard_rows(n, r, world)[0] for r in range(world)] + [n]
    assert bounds == [0, 334, 668, 1001]
    slots = np.array([700, 0, 333, 334, 1000, 667, 668, 5], dtype=np.int32)
    idx = route_rows(slots, bounds)
    assert [i.tolist() for i in idx] == [[1, 2, 7], [3, 5], [0, 4, 6]]
    assert sorted(np.concatenate(idx).tolist()) == list(range(slots.size))
    for r, i in enumerate(idx):
        assert ((slots[i] >= bounds[r]) & (slots[i] < bounds[r + 1])).all()
    assert [i.tolist() for i in route_rows([], bounds)] == [[], [], []]
    assert [i.tolist() for i in route_rows([3, 4], [0, 0, 10])] == [[], [0, 1]]        # an empty shard owns nothing
    for bad in ([1001], [-1]):
        with pytest.raises(IndexError):
            route_rows(bad, bounds)
    with pytest.raises(ValueError):
        route_rows([1], [0, 10, 5])


# ---- driver ----------------------------------------------------------------------------------------------------------------------
def test_incremental_index_is_offered_where_rank_metrics_is_and_refused_for_several_ranks(monkeypatch):
    from fashionern_aaai2024_amd import distributed as fd
    from fashionern_aaai2024_amd.run import _common
    from fashionern_aaai2024_amd.run._cli import build_parser
    for kind in ("fiq", "val", "cirr", "shoes", "200k"):
        p = build_parser(kind)
        assert p.parse_args(["--rank-metrics"]).rank_metrics is True
        assert p.parse_args([]).incremental_index == 0
        assert p.parse_args(["--incremental-index", "64"]).incremental_index == 64
    assert _common._incremental_rows is None
    with _common.incremental_index(64):
        assert _common._incremental_rows == 64
        with _common.incremental_index(None):
            assert _common._incremental_rows is None
        assert _common._incremental_rows == 64
    assert _common._incremental_rows is None
    monkeypatch.setattr(fd, "world_info", lambda: (1, 2))
    with pytest.raises(RuntimeError, match="world > 1"):
        with _common.incremental_index(64):
            pass
    assert _common._incremental_rows is None
    with _common.incremental_index(0):                   # nothing asked for: nothing to refuse
        assert _common._incremental_rows is None

"""Filtered ranking without a GPU: the C ABI entry points fern_sim_topk_filtered / fern_rank_count_filtered (header, library, ctypes
table, argument checks), `RowFilter`'s shape rules, the merged-gallery path of the fiq harness on a filtered subclass of the TEST-ONLY
OracleEngine (tests/filtered_oracle.py) against the recall tuples captured from the imported reference harness
(tests/golden/harness.json), and the filtered `distributed.rank_sharded` / `rank_of_sharded` over gloo."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist

import gloo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
META = json.load(open(os.path.join(HERE, "golden", "harness.json")))


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def test_filtered_entry_points_are_declared_exported_and_typed():
    from fashionern_aaai2024_amd import _lib
    header = open(os.path.join(ROOT, "include", "fern.h")).read()
    lib = _lib.load()
    for name, nargs in (("fern_sim_topk_filtered", 17), ("fern_rank_count_filtered", 16)):
        assert re.search(rf"FERN_API int {name}\(", header)
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name.replace("filtered", "deep").replace("rank_count_deep", "rank_count")][1]) + 3
    assert "run/test/test_fiq.py:157-177" in header and "run/test/test_cirr.py:63-66" in header
    assert "(tags[n] & mask[b]) == value[b]" in header
    assert lib.fern_abi_version() == 3 and "#define FERN_ABI_VERSION 3" in header


def test_filtered_argument_errors_name_the_function():
    from fashionern_aaai2024_amd import _lib
    lib = _lib.load()
    p = 0x1000                                           # never dereferenced: every call below is refused before any HIP call
    topk = lambda ctx, k, tags: lib.fern_sim_topk_filtered(ctx, p, p, None, None, 2, 10, 64, k, p, p, 0, None, tags, p, p, None)      # noqa: E731
    assert topk(None, 5, p) == -1
    assert b"fern_sim_topk_filtered: ctx is NULL" in lib.fern_last_error()
    assert topk(p, 5, None) == -1
    assert b"fern_sim_topk_filtered: tags is NULL" in lib.fern_last_error()
    for k in (0, 1025):
        assert topk(p, k, p) == -1
        assert b"fern_sim_topk_filtered: need 1<=K<=1024" in lib.fern_last_error()
    count = lambda ctx, tags: lib.fern_rank_count_filtered(ctx, p, p, None, 2, 10, 64, p, 1, 0, None, p, tags, p, p, None)      # noqa: E731
    assert count(None, p) == -1
    assert b"fern_rank_count_filtered: ctx is NULL" in lib.fern_last_error()
    assert count(p, None) == -1
    assert b"fern_rank_count_filtered: tags is NULL" in lib.fern_last_error()


def test_every_ranking_entry_point_refuses_too_many_rows_and_a_bad_width_by_name():
    """One argument check serves all twelve ranking entry points: each refuses N = 0x7FFFFFF1 (one row past the int32 index limit) and
    a width its gallery form does not take (30 for fp32 rows, 96 for a bf16-only gallery) with FERN_ERR_ARG and its own name -- with a
    NULL context, and with a context that is never dereferenced, where the message must be the row limit's or the width rule's own
    (the width is judged first), not that of some earlier check."""
    from fashionern_aaai2024_amd import _lib
    lib = _lib.load()
    p = 0x1000                                           # never dereferenced: every call below is refused before any HIP call
    # name -> call(ctx, g32, g16, n, d); the forms each takes: "fp32", "bf16" (bf16-only gallery) or both
    entry = {
        "fern_sim_topk": (("fp32",), lambda c, g32, g16, n, d: lib.fern_sim_topk(c, p, g32, 2, n, d, 5, p, p, 0, None, None)),
        "fern_sim_topk_bf16": (("bf16",), lambda c, g32, g16, n, d: lib.fern_sim_topk_bf16(c, p, g16, 2, n, d, 5, p, p, 0, None, None)),
        "fern_sim_topk_prefiltered": (("fp32",), lambda c, g32, g16, n, d: lib.fern_sim_topk_prefiltered(c, p, g32, p, p, 2, n, d, 5, p, p, 0, None, None)),
        "fern_sim_topk_deep": (("fp32", "bf16"), lambda c, g32, g16, n, d: lib.fern_sim_topk_deep(c, p, g32, g16, None, 2, n, d, 100, p, p, 0, None, None)),
        "fern_sim_topk_filtered": (("fp32", "bf16"), lambda c, g32, g16, n, d: lib.fern_sim_topk_filtered(c, p, g32, g16, None, 2, n, d, 100, p, p, 0, None, p, p, p, None)),
        "fern_sim_topk_items": (("fp32", "bf16"), lambda c, g32, g16, n, d: lib.fern_sim_topk_items(c, p, g32, g16, 2, n, d, 5, p, 5, p, p, p, 0, None, None, None, None, None)),
        "fern_rank_keys": (("fp32", "bf16"), lambda c, g32, g16, n, d: lib.fern_rank_keys(c, p, g32, g16, 2, n, d, p, 1, 0, p, None)),
        "fern_rank_count": (("fp32", "bf16"), lambda c, g32, g16, n, d: lib.fern_rank_count(c, p, g32, g16, 2, n, d, p, 1, 0, None, p, None)),
        "fern_rank_count_filtered": (("fp32", "bf16"), lambda c, g32, g16, n, d: lib.fern_rank_count_filtered(c, p, g32, g16, 2, n, d, p, 1, 0, None, p, p, p, p, None)),
    }
    for name in ("fern_item_rank", "fern_item_keys", "fern_item_count"):
        entry[name] = (("fp32", "bf16"), lambda c, g32, g16, n, d, fn=getattr(lib, name): fn(c, p, g32, g16, 2, n, d, p, 5, p, 1, 0, None, p, None, None, None, None))
    assert len(entry) == 12
    too_many = b"N too large for int32 indices"
    for name, (forms, call) in entry.items():
        for form in forms:
            g32, g16, good, bad, width = (p, None, 64, 30, b"D % 32 == 0") if form == "fp32" else (None, p, 64, 96, b"D % 64 == 0")
            for n, d, why in ((0x7FFFFFF1, good, too_many), (10, bad, width), (0x7FFFFFF1, bad, width)):
                assert call(None, g32, g16, n, d) == -1, (name, form, n, d)
                assert name.encode() + b":" in lib.fern_last_error(), (name, form, n, d, lib.fern_last_error())
                assert call(p, g32, g16, n, d) == -1, (name, form, n, d)
                assert name.encode() + b":" in lib.fern_last_error() and why in lib.fern_last_error(), (name, form, n, d, lib.fern_last_error())
            assert call(None, g32, g16, 10, good) == -1 and name.encode() + b": ctx is NULL" in lib.fern_last_error()      # nothing else to refuse


def test_a_mis_shaped_exclude_idx_is_refused_by_every_ranking_method():
    """Every ranking method of FernEngine converts `exclude_idx` through `_exclude`: a [B + 1] tensor raises ValueError before the
    library is reached -- `sim_topk_bf16` included, which used to hand it to the kernel unchecked."""
    from fashionern_aaai2024_amd.engine import FernEngine, ItemMap

    class Hostless(FernEngine):
        """No context and no library: a call that gets past the argument handling fails with AttributeError, not ValueError."""
        def __init__(self):
            self.device = torch.device("cpu")

        def _gallery_forms(self, q, gallery, bf16_ok=True):
            if bf16_ok and isinstance(gallery, torch.Tensor) and gallery.dtype == torch.bfloat16:
                return self._f32(q), None, gallery, None          # a host tensor stands in for the device tensor the engine asks for
            return super()._gallery_forms(q, gallery, bf16_ok)

    eng = Hostless()
    b, n, d = 3, 7, 64
    q, g = torch.zeros(b, d), torch.zeros(n, d)
    assert eng._exclude(None, b) is None and eng._exclude([1, 2, 3], b).dtype == torch.int32
    items, t = ItemMap(torch.zeros(n, dtype=torch.int32), 1), torch.zeros(b, dtype=torch.int32)
    keys = torch.ones(b, 1, dtype=torch.int64)
    for bad in (torch.zeros(b + 1, dtype=torch.int32), torch.zeros(b, 1, dtype=torch.int32)):
        for call in (lambda: eng._exclude(bad, b),
                     lambda: eng.sim_topk(q, g, 5, exclude_idx=bad),
                     lambda: eng.sim_topk_bf16(q, g.bfloat16(), 5, exclude_idx=bad),
                     lambda: eng.sim_topk_deep(q, g, 100, exclude_idx=bad),
                     lambda: eng.sim_topk_deep(q, g.bfloat16(), 100, exclude_idx=bad),
                     lambda: eng.rank_count(q, g, keys, exclude_idx=bad),
                     lambda: eng.sim_topk_items(q, g, items, 5, exclude_idx=bad),
                     lambda: eng.item_rank_of(q, g, items, t, exclude_idx=bad)):
            with pytest.raises(ValueError, match=r"exclude_idx must be \[B\]"):
                call()
    with pytest.raises(AttributeError):                      # a well-shaped one goes on to the library
        eng.sim_topk_bf16(q, g.bfloat16(), 5, exclude_idx=torch.zeros(b, dtype=torch.int32))


# ---- RowFilter -------------------------------------------------------------------------------------------------------------------
def test_row_filter_shape_checks_and_bit_forms():
    from fashionern_aaai2024_amd.engine import RowFilter
    tags = torch.arange(10, dtype=torch.int32)
    f = RowFilter(tags, 3, 1)                            # scalars broadcast
    t, m, v = f.resolve(4, 10, "cpu")
    assert t.dtype == m.dtype == v.dtype == torch.int32 and m.tolist() == [3] * 4 and v.tolist() == [1] * 4
    assert RowFilter(tags).resolve(2, 10, "cpu")[1].tolist() == [0, 0]          # the default accepts every row
    u = RowFilter(tags.to(torch.uint32), 0xFFFFFFFF, torch.tensor([0x80000000, 5], dtype=torch.uint32))      # uint32 and wide ints are bits
    _, m, v = u.resolve(2, 10, "cpu")
    assert m.tolist() == [-1, -1] and v.tolist() == [-(1 << 31), 5]
    assert RowFilter(tags, -1, 2).mask.item() == -1
    sl = RowFilter(tags, torch.tensor([1, 2, 3]), torch.tensor([4, 5, 6])).rows(1, 3)
    assert sl.mask.tolist() == [2, 3] and sl.value.tolist() == [5, 6] and sl.tags is not None
    with pytest.raises(ValueError, match="tags"):
        RowFilter(torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="integer"):
        RowFilter(torch.zeros(3))
    with pytest.raises(ValueError, match="32 bits"):
        RowFilter(tags, 1 << 32, 0)
    with pytest.raises(ValueError, match="same length"):
        RowFilter(tags, torch.tensor([1, 2]), torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="gallery has 11 rows"):
        f.resolve(4, 11, "cpu")
    with pytest.raises(ValueError, match="mask"):
        RowFilter(tags, torch.tensor([1, 2]), 0).resolve(3, 10, "cpu")


# ---- the merged-gallery harness on the filtered oracle ----------------------------------------------------------------------------
def _category(c, engine):
    """Category 0 is the fixture the golden recalls were captured on; 1 and 2 are further galleries of other sizes and seeds.  All three
    name their rows img00000, img00001, ...: names repeat across the categories."""
    import synthetic_data as sdata
    from fashionern_aaai2024_amd import synth
    from fashionern_aaai2024_amd.model import ERN
    from fashionern_aaai2024_amd.tokenizer import register_tokenizer
    from fashionern_aaai2024_amd.utils import extract_index_features
    register_tokenizer("stub", sdata.stub_tokenizer)
    d = META["d"]
    n, q, gseed, rseed = [(META["n"], META["q"], META["gallery_seed"], META["relative_seed"]), (150, 30, 21, 22), (260, 40, 31, 32)][c]
    clip = sdata.StubCLIP(d).eval()
    model = ERN(clip, d, "cpu", engine=engine)
    model.load_state_dict(synth.fusion_state_dict(d, seed=META["fusion_seed"]))
    gal = sdata.Gallery(n, d, seed=gseed)
    rel = sdata.RelativeDataset(gal, q, "fiq", seed=rseed)
    feats, names, local = extract_index_features(sdata.ClassicDataset(gal), clip, 13, "cpu", d, num_workers=0)
    return clip, model, rel, feats, names, local, d


def test_merged_gallery_reproduces_the_per_category_recalls():
    from filtered_oracle import filtered_oracle
    from fashionern_aaai2024_amd.run import _common, test_fiq
    eng = filtered_oracle()()
    feats, locals_, names, preds, targets, per = [], [], [], [], [], []
    for c in range(3):
        clip, model, rel, f, nm, lc, d = _category(c, eng)
        per.append(tuple(test_fiq.compute_fiq_val_metrics(rel, clip, f, lc, nm, model, "cpu", d, META["batch_size"], 0, "stub")))
        p, t = test_fiq.generate_fiq_val_predictions(clip, rel, model, nm, f, "cpu", d, META["batch_size"], 0, "stub")
        feats.append(f); locals_.append(lc); names.append(nm); preds.append(p); targets.append(t)
    assert list(per[0]) == META["recalls"]["fiq"]                  # the golden tuple, from the separate gallery ...
    all_f, all_l, tags, starts = _common.merge_galleries(feats, locals_)
    assert tags.dtype == torch.int32 and tags.tolist() == [0] * META["n"] + [1] * 150 + [2] * 260 and list(starts) == [0, 200, 350, 610]
    fused = _common.fuse_index(model, all_f, all_l, prepared=True)
    merged = _common.recalls_merged(model, preds, fused, tags, starts, names, targets, (10, 50))
    assert merged == per and list(merged[0]) == META["recalls"]["fiq"]      # ... and unchanged from the merged, filtered one
    # the filter is what does it: unfiltered, the merged gallery ranks other categories' rows into the lists
    top = _common._ranked(model, torch.cat(preds), fused, 50)
    cat_of_row = tags.numpy()[top]
    cat_of_query = np.repeat(np.arange(3), [p.shape[0] for p in preds])
    assert (cat_of_row != cat_of_query[:, None]).any()


def test_merged_gallery_flag_is_offered_by_the_fiq_and_val_drivers_only():
    from fashionern_aaai2024_amd.run._cli import build_parser
    assert build_parser("fiq").parse_args(["--merged-gallery"]).merged_gallery is True
    assert build_parser("val").parse_args([]).merged_gallery is False
    with pytest.raises(SystemExit):
        build_parser("cirr").parse_args(["--merged-gallery"])


def test_unfiltered_harness_calls_do_not_pass_the_keyword():
    """`_ranked` / `target_ranks` hand `row_filter` to the engine only when one is given: the plain OracleEngine does not know it."""
    from oracle_engine import OracleEngine
    from fashionern_aaai2024_amd.run import _common, test_fiq
    clip, model, rel, f, nm, lc, d = _category(0, OracleEngine())
    assert list(test_fiq.compute_fiq_val_metrics(rel, clip, f, lc, nm, model, "cpu", d, META["batch_size"], 0, "stub")) == META["recalls"]["fiq"]
    assert _common._filter_kw(None, 0, 5) == {}


# ---- world 2 over gloo -------------------------------------------------------------------------------------------------------------
def _sharded_case():
    """Operands in {-1, 0, 1} / 8: every dot product is exact in fp32 in any summation order, so a shard's scores are the whole
    gallery's bit for bit (and ties abound).  Ragged: 701 rows over two ranks are 351 + 350.  Tags: category = row % 3 in bits 0-1,
    a live bit (bit 2) cleared on every seventh row."""
    from fashionern_aaai2024_amd.engine import RowFilter
    n, d, b = 701, 32, 6
    g = torch.Generator().manual_seed(5)
    gallery = torch.randint(-1, 2, (n, d), generator=g).float() / 8
    q = torch.randint(-1, 2, (b, d), generator=g).float() / 8
    rows = torch.arange(n)
    tags = ((rows % 3) | ((rows % 7 != 0).long() << 2)).to(torch.int32)
    mask = torch.tensor([7, 7, 7, 4, 0, 1], dtype=torch.int32)
    value = torch.tensor([4, 5, 6, 4, 0, 2], dtype=torch.int32)       # three categories among the live rows; live; all; nothing
    targets = torch.tensor([[7, 351, 699], [352, 4, -1], [5, 401, 350], [700, 701, 8], [5, 352, 12], [650, 2, 351]], dtype=torch.int32)
    ex = torch.tensor([6, -1, 350, 699, 5, 400], dtype=torch.int32)
    return gallery, q, targets, ex, tags, mask, value, RowFilter


def _worker(rank, world, out_dir):
    from filtered_oracle import filtered_oracle
    from fashionern_aaai2024_amd import distributed as fd
    gallery, q, targets, ex, tags, mask, value, RowFilter = _sharded_case()
    eng = filtered_oracle()()
    start, stop, _ = fd.shard_rows(gallery.shape[0], rank, world)
    flt = RowFilter(tags[start:stop], mask, value)                 # tags shard with the rows
    ranks = fd.rank_of_sharded(eng, q, gallery[start:stop], start, targets, exclude_idx=ex, row_filter=flt)
    s, i = fd.rank_sharded(eng, q, gallery[start:stop], start, 50, exclude_idx=ex, row_filter=flt)
    s2, i2 = fd.rank_sharded(eng, q, gallery[start:stop], start, 200, row_filter=flt)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), ranks=ranks.numpy(), s=s.numpy(), i=i.numpy(), s2=s2.numpy(), i2=i2.numpy())


def test_filtered_sharded_ranking_equals_the_unsharded_result(tmp_path):
    from filtered_oracle import filtered_oracle
    gloo.spawn(2, _worker, str(tmp_path))
    gallery, q, targets, ex, tags, mask, value, RowFilter = _sharded_case()
    eng = filtered_oracle()()
    flt = RowFilter(tags, mask, value)
    ranks = eng.rank_of(q, gallery, targets, exclude_idx=ex, row_filter=flt).numpy()
    s, i = eng.sim_topk(q, gallery, 50, exclude_idx=ex, row_filter=flt)
    s2, i2 = eng.sim_topk(q, gallery, 200, row_filter=flt)
    assert (ranks >= 0).sum() >= 5 and (ranks[5] == -1).all() and (i[5] == -1).all() and (i[4] >= 0).all()
    assert ranks[0, 0] == -1 and ranks[0, 2] >= 0                   # query 0 wants live rows of category 0: row 7 is category 1, row 699 fits
    for rank in range(2):
        got = np.load(tmp_path / f"r{rank}.npz")
        assert np.array_equal(got["ranks"], ranks)
        assert np.array_equal(got["i"], i.numpy()) and np.array_equal(got["s"], s.numpy())
        assert np.array_equal(got["i2"], i2.numpy()) and np.array_equal(got["s2"], s2.numpy())


def test_filtered_sharded_helpers_make_no_collective_in_a_world_of_one():
    from filtered_oracle import filtered_oracle
    from fashionern_aaai2024_amd import distributed as fd
    assert not (dist.is_available() and dist.is_initialized())
    gallery, q, targets, ex, tags, mask, value, RowFilter = _sharded_case()
    eng = filtered_oracle()()
    flt = RowFilter(tags, mask, value)
    got = fd.rank_of_sharded(eng, q, gallery, 0, targets, exclude_idx=ex, row_filter=flt)
    assert np.array_equal(got.numpy(), eng.rank_of(q, gallery, targets, exclude_idx=ex, row_filter=flt).numpy())
    s, i = fd.rank_sharded(eng, q, gallery, 0, 50, row_filter=flt)
    assert torch.equal(i, eng.sim_topk(q, gallery, 50, row_filter=flt)[1])

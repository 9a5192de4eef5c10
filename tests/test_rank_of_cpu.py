"""Exact target ranks without a GPU: the C ABI entry points fern_rank_keys / fern_rank_count (header, library, ctypes table, argument
checks), the metric arithmetic of run/_common.retrieval_metrics, the rank-metric harness functions against the fixtures captured from
the imported reference harness (tests/golden/harness.json, the TEST-ONLY OracleEngine), and distributed.rank_of_sharded over gloo."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist

import gloo
from rank_oracle import RankOracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
META = json.load(open(os.path.join(GOLD, "harness.json")))
ARR = np.load(os.path.join(GOLD, "harness.npz"))


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def test_rank_entry_points_are_declared_exported_and_typed():
    from fashionern_aaai2024_amd import _lib
    header = open(os.path.join(ROOT, "include", "fern.h")).read()
    lib = _lib.load()
    for name, nargs in (("fern_rank_keys", 12), ("fern_rank_count", 13)):
        assert re.search(rf"FERN_API int {name}\(", header)
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert "run/test/test_fiq.py:49-60" in header
    assert lib.fern_abi_version() == 3


def test_rank_argument_errors_name_the_function():
    from fashionern_aaai2024_amd import _lib
    lib = _lib.load()
    p = 0x1000                                           # never dereferenced: every call below is refused before any HIP call
    assert lib.fern_rank_keys(None, p, p, None, 2, 10, 64, p, 1, 0, p, None) == -1
    assert b"fern_rank_keys: ctx is NULL" in lib.fern_last_error()
    assert lib.fern_rank_count(None, p, p, None, 2, 10, 64, p, 1, 0, None, p, None) == -1
    assert b"fern_rank_count: ctx is NULL" in lib.fern_last_error()


# ---- retrieval_metrics -----------------------------------------------------------------------------------------------------------
def test_retrieval_metrics_on_hand_made_ranks():
    from fashionern_aaai2024_amd.run._common import _pct, retrieval_metrics
    # three queries, up to three targets each: any-hit = the minimum over the valid ones; -1 = no target
    ranks = np.array([[7, 2, -1], [-1, -1, -1], [49, 50, 1000]])
    m = retrieval_metrics(ranks, (1, 3, 50))
    assert m["recall@1"] == 0.0
    assert m["recall@3"] == _pct(1, 3) and m["recall@50"] == _pct(2, 3)
    assert m["recall@3"] == (torch.tensor(1) / 3).item() * 100          # the reference's float32 sum / len, then * 100
    assert m["median_rank"] == 26.5 and m["mean_rank"] == 26.5          # places 3 and 50 (1-based); the query without a target is left out
    assert m["mrr"] == pytest.approx((1 / 3 + 1 / 50) / 3)              # ... and counts as a miss here
    flat = retrieval_metrics(np.array([0, 9, 10, -1]), (10,))
    assert flat["recall@10"] == _pct(2, 4) == 50.0
    assert flat["median_rank"] == 10.0 and flat["mean_rank"] == pytest.approx(22 / 3)
    empty = retrieval_metrics(np.array([-1, -1]), (10,))
    assert empty["recall@10"] == 0.0 and np.isnan(empty["median_rank"]) and empty["mrr"] == 0.0


# ---- the harness against the oracle engine -----------------------------------------------------------------------------------------
def _build(kind):
    import synthetic_data as sdata
    from fashionern_aaai2024_amd import synth
    from fashionern_aaai2024_amd.model import ERN
    from fashionern_aaai2024_amd.tokenizer import register_tokenizer
    from fashionern_aaai2024_amd.utils import extract_index_features
    register_tokenizer("stub", sdata.stub_tokenizer)
    d, n, q = META["d"], META["n"], META["q"]
    clip = sdata.StubCLIP(d).eval()
    model = ERN(clip, d, "cpu", engine=RankOracle())
    model.load_state_dict(synth.fusion_state_dict(d, seed=META["fusion_seed"]))
    gal = sdata.Gallery(n, d, seed=META["gallery_seed"], dup_names=(kind == "200k"))
    rel = sdata.RelativeDataset(gal, q, kind, seed=META["relative_seed"])
    feats, names, local = extract_index_features(sdata.ClassicDataset(gal), clip, 13, "cpu", d, num_workers=0)
    return clip, model, rel, feats, names, local, d


@pytest.mark.parametrize("kind", ["fiq", "cirr", "200k"])
def test_rank_metrics_reproduce_the_reference_recalls(kind):
    from fashionern_aaai2024_amd.run import rank_metrics
    fn = {"fiq": rank_metrics.compute_fiq_rank_metrics, "cirr": rank_metrics.compute_cirr_rank_metrics,
          "200k": rank_metrics.compute_200k_rank_metrics}[kind]
    clip, model, rel, feats, names, local, d = _build(kind)
    ks = (1, 5, 10, 50) if kind == "cirr" else (10, 50)
    res = fn(rel, clip, feats, local, names, model, "cpu", d, META["batch_size"], 0, "stub", ks=ks)
    golden = META["recalls"][kind][3:] if kind == "cirr" else META["recalls"][kind]      # cirr: (G@1, G@2, G@3, R@1, R@5, R@10, R@50)
    assert [res[f"recall@{k}"] for k in ks] == golden, (res, golden)
    assert set(res) == {f"recall@{k}" for k in ks} | {"median_rank", "mean_rank", "mrr"}
    assert 1.0 <= res["median_rank"] <= META["n"] and 1.0 <= res["mean_rank"] <= META["n"] and 0.0 < res["mrr"] <= 1.0


def test_ranks_below_50_agree_with_the_golden_top50_lists():
    from fashionern_aaai2024_amd.run import _common, test_fiq
    clip, model, rel, feats, names, local, d = _build("fiq")
    pred, targets = test_fiq.generate_fiq_val_predictions(clip, rel, model, names, feats, "cpu", d, META["batch_size"], 0, "stub")
    fused = _common.fuse_index(model, feats, local, prepared=True)
    tgt = _common._unique_rows(names, targets, "target")
    ranks = _common.target_ranks(model, pred, fused, tgt)
    assert ranks.shape == (len(targets), 1) and ranks.dtype == np.int32
    top50 = ARR["fiq_top50"]
    hit = top50 == tgt[:, None]
    assert np.array_equal(ranks[:, 0] < 50, hit.any(axis=1))
    in50 = hit.any(axis=1)
    assert in50.any() and not in50.all()                  # the fixture has targets on both sides of place 50
    assert np.array_equal(ranks[in50, 0], hit[in50].argmax(axis=1))
    assert (ranks[~in50, 0] >= 50).all()


# ---- world 2 over gloo -------------------------------------------------------------------------------------------------------------
def _sharded_case():
    """Operands in {-1, 0, 1} / 8: every dot product is exact in fp32 in any summation order, so a shard's scores are the whole
    gallery's bit for bit (and ties abound).  Ragged: 701 rows over two ranks are 351 + 350."""
    n, d, b = 701, 32, 6
    g = torch.Generator().manual_seed(5)
    gallery = torch.randint(-1, 2, (n, d), generator=g).float() / 8
    q = torch.randint(-1, 2, (b, d), generator=g).float() / 8
    targets = torch.tensor([[0, 350, 700], [351, 5, -1], [400, 400, 349], [700, 701, 3], [5, 352, 12], [650, 2, 351]], dtype=torch.int32)
    ex = torch.tensor([3, -1, 349, 700, 5, 400], dtype=torch.int32)      # row 2 / 3 / 4: the excluded row is one of the targets
    return gallery, q, targets, ex


def _worker(rank, world, out_dir):
    from fashionern_aaai2024_amd import distributed as fd
    gallery, q, targets, ex = _sharded_case()
    eng = RankOracle()
    start, stop, _ = fd.shard_rows(gallery.shape[0], rank, world)
    plain = fd.rank_of_sharded(eng, q, gallery[start:stop], start, targets)
    excl = fd.rank_of_sharded(eng, q, gallery[start:stop], start, targets, exclude_idx=ex)
    flat = fd.rank_of_sharded(eng, q, gallery[start:stop], start, targets[:, 0])
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), plain=plain.numpy(), excl=excl.numpy(), flat=flat.numpy())


def test_rank_of_sharded_equals_the_unsharded_ranks(tmp_path):
    gloo.spawn(2, _worker, str(tmp_path))
    gallery, q, targets, ex = _sharded_case()
    eng = RankOracle()
    plain = eng.rank_of(q, gallery, targets).numpy()
    excl = eng.rank_of(q, gallery, targets, exclude_idx=ex).numpy()
    assert (plain[1, 2], plain[3, 1]) == (-1, -1) and (excl[2, 2], excl[3, 0], excl[4, 0]) == (-1, -1, -1)
    assert (plain >= 0).sum() == 16 and len(np.unique(plain[plain >= 0])) > 8      # ranks all over the gallery, not a corner of it
    for rank in range(2):
        got = np.load(tmp_path / f"r{rank}.npz")
        assert np.array_equal(got["plain"], plain)
        assert np.array_equal(got["excl"], excl)
        assert np.array_equal(got["flat"], plain[:, 0])


def test_rank_of_sharded_makes_no_collective_in_a_world_of_one():
    from fashionern_aaai2024_amd import distributed as fd
    assert not (dist.is_available() and dist.is_initialized())
    gallery, q, targets, ex = _sharded_case()
    eng = RankOracle()
    got = fd.rank_of_sharded(eng, q, gallery, 0, targets, exclude_idx=ex)
    assert np.array_equal(got.numpy(), eng.rank_of(q, gallery, targets, exclude_idx=ex).numpy())

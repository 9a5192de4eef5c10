"""Candidate ranking without a GPU: the CPU oracle (tests/candidates_oracle.py) against a brute-force loop on tiny cases, the C ABI entry
point fern_sim_topk_candidates (header, library, ctypes table, ABI version), the engine wrapper's argument errors, and
distributed.rank_candidates_sharded over gloo with the oracle engine."""
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist

import gloo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the oracle against a brute-force loop ---------------------------------------------------------------------------------------------
def _brute(scores, cand, k, idx_offset, exclude, eligible):
    """One query at a time, in plain Python: the set of place-taking rows, sorted by (score descending, global index ascending)."""
    b, n = scores.shape
    out_s = np.full((b, k), -np.inf, dtype=np.float32)
    out_i = np.full((b, k), -1, dtype=np.int32)
    place = np.full(cand.shape, -1, dtype=np.int32)
    for r in range(b):
        rows = set()
        for c in cand[r]:
            loc = int(c) - idx_offset
            if c < 0 or loc < 0 or loc >= n or (exclude is not None and c == exclude[r]) or (eligible is not None and not eligible[r, loc]):
                continue
            rows.add(int(c))
        order = sorted(rows, key=lambda c: (-float(scores[r, c - idx_offset]), c))
        for p, c in enumerate(order[:k]):
            out_s[r, p], out_i[r, p] = scores[r, c - idx_offset], c
        for j, c in enumerate(cand[r]):
            if int(c) in rows:
                place[r, j] = order.index(int(c))
    return out_s, out_i, place


def _tiny():
    """Operands in {-1, 0, 1} / 8: every score is exact in fp32 and ties abound."""
    g = torch.Generator().manual_seed(2)
    n, d, b = 23, 8, 6
    gallery = torch.randint(-1, 2, (n, d), generator=g).float() / 8
    q = torch.randint(-1, 2, (b, d), generator=g).float() / 8
    cand = torch.tensor([[3, 3, 7, -1, 22, 23, 40, 7, 0, 5],            # duplicates, -1, past the gallery
                         [-1, -5, 99, 23, -1, 1000, 24, -2, 23, 50],      # all invalid
                         [4, 9, 4, 9, 4, 9, 14, 19, 1, 2],
                         [10, 11, 12, 13, 14, 15, 16, 17, 18, 19],
                         [0, 22, 0, 22, 11, 11, -1, -1, 6, 6],
                         [5, 5, 5, 5, 5, 5, 5, 5, 5, 5]], dtype=torch.int32)
    return gallery, q, cand


@pytest.mark.parametrize("k", (1, 4, 10, 17))          # 17 > M = 10
@pytest.mark.parametrize("idx_offset", (0, 5))
@pytest.mark.parametrize("use_exclude", (False, True))
@pytest.mark.parametrize("use_filter", (False, True))
def test_oracle_equals_a_brute_force_loop(k, idx_offset, use_exclude, use_filter):
    from candidates_oracle import candidates_oracle
    from fashionern_aaai2024_amd.engine import RowFilter
    gallery, q, cand = _tiny()
    n = gallery.shape[0]
    cand = cand + idx_offset * (cand >= 0)              # the same rows in the shifted frame; negatives stay negative
    ex = torch.tensor([3, 0, 9, 30, 22, 5], dtype=torch.int32) + idx_offset if use_exclude else None
    flt = RowFilter((torch.arange(n) % 3).to(torch.int32), 3, torch.tensor([0, 1, 2, 0, 1, 2], dtype=torch.int32)) if use_filter else None
    eng = candidates_oracle()()
    s, i, p = eng.sim_topk_candidates(q, gallery, cand, k, idx_offset=idx_offset, exclude_idx=ex, row_filter=flt, places=True)
    el = None if flt is None else ((torch.arange(n)[None, :] % 3) == flt.value[:, None]).numpy()
    ws, wi, wp = _brute(eng._scores(q, gallery), cand.numpy(), k, idx_offset, None if ex is None else ex.numpy(), el)
    assert np.array_equal(i.numpy(), wi) and np.array_equal(s.numpy().view(np.int32), ws.view(np.int32)) and np.array_equal(p.numpy(), wp)
    assert (i[1] == -1).all() and (p[1] == -1).all() and torch.isinf(s[1]).all()        # the all-invalid list
    two = eng.sim_topk_candidates(q, gallery, cand, k, idx_offset=idx_offset, exclude_idx=ex, row_filter=flt)
    assert len(two) == 2 and torch.equal(two[1], i)


def test_oracle_on_an_empty_gallery():
    from candidates_oracle import candidates_oracle
    s, i, p = candidates_oracle()().sim_topk_candidates(torch.zeros(2, 8), torch.zeros(0, 8), torch.tensor([[0, 1], [2, -1]]), 3, places=True)
    assert (i == -1).all() and (p == -1).all() and torch.isinf(s).all()


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_candidates_entry_point_is_declared_exported_and_typed():
    from fashionern_aaai2024_amd import _lib
    header = open(os.path.join(ROOT, "include", "fern.h")).read()
    lib = _lib.load()
    decl = re.search(r"FERN_API int fern_sim_topk_candidates\((.*?)\);", header, flags=re.S)
    assert decl and hasattr(lib, "fern_sim_topk_candidates")
    params = [p for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if p.strip()]
    assert len(params) == len(_lib.SIGNATURES["fern_sim_topk_candidates"][1]) == 19
    assert "run/test/test_cirr.py:55-69" in header
    assert lib.fern_abi_version() == 3 and "#define FERN_ABI_VERSION 3" in header


def test_candidates_argument_errors_name_the_function():
    from fashionern_aaai2024_amd import _lib
    lib = _lib.load()
    p = 0x1000                                          # never dereferenced: every call below is refused before any HIP call

    def call(**over):
        a = dict(ctx=None, q=p, gallery=p, gallery_bf16=None, B=2, N=10, D=64, cand=p, M=6, K=5, out_scores=p, out_idx=p, out_place=None,
                 idx_offset=0, exclude_idx=None, tags=None, mask=None, value=None, stream=None)
        a.update(over)
        return lib.fern_sim_topk_candidates(*a.values()), lib.fern_last_error().decode()

    assert call() == (-1, "fern_sim_topk_candidates: ctx is NULL")              # nothing else to refuse: the context comes last
    for over, text in ((dict(M=0), "need 1<=M<=4096"), (dict(M=4097), "need 1<=M<=4096"), (dict(K=0), "need 1<=K<=1024"),
                       (dict(K=1025), "need 1<=K<=1024"), (dict(tags=p), "mask or value is NULL"), (dict(cand=None), "NULL argument"),
                       (dict(D=48), "the fp32 form needs D % 32 == 0"),
                       (dict(gallery=None, gallery_bf16=p, D=96), "a bf16-only gallery needs D % 64 == 0, D <= 768"),
                       (dict(gallery=None), "gallery and gallery_bf16 are both NULL")):
        assert call(**over) == (-1, "fern_sim_topk_candidates: " + text), over


# ---- the engine wrapper ----------------------------------------------------------------------------------------------------------------
def test_engine_wrapper_argument_errors():
    from fashionern_aaai2024_amd.engine import FernEngine

    class Hostless(FernEngine):
        """No context and no library: a call that gets past the argument handling fails with AttributeError, not ValueError."""
        def __init__(self):
            self.device = torch.device("cpu")

    eng = Hostless()
    b, n, d = 3, 7, 64
    q, g = torch.zeros(b, d), torch.zeros(n, d)
    good = torch.zeros(b, 4, dtype=torch.int32)
    for bad in (torch.zeros(b, dtype=torch.int32), torch.zeros(b + 1, 4, dtype=torch.int32), torch.zeros(b, 4), torch.zeros(b, 4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="candidates must be an integer"):
            eng.sim_topk_candidates(q, g, bad, 5)
    with pytest.raises(ValueError, match=r"exclude_idx must be \[B\]"):
        eng.sim_topk_candidates(q, g, good, 5, exclude_idx=torch.zeros(b + 1, dtype=torch.int32))
    with pytest.raises(TypeError, match="row_filter must be a RowFilter"):
        eng.sim_topk_candidates(q, g, good, 5, row_filter=(1, 2, 3))
    with pytest.raises(ValueError, match="must share D"):
        eng.sim_topk_candidates(q, torch.zeros(n, d + 32), good, 5)
    for ok in (good, good.tolist(), good.numpy().astype(np.int64)):      # well-formed lists go on to the library
        with pytest.raises(AttributeError):
            eng.sim_topk_candidates(q, g, ok, 5)


def test_recalls_cirr_subset_and_pipeline_keywords_exist():
    import inspect

    from fashionern_aaai2024_amd.pipeline import ComposedQueryPipeline, QueryResult
    from fashionern_aaai2024_amd.run import _cli, _common
    assert inspect.signature(_common.recalls_cirr).parameters["subset"].default is None and _common._cirr_subset == "gather"
    with pytest.raises(ValueError):
        _common.recalls_cirr(None, None, None, [], [], [], [], subset="sorted")
    assert inspect.signature(ComposedQueryPipeline.submit).parameters["candidates"].default is None
    assert list(inspect.signature(QueryResult.__init__).parameters)[-1] == "place"
    assert _cli.build_parser("cirr").parse_args(["--subset-candidates"]).subset_candidates is True
    with pytest.raises(SystemExit):
        _cli.build_parser("fiq").parse_args(["--subset-candidates"])


# ---- world 2 over gloo -----------------------------------------------------------------------------------------------------------------
def _sharded_case():
    """Operands in {-1, 0, 1} / 8 (exact scores, many ties); 701 rows over two ranks are 351 + 350; lists that straddle the cut, with
    duplicates, negatives and entries past the gallery."""
    from fashionern_aaai2024_amd.engine import RowFilter
    n, d, b, m = 701, 32, 6, 90
    g = torch.Generator().manual_seed(5)
    gallery = torch.randint(-1, 2, (n, d), generator=g).float() / 8
    q = torch.randint(-1, 2, (b, d), generator=g).float() / 8
    cand = torch.randint(-4, n + 4, (b, m), generator=g, dtype=torch.int32)
    cand[:, 5] = cand[:, 4]
    ex = cand[:, 0].clone()
    rows = torch.arange(n)
    flt = (((rows % 3) | ((rows % 7 != 0).long() << 2)).to(torch.int32), torch.tensor([4, 4, 7, 7, 0, 1], dtype=torch.int32),
           torch.tensor([4, 4, 4, 5, 0, 2], dtype=torch.int32))
    return gallery, q, cand, ex, flt, RowFilter


def _worker(rank, world, out_dir):
    from candidates_oracle import candidates_oracle
    from fashionern_aaai2024_amd import distributed as fd
    gallery, q, cand, ex, (tags, mask, value), RowFilter = _sharded_case()
    eng = candidates_oracle()()
    start, stop, _ = fd.shard_rows(gallery.shape[0], rank, world)
    s, i = fd.rank_candidates_sharded(eng, q, gallery[start:stop], start, cand, 50)
    s2, i2 = fd.rank_candidates_sharded(eng, q, gallery[start:stop], start, cand, 120, exclude_idx=ex, row_filter=RowFilter(tags[start:stop], mask, value))
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), s=s.numpy(), i=i.numpy(), s2=s2.numpy(), i2=i2.numpy())


def test_sharded_candidate_ranking_equals_the_unsharded_oracle(tmp_path):
    from candidates_oracle import candidates_oracle
    from fashionern_aaai2024_amd import distributed as fd
    gloo.spawn(2, _worker, str(tmp_path))
    gallery, q, cand, ex, (tags, mask, value), RowFilter = _sharded_case()
    eng = candidates_oracle()()
    s, i = eng.sim_topk_candidates(q, gallery, cand, 50)
    s2, i2 = eng.sim_topk_candidates(q, gallery, cand, 120, exclude_idx=ex, row_filter=RowFilter(tags, mask, value))
    assert (i >= 0).all() and (i2[5] == -1).all() and (i2[4] >= 0).sum() > 50 and ((i < 351).any() and (i >= 351).any())
    for rank in range(2):
        got = np.load(tmp_path / f"r{rank}.npz")
        assert np.array_equal(got["i"], i.numpy()) and np.array_equal(got["s"], s.numpy())
        assert np.array_equal(got["i2"], i2.numpy()) and np.array_equal(got["s2"], s2.numpy())
    # a world of one makes no collective
    assert not (dist.is_available() and dist.is_initialized())
    one = fd.rank_candidates_sharded(eng, q, gallery, 0, cand, 50)
    assert torch.equal(one[1], i) and torch.equal(one[0], s)

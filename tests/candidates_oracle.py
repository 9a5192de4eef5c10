"""The CPU oracle of candidate ranking (include/fern.h: fern_sim_topk_candidates), without a second copy of the ranking rules.
TEST INFRASTRUCTURE.

``candidates_oracle()`` returns the rank oracle over ``oracle.chain.chain_scores`` (tests/rank_oracle.py: ``CandidatesOracle``; the fp32
chain of oracle/chain.c), whose ``sim_topk_candidates`` orders by ``make_keys`` (score descending, global index ascending as one
unsigned compare).  The set semantics are restated here in a few lines of numpy:

    query b ranks the SET of rows named by candidates[b]; an entry takes no place if it is negative, outside [idx_offset, idx_offset + N),
    equal to exclude_idx[b] or ineligible under the row filter; a row named twice counts once; place[b][j] = the number of distinct
    place-taking candidates with a greater key, -1 for an entry that takes none; unfilled places are -inf / -1.
"""
from __future__ import annotations

import numpy as np


def valid_entries(cand, n, idx_offset=0, exclude_idx=None, eligible=None):
    """bool [B, M]: which entries of `cand` (int64 [B, M], global indices) take a place; `eligible`: bool [B, N] or None."""
    local = cand - idx_offset
    ok = (cand >= 0) & (local >= 0) & (local < n)
    if exclude_idx is not None:
        ok &= cand != np.asarray(exclude_idx, dtype=np.int64)[:, None]
    if eligible is not None and n:
        ok &= np.take_along_axis(eligible, np.where(ok, local, 0), axis=1)
    return ok


def rank_candidates(scores, cand, k, idx_offset=0, exclude_idx=None, eligible=None, make_keys=None):
    """(scores [B,k] f32, idx [B,k] int32, place [B,M] int32) from a full score matrix `scores` [B, N] (numpy f32)."""
    b, n = scores.shape
    cand = np.asarray(cand, dtype=np.int64)
    ok = valid_entries(cand, n, idx_offset, exclude_idx, eligible)
    local = np.where(ok, cand - idx_offset, 0)
    es = np.take_along_axis(scores, local, axis=1) if n else np.zeros(cand.shape, dtype=np.float32)
    keys = np.where(ok, make_keys(es, np.where(ok, cand, 0)), np.uint64(0))           # 0: takes no place
    out_s = np.full((b, k), -np.inf, dtype=np.float32)
    out_i = np.full((b, k), -1, dtype=np.int32)
    place = np.full(cand.shape, -1, dtype=np.int32)
    for r in range(b):
        distinct = np.unique(keys[r][keys[r] != 0])[::-1]                             # descending: a key names one row
        kk = min(k, len(distinct))
        first = {int(key): j for j, key in reversed(list(enumerate(keys[r])))}        # any entry of a row carries its score and index
        for p in range(kk):
            j = first[int(distinct[p])]
            out_s[r, p], out_i[r, p] = es[r, j], cand[r, j]
        asc = distinct[::-1]
        place[r] = np.where(ok[r], len(asc) - np.searchsorted(asc, keys[r], side="right"), -1)
    return out_s, out_i, place


def candidates_oracle():
    from rank_oracle import CandidatesOracle
    return CandidatesOracle

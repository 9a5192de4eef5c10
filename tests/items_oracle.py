"""The CPU oracle of item-level ranking (include/fern.h: fern_sim_topk_items, fern_item_rank).  TEST INFRASTRUCTURE.

A numpy restatement of the definition, on any [B, N] score matrix: apply `exclude_idx` and the row filter, sort the rows stably by
(score descending, index ascending), keep the first row of every item, pad.  A rank is the position of the target item in that list.
`chain_item_topk` / `chain_item_ranks` feed it oracle.chain's fp32-chain scores (as tests/test_gpu_rank_deep.py:_oracle does);
`items_oracle()` returns the engine that serves them as the item protocol of FernEngine to the CPU tests (tests/rank_oracle.py).
"""
from __future__ import annotations

import numpy as np

from oracle.rank import masked_scores


def item_lists(masked, items, n_items):
    """Per query the item-level ranking as (local row, item id) arrays: the stable (-score, index) order of the rows that score above
    -inf and whose id is inside [0, n_items), first row of every item only."""
    items = np.asarray(items, dtype=np.int64)
    out = []
    for row in masked:
        order = np.argsort(-row, kind="stable")
        order = order[(row[order] > -np.inf) | np.isnan(row[order])]
        order = order[(items[order] >= 0) & (items[order] < n_items)]
        _, first = np.unique(items[order], return_index=True)
        rows = order[np.sort(first)]
        out.append((rows, items[rows]))
    return out


def item_topk(masked, items, n_items, k, idx_offset=0):
    """(scores, idx, item) [B, k] of the definition; unfilled places -inf / -1 / -1."""
    b = masked.shape[0]
    out_s = np.full((b, k), -np.inf, dtype=np.float32)
    out_i = np.full((b, k), -1, dtype=np.int32)
    out_t = np.full((b, k), -1, dtype=np.int32)
    for r, (rows, ids) in enumerate(item_lists(masked, items, n_items)):
        kk = min(k, len(rows))
        out_s[r, :kk] = masked[r, rows[:kk]]
        out_i[r, :kk] = rows[:kk] + idx_offset
        out_t[r, :kk] = ids[:kk]
    return out_s, out_i, out_t


def item_ranks(masked, items, n_items, target_items):
    """int32 [B, m]: the position of every target item in its query's list, -1 when it is not in it."""
    t = np.asarray(target_items, dtype=np.int64)
    t = t[:, None] if t.ndim == 1 else t
    out = np.full(t.shape, -1, dtype=np.int32)
    for r, (_, ids) in enumerate(item_lists(masked, items, n_items)):
        place = np.full(n_items, -1, dtype=np.int32)
        place[ids] = np.arange(len(ids), dtype=np.int32)
        ok = (t[r] >= 0) & (t[r] < n_items)
        out[r, ok] = place[t[r][ok]]
    return out


def chain_item_topk(q, g, items, n_items, k, idx_offset=0, exclude_idx=None, eligible=None):
    from oracle import chain
    s = chain.chain_scores(np.asarray(q, dtype=np.float32), np.asarray(g, dtype=np.float32))
    return item_topk(masked_scores(s, idx_offset, exclude_idx, eligible), items, n_items, k, idx_offset)


def chain_item_ranks(q, g, items, n_items, target_items, idx_offset=0, exclude_idx=None, eligible=None):
    from oracle import chain
    s = chain.chain_scores(np.asarray(q, dtype=np.float32), np.asarray(g, dtype=np.float32))
    return item_ranks(masked_scores(s, idx_offset, exclude_idx, eligible), items, n_items, target_items)


def items_oracle():
    from rank_oracle import RankOracle
    return RankOracle

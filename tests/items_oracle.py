"""The CPU oracle of item-level ranking (include/fern.h: fern_sim_topk_items, fern_item_rank).  TEST INFRASTRUCTURE.

A numpy restatement of the definition, on any [B, N] score matrix: apply `exclude_idx` and the row filter, sort the rows stably by
(score descending, index ascending), keep the first row of every item, pad.  A rank is the position of the target item in that list.
`chain_item_topk` / `chain_item_ranks` feed it oracle.chain's fp32-chain scores (as tests/test_gpu_rank_deep.py:_oracle does);
`items_oracle()` returns a subclass of the test-only OracleEngine with the item protocol of FernEngine for the CPU tests.
"""
from __future__ import annotations

import numpy as np
import torch


def masked_scores(scores, idx_offset=0, exclude_idx=None, eligible=None):
    """A copy of `scores` [B, N] with the excluded row (a global index per query) and the ineligible rows (bool [B, N]) at -inf."""
    s = np.array(scores, dtype=np.float32, copy=True)
    b, n = s.shape
    if eligible is not None:
        s[~np.asarray(eligible, dtype=bool)] = -np.inf
    if exclude_idx is not None:
        ex = np.asarray(exclude_idx, dtype=np.int64) - idx_offset
        for r in np.nonzero((ex >= 0) & (ex < n))[0]:
            s[r, ex[r]] = -np.inf
    return s


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
    from filtered_oracle import eligible as _eligible, filtered_oracle
    from test_rank_of_cpu import _make_keys

    class ItemsOracle(filtered_oracle()):
        """The filtered oracle engine + FernEngine's item protocol, from its own scores (q @ g.T)."""

        def _item_masked(self, q, gallery, items, idx_offset, exclude_idx, row_filter):
            s = self._scores(q, gallery)
            ids = items.resolve(s.shape[1], "cpu").numpy()
            el = None if row_filter is None else _eligible(row_filter, *s.shape).numpy()
            ex = None if exclude_idx is None else torch.as_tensor(exclude_idx).numpy()
            return masked_scores(s, idx_offset, ex, el), ids

        def sim_topk_items(self, q, gallery, items, k, idx_offset=0, exclude_idx=None, row_filter=None):
            m, ids = self._item_masked(q, gallery, items, idx_offset, exclude_idx, row_filter)
            return tuple(torch.from_numpy(a) for a in item_topk(m, ids, items.n_items, k, idx_offset))

        def item_rank_of(self, q, gallery, items, target_items, idx_offset=0, exclude_idx=None, row_filter=None):
            m, ids = self._item_masked(q, gallery, items, idx_offset, exclude_idx, row_filter)
            out = item_ranks(m, ids, items.n_items, self._2d(target_items, np.int64))
            return torch.from_numpy(out[:, 0] if torch.as_tensor(target_items).dim() == 1 else out)

        def _best(self, q, gallery, items, idx_offset, exclude_idx, row_filter):
            """uint64 [B, n_items]: the key of every item's representative in this gallery (shard), 0 when it has none."""
            m, ids = self._item_masked(q, gallery, items, idx_offset, exclude_idx, row_filter)
            best = np.zeros((m.shape[0], items.n_items), dtype=np.uint64)
            for r, (rows, its) in enumerate(item_lists(m, ids, items.n_items)):
                best[r, its] = _make_keys(m[r, rows], rows + idx_offset)
            return best

        def item_keys(self, q, gallery, items, target_items, idx_offset=0, exclude_idx=None, row_filter=None):
            best = self._best(q, gallery, items, idx_offset, exclude_idx, row_filter)
            t = self._2d(target_items, np.int64)
            ok = (t >= 0) & (t < items.n_items)
            keys = np.where(ok, np.take_along_axis(best, np.where(ok, t, 0), axis=1), np.uint64(0))
            return torch.from_numpy(keys.view(np.int64).copy())

        def item_count(self, q, gallery, items, keys, idx_offset=0, exclude_idx=None, row_filter=None):
            best = self._best(q, gallery, items, idx_offset, exclude_idx, row_filter)
            k = self._2d(keys, np.int64).view(np.uint64)
            count = (best[:, :, None] > k[:, None, :]).sum(axis=1)
            return torch.from_numpy(np.where(k == 0, -1, count).astype(np.int32))

    return ItemsOracle

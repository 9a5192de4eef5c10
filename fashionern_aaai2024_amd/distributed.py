"""Multi-GPU layout of the path: one process per GPU, torch.distributed over RCCL ("nccl" on ROCm) / xGMI.

The reference's inference is single-GPU with no collective; sharding is new design:

* **gallery build** -- rank r fuses rows [r*ceil(N/W), ...) of the gallery (``mode="index"``), then ONE
  ``all_gather`` of the fused [N/W, D] blocks leaves the whole fused gallery on every GPU (46k x 512 fp32 = 94 MB;
  1M x 512 = 2 GB: trivially resident in 288 GB).  xGMI is point-to-point, so a single large all-gather (one shard
  per link) is the right shape -- there is nothing to bucket;
* **queries** -- data-parallel: every rank encodes, fuses and ranks its own B/W queries against the replicated
  gallery; no per-batch collective.  Results are gathered only for reporting;
* **sharded ranking** (alternative for very large N or tiny B): keep the gallery sharded, all-gather the fused
  queries [B, D], rank locally with ``idx_offset``, all-gather the [B, K] candidates and merge them
  (``topk_merge``: score desc, global index asc -- identical to the single-GPU ordering).

The compute object is an engine (``FernEngine`` in production).  Collectives go through ``torch.distributed`` so the
same code runs over RCCL on GPUs and over gloo in the CPU tests.
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import numpy as np

import torch
import torch.distributed as dist

from .engine import per_query


def init_from_env(backend: Optional[str] = None) -> Tuple[int, int, int]:
    """Initialise the default process group from RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* (torchrun contract).
    Returns (rank, world, local_rank); a single process without those variables is (0, 1, 0) with no group."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        if backend is None:
            # FERN_DIST_BACKEND overrides (debug: e.g. two ranks sharing the one GPU of a dev box over gloo)
            backend = os.environ.get("FERN_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend == "nccl":
            torch.cuda.set_device(local)
            dist.init_process_group(backend, rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, world, local


def world_info() -> Tuple[int, int]:
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _all_gather_into(out: torch.Tensor, inp: torch.Tensor) -> None:
    """`dist.all_gather_into_tensor(out, inp)` as BYTES (a bf16 / int32 block needs no dtype support from the backend), and
    through the host when the backend is gloo but the tensors live on a GPU (the debug layout: several ranks sharing the one GPU
    of a dev box, FERN_DIST_BACKEND=gloo) -- RCCL takes the device tensors as they are."""
    inp = inp.contiguous()
    if dist.get_backend() == "gloo" and inp.is_cuda:
        host = torch.empty(out.shape, dtype=out.dtype)
        dist.all_gather_into_tensor(host.view(torch.uint8).view(-1), inp.cpu().view(torch.uint8).view(-1))
        out.copy_(host)
        return
    dist.all_gather_into_tensor(out.view(torch.uint8).view(-1), inp.view(torch.uint8).view(-1))


def shard_rows(n: int, rank: int, world: int) -> Tuple[int, int, int]:
    """Contiguous equal shards of ceil(n / world) rows (the last ones may be short or empty): (start, stop, per)."""
    per = (n + world - 1) // world
    start = min(n, rank * per)
    return start, min(n, start + per), per


def build_gallery(engine, index_features: torch.Tensor, index_local: torch.Tensor, normalize_input: bool = True, prepared: bool = False):
    """Fused gallery [N, D] on every rank.  ``index_features`` / ``index_local`` are the FULL raw index (every rank
    holds or can address it); each rank fuses only its shard, then one all_gather replicates the result.
    ``prepared`` (world > 1, an engine with `prepare_gallery`): return the gathered `PreparedGallery` (`all_gather_prepared`: each rank
    prepares only its shard) instead of the fp32 tensor."""
    rank, world = world_info()
    n, d = index_features.shape
    if world == 1:
        return engine.index_fuse(index_features, index_local, normalize_input=normalize_input)
    start, stop, per = shard_rows(n, rank, world)
    dev = engine.device
    block = torch.zeros((per, d), dtype=torch.float32, device=dev)       # padded so every rank contributes `per` rows
    if stop > start:
        block[: stop - start] = engine.index_fuse(index_features[start:stop], index_local[start:stop],
                                                  normalize_input=normalize_input)
    if prepared and hasattr(engine, "prepare_gallery") and d % 4 == 0:
        return all_gather_prepared(engine, block, n)
    full = torch.empty((world * per, d), dtype=torch.float32, device=dev)
    _all_gather_into(full, block)
    return full[:n]


def all_gather_shards(block: torch.Tensor, n_total: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ONE all_gather of equally sized per-rank blocks [per, ...] (``per = ceil(n_total / world)``, short shards zero-padded by
    the caller) -> the first ``n_total`` rows of their concatenation on every rank.  This is the path's only data-path
    collective: one shard per xGMI link, nothing to bucket.  ``out`` ([world * per, ...], same dtype / device): the gallery
    store of a serving process, allocated when the process starts -- the collective writes straight into it (world 1: one copy)."""
    rank, world = world_info()
    if out is not None and (tuple(out.shape) != (world * block.shape[0],) + tuple(block.shape[1:]) or out.dtype != block.dtype
                            or out.device != block.device or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous [{world * block.shape[0]}, ...] {block.dtype} tensor on {block.device}")
    if world == 1:
        if out is None:
            return block[:n_total]
        out.copy_(block)
        return out[:n_total]
    block = block.contiguous()
    full = out if out is not None else torch.empty((world * block.shape[0],) + tuple(block.shape[1:]), dtype=block.dtype, device=block.device)
    _all_gather_into(full, block)      # as bytes: a bf16 gallery (config 5) needs no bf16 support from the backend (gloo has none)
    return full[:n_total]


def _all_reduce(x: torch.Tensor, op) -> torch.Tensor:
    """In-place all-reduce of a small tensor (through the host under the gloo debug backend with device tensors)."""
    if dist.get_backend() == "gloo" and x.is_cuda:
        h = x.cpu()
        dist.all_reduce(h, op=op)
        x.copy_(h)
    else:
        dist.all_reduce(x, op=op)
    return x


def all_gather_prepared(engine, block: torch.Tensor, n_total: int, out=None):
    """The replicated gallery in its PREPARED form (engine.prepare_gallery: fp32 rows + certified bf16 pre-filter copy + the three norms)
    without any rank preparing more than its own shard (round 5 all-gathered the fp32 blocks and then ran
    `fern_gallery_prepare` over the WHOLE gallery on every rank -- 35 ms at 1M rows, W times the work).  `block` [per, D] fp32 is this
    rank's fused shard, zero-padded to ``per = ceil(n_total / world)`` rows.  Each rank prepares its block; the fp32 blocks and the
    bf16 blocks are all-gathered (as bytes) and the norms MAX-reduced: a maximum of maxima is exact and a zero padding row has norm 0,
    so rows, bf16 copy and the four floats are bit for bit what preparing the gathered gallery gives.
    `out`: a `PreparedGallery` whose tensors are [world * per, D] stores to gather into (a serving process's gallery)."""
    from .engine import PreparedGallery
    rank, world = world_info()
    block = block.contiguous()
    mine = engine.prepare_gallery(block)
    if world == 1:
        if out is None:
            return PreparedGallery(mine.f32[:n_total], mine.bf16[:n_total], mine.meta)
        out.f32.copy_(mine.f32)
        out.bf16.copy_(mine.bf16)
        out.meta.copy_(mine.meta)
        return PreparedGallery(out.f32[:n_total], out.bf16[:n_total], out.meta)
    f32 = all_gather_shards(mine.f32, n_total, out=None if out is None else out.f32)
    b16 = all_gather_shards(mine.bf16, n_total, out=None if out is None else out.bf16)
    meta = mine.meta.clone() if out is None else out.meta.copy_(mine.meta)
    _all_reduce(meta, dist.ReduceOp.MAX)
    return PreparedGallery(f32, b16, meta)


def build_gallery_from_shard(engine, shard_features: torch.Tensor, shard_local: torch.Tensor, n_total: int,
                             normalize_input: bool = True) -> torch.Tensor:
    """Sharded gallery build: this rank holds ONLY its own rows [start, stop) of the raw index
    (``shard_rows(n_total, rank, world)``), fuses them with ``mode="index"`` and the fused blocks are all-gathered.  Unlike
    ``build_gallery`` no rank ever needs the whole raw index (6.6 GB of local features at C3, 27 GB at C5)."""
    rank, world = world_info()
    start, stop, per = shard_rows(n_total, rank, world)
    if shard_features.shape[0] != stop - start:
        raise ValueError(f"rank {rank} must hold rows [{start}, {stop}) of the index, got {shard_features.shape[0]} rows")
    block = torch.zeros((per, shard_features.shape[1]), dtype=torch.float32, device=engine.device)
    if stop > start:
        block[: stop - start] = engine.index_fuse(shard_features, shard_local, normalize_input=normalize_input)
    return all_gather_shards(block, n_total)


def rank_replicated(engine, queries: torch.Tensor, gallery: torch.Tensor, k: int, exclude_idx=None):
    """Query-data-parallel ranking: this rank's queries against the replicated gallery.  No collective.  k > 64: the deep ranking."""
    if k > 64:
        return engine.sim_topk_deep(queries, gallery, k, exclude_idx=exclude_idx)
    return engine.sim_topk(queries, gallery, k, exclude_idx=exclude_idx)


def _filter_kw(row_filter) -> dict:
    """An unfiltered call passes NO `row_filter` keyword: an engine that does not know filters serves it."""
    return {} if row_filter is None else {"row_filter": row_filter}


def _gather_merge(engine, scores: torch.Tensor, idx: torch.Tensor, extra: Optional[torch.Tensor] = None):
    """The shards' local [B, K] lists (global indices) -> (scores, idx, gathered): every list is all-gathered as [world, B, K] and the
    first two are merged (`engine.topk_merge`: score descending, global index ascending).  `gathered` is the all-gathered (idx, extra)
    for a caller that looks something up beside the merge.  World 1: the local lists, None, no collective."""
    rank, world = world_info()
    if world == 1:
        return scores, idx, None
    b, kk = scores.shape
    full = [torch.empty((world * b, kk), dtype=t.dtype, device=t.device)      # concatenated along dim 0 == [world, B, K]
            for t in (scores, idx, extra) if t is not None]
    for out, t in zip(full, (scores, idx, extra)):
        _all_gather_into(out, t)
    full = [t.view(world, b, kk) for t in full]
    merged_s, merged_i = engine.topk_merge(full[0], full[1])
    return merged_s, merged_i, tuple(full[1:])


def rank_sharded(engine, queries: torch.Tensor, gallery_shard: torch.Tensor, shard_start: int, k: int, exclude_idx=None, row_filter=None):
    """Gallery-sharded ranking of the SAME query batch on every rank: local top-K with global indices, all-gather of
    the [B, K] candidates, merge.  Returns the global (scores, idx) on every rank.  k > 64: the deep ranking and the wide merge.
    `row_filter`: the SHARD's `RowFilter` -- tags shard with the rows, mask / value are the same on every rank; the filtered lists
    merge exactly like the unfiltered ones."""
    rank_fn = engine.sim_topk_deep if k > 64 else engine.sim_topk
    s, i = rank_fn(queries, gallery_shard, k, idx_offset=shard_start, exclude_idx=exclude_idx, **_filter_kw(row_filter))
    return _gather_merge(engine, s, i)[:2]


def rank_from_sharded(engine, queries: torch.Tensor, gallery_shard, shard_start: int, k: int, from_keys, exclude_idx=None, row_filter=None):
    """Gallery-sharded CONTINUATION of a result list for the SAME query batch on every rank: `FernEngine.sim_topk_from` on the shard with
    ``idx_offset = shard_start`` -- the cursor `from_keys` [B] carries a global row index, so every shard answers "my best k at or below
    this key" whether or not it owns the cursor's row -- then the all-gather and merge of `rank_sharded`.  Returns the global
    (scores, idx) on every rank; `engine.next_from` of it is the next cursor.  World 1 makes no collective.  `row_filter`: the SHARD's.
    Random access by OFFSET on a sharded gallery is out of scope: a global select is not additive over shards (the key at a global
    place is not a function of the shards' keys at any local places), so sharded callers page by cursor."""
    s, i = engine.sim_topk_from(queries, gallery_shard, k, from_keys, idx_offset=shard_start, exclude_idx=exclude_idx, **_filter_kw(row_filter))
    return _gather_merge(engine, s, i)[:2]


def rank_candidates_sharded(engine, queries: torch.Tensor, gallery_shard, shard_start: int, candidates, k: int, exclude_idx=None, row_filter=None):
    """Gallery-sharded CANDIDATE ranking of the SAME query batch and the SAME lists on every rank (`FernEngine.sim_topk_candidates`):
    `candidates` [B,M] hold global row indices, the local call runs with ``idx_offset = shard_start``, so a shard ranks the candidates
    it owns and the others take no place there; then the all-gather and merge of `rank_sharded`.  Returns the global (scores, idx) on
    every rank.  `row_filter`: the SHARD's.  No places: a place inside the whole list is not a function of the places inside the shards'
    parts (count the keys with `rank_of_sharded` instead)."""
    s, i = engine.sim_topk_candidates(queries, gallery_shard, candidates, k, idx_offset=shard_start, exclude_idx=exclude_idx, **_filter_kw(row_filter))
    return _gather_merge(engine, s, i)[:2]


def route_rows(slots, bounds) -> List[np.ndarray]:
    """Host-side partition of a gallery UPDATE by owning shard.  `slots` [m] are global gallery rows (the slots of a sharded
    `live_gallery.LiveGallery`: shard r holds rows [bounds[r], bounds[r + 1]) and its store has ``slot_offset = bounds[r]``), `bounds`
    the W + 1 ascending shard boundaries.  Returns W int64 arrays: for each rank the POSITIONS in `slots` (ascending, so the caller's
    order is kept) of the rows it owns -- ``rows[idx[r]]`` / ``slots[idx[r]]`` is what rank r appends or replaces.  No collective: an
    update is routed, each shard applies its part.  Raises on a slot outside [bounds[0], bounds[-1])."""
    sl = np.asarray(slots).astype(np.int64).reshape(-1)
    b = np.asarray(bounds, dtype=np.int64).reshape(-1)
    if b.size < 2 or (np.diff(b) < 0).any():
        raise ValueError("bounds must be W + 1 ascending shard boundaries")
    if sl.size and (sl.min() < b[0] or sl.max() >= b[-1]):
        raise IndexError(f"a slot lies outside [{int(b[0])}, {int(b[-1])})")
    owner = np.searchsorted(b, sl, side="right") - 1
    return [np.nonzero(owner == r)[0] for r in range(b.size - 1)]


def _count_keys(keys: torch.Tensor, count) -> torch.Tensor:
    """The target-rank sequence over the shards.  `keys` int64 [B, m] hold each target's key on the shard that owns it and 0 on every
    other, so their SUM all-reduce is exact, wrap-around included; `count(keys)` is this shard's int32 [B, m] count of what outranks
    them, -1 for a key of 0 -- which is -1 on every rank: summed as 0, restored after the SUM.  Two small collectives; world 1 makes
    none and returns `count(keys)` as it is."""
    rank, world = world_info()
    if world == 1:
        return count(keys)
    _all_reduce(keys, dist.ReduceOp.SUM)
    counts = _all_reduce(count(keys).clamp(min=0), dist.ReduceOp.SUM)
    return torch.where(keys == 0, torch.full_like(counts, -1), counts)


def rank_of_sharded(engine, queries: torch.Tensor, gallery_shard, shard_start: int, targets, exclude_idx=None, row_filter=None):
    """Gallery-sharded exact target ranks of the SAME query batch on every rank (`FernEngine.rank_of` on the whole gallery): the key of
    a target comes from the shard that owns its row -- every other rank contributes 0, so the int64 SUM all-reduce is exact, wrap-around
    included -- then every rank counts the rows of its shard that outrank the keys and the counts are SUM-reduced.  Two small
    collectives of [B, m] integers; world 1 makes none.  Returns int32 shaped like `targets` on every rank; -1 for a target < 0,
    outside the gallery, or equal to the query's excluded row.  `row_filter`: the SHARD's `RowFilter` (tags shard with the rows): only
    eligible rows are counted, and the shard that owns a target drops its key when the target is not eligible (-1 on every rank)."""
    t2, restore = per_query(targets, queries.shape[0], torch.int32, "targets")
    keys = engine.rank_keys(queries, gallery_shard, t2, idx_offset=shard_start)
    if row_filter is not None:
        n = gallery_shard.shape[0]
        local = t2.to(device=keys.device, dtype=torch.int64) - int(shard_start)
        mine = (local >= 0) & (local < n)
        ok = row_filter.eligible(*row_filter.resolve(keys.shape[0], n, keys.device), local)
        keys = torch.where(mine & ~ok, torch.zeros_like(keys), keys)
    if exclude_idx is not None:      # on every rank alike, so before or after the keys' SUM is the same
        ex = torch.as_tensor(exclude_idx).to(device=keys.device, dtype=torch.int32)
        keys = torch.where(t2.to(keys.device) == ex[:, None], torch.zeros_like(keys), keys)
    return restore(_count_keys(keys, lambda ky: engine.rank_count(queries, gallery_shard, ky, idx_offset=shard_start, exclude_idx=exclude_idx,
                                                                  **_filter_kw(row_filter))))


def _require_unsplit_items(items) -> None:
    """The item-level sharded helpers need every item's rows inside ONE shard.  Checked cheaply: the (min id, max id) of every shard's
    rows (ids outside [0, n_items) belong to no item) are all-gathered and must be disjoint ranges -- which contiguous items sharded at
    item boundaries give.  Every rank sees the same ranges, so every rank raises."""
    rank, world = world_info()
    if world == 1:
        return
    ids = items.items
    ids = ids[(ids >= 0) & (ids < items.n_items)]
    span = torch.tensor([int(ids.min()), int(ids.max())] if ids.numel() else [0, -1], dtype=torch.int64, device=items.items.device)
    spans = torch.empty((world, 2), dtype=torch.int64, device=span.device)
    _all_gather_into(spans, span)
    held = sorted((lo, hi, r) for r, (lo, hi) in enumerate(spans.tolist()) if hi >= lo)
    for (lo_a, hi_a, ra), (lo_b, hi_b, rb) in zip(held, held[1:]):
        if lo_b <= hi_a:
            raise ValueError(f"item ids of rank {ra} [{lo_a}, {hi_a}] and rank {rb} [{lo_b}, {hi_b}] overlap: item-level sharded ranking needs "
                             "every item's rows inside one shard (shard the gallery at item boundaries)")


def rank_items_sharded(engine, queries: torch.Tensor, gallery_shard, shard_start: int, items, k: int, exclude_idx=None, row_filter=None):
    """Gallery-sharded item-level ranking of the SAME query batch on every rank (`FernEngine.sim_topk_items` on the whole gallery).
    `items`: the SHARD's `ItemMap` (`ItemMap.rows(start, stop)`: global ids); NO ITEM MAY HAVE ROWS IN TWO SHARDS (ValueError otherwise,
    `_require_unsplit_items`).  Then a shard's list holds the true representative of every item it lists, the lists share no item and
    merge like row lists (`topk_merge`); the item ids travel beside the merge and are looked up by the merged global row index.
    Returns (scores, idx, item) on every rank."""
    _require_unsplit_items(items)
    s, i, it = engine.sim_topk_items(queries, gallery_shard, items, k, idx_offset=shard_start, exclude_idx=exclude_idx, **_filter_kw(row_filter))
    ms, mi, gathered = _gather_merge(engine, s, i, it)
    if gathered is None:
        return s, i, it
    # a global row index appears in one list only: sort each query's gathered indices once, look the merged ones up
    b, wk = s.shape[0], gathered[0].shape[0] * s.shape[1]
    cat_i, cat_t = (t.permute(1, 0, 2).reshape(b, wk) for t in gathered)
    sorted_i, perm = cat_i.to(torch.int64).sort(dim=1)
    pos = torch.searchsorted(sorted_i, mi.to(torch.int64).contiguous()).clamp(max=wk - 1)
    mt = cat_t.gather(1, perm.gather(1, pos))
    return ms, mi, torch.where(mi >= 0, mt, torch.full_like(mt, -1))


def item_rank_of_sharded(engine, queries: torch.Tensor, gallery_shard, shard_start: int, items, target_items, exclude_idx=None, row_filter=None):
    """Gallery-sharded item-level target ranks (`FernEngine.item_rank_of` on the whole gallery), under the same requirement as
    `rank_items_sharded`.  The key of a target item is its representative's, from the shard that owns the item -- every other rank
    contributes 0, so the int64 SUM all-reduce is exact -- then every rank counts the items of its shard whose representative outranks
    the key and the counts are SUM-reduced; a shard that does not own the target counts against the owner's key and so adds its items, never
    a -1.  Returns int32 shaped like `target_items` on every rank; -1 for an id outside [0, n_items) or an item without an eligible row."""
    rank, world = world_info()
    _require_unsplit_items(items)
    t2, restore = per_query(target_items, queries.shape[0], torch.int32, "target_items")
    kw = dict(idx_offset=shard_start, exclude_idx=exclude_idx, **_filter_kw(row_filter))
    if world == 1:
        return restore(engine.item_rank_of(queries, gallery_shard, items, t2, **kw))
    keys = engine.item_keys(queries, gallery_shard, items, t2, **kw)
    return restore(_count_keys(keys, lambda ky: engine.item_count(queries, gallery_shard, items, ky, **kw)))


def share_gemm_tiles(engine, src: int = 0) -> None:
    """Every rank adopts rank `src`'s GEMM tile choices (the per-shape tuner runs independently in each process; all choices
    give bit-identical results, but different tiles run at slightly different speeds and a multi-GPU step is as slow as its
    slowest rank).  Call after the warm-up that visited the shapes."""
    rank, world = world_info()
    if world == 1:
        return
    box = [engine.tuner_export() if rank == src else None]
    dist.broadcast_object_list(box, src=src)
    if rank != src:
        engine.tuner_import(box[0])


def gather_rows(x: torch.Tensor) -> torch.Tensor:
    """Concatenate equally-shaped per-rank results along dim 0 on every rank (reporting / recall on rank 0)."""
    rank, world = world_info()
    if world == 1:
        return x
    out = torch.empty((world * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    _all_gather_into(out, x)
    return out


def gather_ragged(x: torch.Tensor, objs: Optional[list] = None):
    """Per-rank results with DIFFERENT row counts (a query shard whose loader dropped unreadable items, the short last shard)
    -> their concatenation in rank order on every rank.  `objs` (one Python object per row: names, member lists) travel with
    them.  Returns `x_all` or `(x_all, objs_all)`."""
    rank, world = world_info()
    if world == 1:
        return x if objs is None else (x, list(objs))
    meta = [None] * world
    dist.all_gather_object(meta, (int(x.shape[0]), None if objs is None else list(objs)))
    counts = [m[0] for m in meta]
    per = max(counts)
    block = torch.zeros((per,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    block[: x.shape[0]] = x
    full = torch.empty((world * per,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    if per:
        _all_gather_into(full, block)
    out = torch.cat([full[r * per: r * per + c] for r, c in enumerate(counts)], dim=0)
    if objs is None:
        return out
    return out, [o for m in meta for o in m[1]]


def extract_index_features_sharded(dataset, clip_model, patch_num, device, feature_dim, batch_size: int = 32, num_workers: int = 0):
    """Gallery ENCODE sharded over the ranks (the other half of the gallery build): rank r runs the reference's
    `extract_index_features` loop (utils/utils.py:44-69) on items [r*ceil(N/W), ...) of `dataset`, then the raw features, the
    13-patch local features and the names are all-gathered so that every rank returns the same
    `(index_whole_features [N,D], index_names, index_local_features [N,P,D])` the single-GPU function returns."""
    from torch.utils.data import Subset

    from .utils import extract_index_features
    rank, world = world_info()
    n = len(dataset)
    if world == 1:
        return extract_index_features(dataset, clip_model, patch_num, device, feature_dim, batch_size, num_workers)
    start, stop, per = shard_rows(n, rank, world)
    device = torch.device(device)
    feats = torch.zeros((per, feature_dim), dtype=torch.float32, device=device)
    local = torch.zeros((per, patch_num, feature_dim), dtype=torch.float32, device=device)
    names = []
    if stop > start:
        f, names, l = extract_index_features(Subset(dataset, range(start, stop)), clip_model, patch_num, device, feature_dim,
                                             batch_size, num_workers)
        feats[: f.shape[0]] = f
        local[: l.shape[0]] = l
    all_f = torch.empty((world * per, feature_dim), dtype=torch.float32, device=device)
    all_l = torch.empty((world * per, patch_num, feature_dim), dtype=torch.float32, device=device)
    _all_gather_into(all_f, feats)
    _all_gather_into(all_l, local)
    gathered = [None] * world
    dist.all_gather_object(gathered, list(names))
    counts = [len(g) for g in gathered]
    keep = torch.cat([torch.arange(r * per, r * per + c, device=device) for r, c in enumerate(counts)]) if sum(counts) else \
        torch.empty(0, dtype=torch.long, device=device)
    return all_f[keep], [nm for g in gathered for nm in g], all_l[keep]

"""Shared body of the per-dataset harness modules.

The reference repeats the same ~100 lines per dataset (run/test/test_*.py, run/valid/validate_*.py); the
arithmetic that matters is identical and lives here once:

* query loop  (test_fiq.py:67-122): caption formatting, tokenise, encode_text x2, RAW reference-feature lookup,
  ``model(..., mode="test")``;
* rank step   (test_fiq.py:45-50): normalise gallery -> ``mode="index"`` -> cosine ranking.  The reference
  materialises ``1 - Q @ G.T`` and fully argsorts it; only ranks < 50 (51 with the CIRR reference removed) and the
  scores of <= 6 named members are consumed, so this asks the engine for top-K (+ gathered member scores) instead;
* recall      (test_fiq.py:54-60, test_cirr.py:55-80, test_200k.py:53-60): name compares on the host, percentages
  computed exactly as the reference does (float32 ``sum / len`` then ``* 100``).

Under ``torch.distributed`` (torchrun, one process per GPU) the same functions shard their work and keep their
contracts on EVERY rank: the query loop runs on this rank's contiguous slice of the relative dataset and the fused queries are
gathered (so ``generate_*_val_predictions`` still returns all Q predictions in dataset order), the gallery is fused shard by
shard + one all-gather (``distributed.build_gallery``), each rank ranks its own slice of the queries against the replicated
gallery (no per-batch collective) and the [Q, K] index rows are gathered for the recall arithmetic.  With one process nothing
changes.
"""
from __future__ import annotations

import contextlib
from collections import Counter
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch.utils.data import DataLoader, Subset

from .. import distributed as fd
from ..engine import next_from
from ..tokenizer import get_tokenizer
from ..utils import collate_fn, host_threads, make_loader

TOPK = 50


def _engine_of(model):
    eng = getattr(model, "engine", None)
    if eng is None:
        raise RuntimeError("the ranking step needs model.engine (a FernEngine): no CPU ranking fallback exists")
    return eng


def format_fiq_captions(captions) -> List[str]:
    """test_fiq.py:93-97: collated [2][B] caption lists -> 'Cap1 and cap2' per item."""
    flat = np.array(captions).T.flatten().tolist()
    return [f"{flat[i].strip('.?, ').capitalize()} and {flat[i + 1].strip('.?, ')}" for i in range(0, len(flat), 2)]


def generate_predictions(kind: str, clip_model, relative_val_dataset, model, index_names, index_features, device,
                         feature_dim, batch_size, num_workers, clip_model_name) -> Dict[str, object]:
    tokenizer = get_tokenizer(clip_model_name)
    device = torch.device(device)
    rank, world = fd.world_info()
    if world > 1:       # query data parallel: this rank's contiguous slice of the queries
        q_start, q_stop, _ = fd.shard_rows(len(relative_val_dataset), rank, world)
        relative_val_dataset = Subset(relative_val_dataset, range(q_start, q_stop))
    loader = make_loader(relative_val_dataset, batch_size, num_workers, device, collate_fn)
    name_to_row = {n: i for i, n in enumerate(index_names)}      # duplicates: last row wins, like dict(zip(...)) (:88)
    # The HIP encoder + fusion on one engine: the loop below keeps its reference shape (same batches, same arithmetic, bit-identical
    # features) but every batch is ONE asynchronous lane job of a ComposedQueryPipeline -- uploads, the RAW reference-feature
    # lookup, one text-tower pass (the reference's two encode_text calls) and mode="test" -- so the host tokenises batch i + 1 while
    # batch i's kernels run and consecutive batches overlap on three streams; the only wait is at the end of the loop.
    # FERN_HARNESS_LANES=0 keeps the plain call-by-call loop (any clip_model / model objects take that path anyway).
    pipe = _query_pipeline(clip_model, model, device)
    pipe_box = [pipe]
    pending = []
    predicted: List[torch.Tensor] = []
    target_names: List[str] = []
    reference_names: List[str] = []
    group_members: List[List[str]] = []
    def parse(batch):
        members = None
        if kind in ("fiq", "val"):
            ref_names, batch_targets, captions, ref_patch = batch
            captions = format_fiq_captions(captions)
        elif kind == "cirr":
            ref_names, batch_targets, captions, ref_patch, members = batch
            members = np.array(members).T.tolist()                                   # test_cirr.py:113
        elif kind == "shoes":
            ref_names, batch_targets, captions, ref_patch, _ = batch
        elif kind == "200k":
            _, ref_names, captions, batch_targets, _, ref_patch = batch              # test_200k.py:89
        else:
            raise ValueError(kind)
        return ref_names, batch_targets, captions, ref_patch, members

    def prepared_batches():
        """Fast path: everything the host does per batch BEFORE the engine sees it -- DataLoader iteration, caption formatting,
        tokenising, the name -> row lookup, pinning -- runs in a producer thread, a few batches ahead of the consumer (the main
        thread spends its time inside libfern calls, which release the GIL)."""
        import queue
        import threading
        q: "queue.Queue" = queue.Queue(maxsize=6)
        stop = threading.Event()

        def produce():
            try:
                for batch in loader:
                    ref_names, batch_targets, captions, ref_patch, members = parse(batch)
                    text_inputs = tokenizer(list(captions), context_length=77)
                    if not text_inputs.is_cuda and text_inputs.numel() and (int(text_inputs.min()) < 0 or int(text_inputs.max()) >= clip_model.cfg.vocab_size):
                        raise IndexError(f"token id out of range [0, {clip_model.cfg.vocab_size})")      # nn.Embedding's error in the reference
                    rows = torch.tensor([name_to_row[n] for n in ref_names], dtype=torch.int64)
                    if device.type == "cuda" and not text_inputs.is_cuda:
                        text_inputs, rows = text_inputs.pin_memory(), rows.pin_memory()
                    item = (ref_names, batch_targets, members, text_inputs, ref_patch, rows)
                    while not stop.is_set():
                        try:
                            q.put(item, timeout=0.1)
                            break
                        except queue.Full:
                            continue
                    if stop.is_set():
                        return
                last = None
            except BaseException as e:      # noqa: BLE001 -- handed to the consumer, which re-raises it
                last = e
            # the terminal item obeys the same stop / timeout protocol as the batches: a consumer that has gone away while the queue
            # is full must not leave this thread (and the loader, its worker pool and the pinned batches it holds) blocked forever
            while not stop.is_set():
                try:
                    q.put(last, timeout=0.1)
                    return
                except queue.Full:
                    continue

        t = threading.Thread(target=produce, name="fern-harness-producer", daemon=True)
        t.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:
            stop.set()

    with host_threads():
        if pipe is not None:
            window = 4 * len(pipe.engines)      # results older than this are collected: their pinned host batches (B x 13 x D fp32) go back
            for ref_names, batch_targets, members, text_inputs, ref_patch, rows in prepared_batches():
                pending.append(_submit_fuse(pipe_box, clip_model, model, device, text_inputs, ref_patch, rows, index_features))
                if len(pending) - len(predicted) > window:
                    done = pending[len(predicted)]
                    predicted.append(done.wait())
                    done.release()
                target_names.extend(batch_targets)
                reference_names.extend(ref_names)
                if members is not None:
                    group_members.extend(members)
        else:
            for batch in loader:
                ref_names, batch_targets, captions, ref_patch, members = parse(batch)
                text_inputs = tokenizer(list(captions), context_length=77)
                ref_patch = ref_patch.to(device)
                with torch.no_grad():
                    visual_emb = ref_patch.transpose(0, 1)                                   # [13,B,D]  (:101)
                    text_features, _ = clip_model.encode_text(text_inputs, visual_emb=visual_emb)              # :102
                    text_seq = clip_model.encode_text(text_inputs, mode="seq", visual_emb=visual_emb)          # :103
                    rows = torch.as_tensor([name_to_row[n] for n in ref_names], device=index_features.device)
                    ref_feats = index_features[rows]                                         # RAW gallery features (:104-107)
                    fused = model(ref_feats=ref_feats.to(device), ref_local_feats=ref_patch, text_feats=text_features.to(device),
                                  text_seq_feats=text_seq.to(device), mode="test")           # :112-118
                predicted.append(fused)
                target_names.extend(batch_targets)
                reference_names.extend(ref_names)
                if members is not None:
                    group_members.extend(members)
    if pipe is not None:
        for p in pending[len(predicted):]:
            predicted.append(p.wait())
            p.release()
    pred = torch.cat(predicted, dim=0) if predicted else torch.empty((0, feature_dim), device=device)
    if world > 1:       # every rank returns all Q predictions in dataset order, like the single-process loop
        per_row = [(t, r, group_members[i] if group_members else None) for i, (t, r) in enumerate(zip(target_names, reference_names))]
        pred, per_row = fd.gather_ragged(pred, per_row)
        target_names, reference_names = [p[0] for p in per_row], [p[1] for p in per_row]
        group_members = [p[2] for p in per_row] if any(p[2] is not None for p in per_row) else []
    return {"predicted": pred, "targets": target_names, "references": reference_names, "members": group_members}


def _query_pipeline(clip_model, model, device):
    """A 4-lane ComposedQueryPipeline (FERN_HARNESS_LANES; round 6: 4 -- one hardware queue per lane with GPU_MAX_HW_QUEUES=8, _lib.py) when the
    encoder and the fusion model are the HIP ones on ONE engine on a GPU, else None."""
    import os
    from ..clip_model import FernCLIP
    from ..engine import FernEngine
    lanes = int(os.environ.get("FERN_HARNESS_LANES", "4"))
    eng = getattr(model, "engine", None)
    if lanes < 1 or not isinstance(clip_model, FernCLIP) or not isinstance(eng, FernEngine) or clip_model.engine is not eng or device.type != "cuda":
        return None
    from ..pipeline import ComposedQueryPipeline
    # kept on the engine across calls (the reference's drivers evaluate category after category, test_fiq.py:176-190): forked
    # contexts allocate their workspaces on first use, which is worth paying once
    pipe = getattr(eng, "_harness_pipe", None)
    if pipe is None or len(pipe.engines) != lanes:
        if pipe is not None:
            pipe.close()
        pipe = eng._harness_pipe = ComposedQueryPipeline(eng, lanes=lanes)
    # A fork copies the parent's precision when it is MADE and fern_set_precision changes only the context it is called on: a caller
    # that switched the engine's precision since the last harness call (FernCLIP.set_precision / engine.set_precision) would get two of
    # every three batches at the old one.  The parent is the statement of what the caller wants.
    want = eng.precision
    if any(e.precision != want for e in pipe.engines[1:]):
        pipe.set_precision(want)
    return pipe


def _submit_fuse(pipe_box, clip_model, model, device, *args):
    """submit_fuse, rebuilding the cached pipeline once if its forks went stale (the weights were re-loaded since it was made)."""
    from .._lib import FernError
    try:
        return pipe_box[0].submit_fuse(*args)
    except FernError as e:
        if "stale" not in str(e):
            raise
        eng = model.engine
        eng._harness_pipe.close()
        eng._harness_pipe = None
        pipe_box[0] = _query_pipeline(clip_model, model, device)
        return pipe_box[0].submit_fuse(*args)


_incremental_rows: Optional[int] = None      # set by `incremental_index` (the drivers' --incremental-index ROWS)


@contextlib.contextmanager
def incremental_index(rows: Optional[int]):
    """While active, `fuse_index` builds every gallery the way a serving process grows one: fused in chunks of `rows` index rows, each
    chunk appended to a `live_gallery.LiveGallery` (`fuse_index_incremental`).  None / 0: nothing changes.  Refused under
    torch.distributed with more than one rank -- a sharded store is updated shard by shard (distributed.route_rows), not by this loop."""
    global _incremental_rows
    if rows and fd.world_info()[1] > 1:
        raise RuntimeError("--incremental-index builds the gallery in one process: it is not available under torch.distributed with world > 1")
    if rows is not None and int(rows) < 0:
        raise ValueError(f"incremental index chunk must be >= 1 rows, got {rows}")
    saved, _incremental_rows = _incremental_rows, (int(rows) if rows else None)
    try:
        yield
    finally:
        _incremental_rows = saved


def fuse_index_incremental(model, index_features, index_local_features, rows: int):
    """The fused gallery of `fuse_index` built incrementally: chunks of `rows` index rows are fused (test_fiq.py:45-46 per chunk: the
    fusion is batch-invariant) and appended to a `LiveGallery` of capacity N.  Returns the store; its `gallery()` -- a `PreparedGallery`
    over the N rows -- holds the bytes of the one-shot `fuse_index` + `prepare_gallery`."""
    from ..live_gallery import LiveGallery
    eng = _engine_of(model)
    n, d = index_features.shape
    live = LiveGallery(eng, max(int(n), 1), int(d), form="prepared", tags=False)
    for o in range(0, n, int(rows)):
        live.append(eng.index_fuse(index_features[o:o + rows], index_local_features[o:o + rows], normalize_input=True))
    return live


def fuse_index(model, index_features, index_local_features, prepared: bool = False):
    """test_fiq.py:45-46.  N ranks: each fuses ceil(N/W) rows, ONE all-gather replicates the fused gallery.  ``prepared``: under
    torch.distributed the ranking form of the gallery (`PreparedGallery`) is gathered too -- every rank prepares only its shard --
    and returned instead of the tensor (what `_ranked` would otherwise build from the whole gallery on every rank).  Inside
    `incremental_index(rows)` the gallery is grown chunk by chunk in a `LiveGallery` instead and its prepared view is returned."""
    if _incremental_rows:
        return fuse_index_incremental(model, index_features, index_local_features, _incremental_rows).gallery()
    return fd.build_gallery(_engine_of(model), index_features, index_local_features, normalize_input=True, prepared=prepared)


def _my_rows(q: int):
    rank, world = fd.world_info()
    return fd.shard_rows(q, rank, world)


def _filter_kw(row_filter, start: int, stop: int) -> dict:
    """The engine keyword of a query slice's row filter -- nothing at all when there is none, so engines that do not know the keyword
    keep working."""
    return {} if row_filter is None else {"row_filter": row_filter.rows(start, stop)}


def _ranked(model, predicted, index_fused, k, exclude=None, row_filter=None) -> np.ndarray:
    """Top-k gallery rows of every query as a host array [Q, k]: this rank ranks its slice of the queries, the index rows are
    gathered (rank order == query order).  The engine is synchronised before the result is read, so a ranking error the
    kernels can only flag (fern_sync) raises here instead of being counted as misses.  `row_filter` (`engine.RowFilter`, mask / value
    per query or scalar): every query ranks only the rows that are eligible for it."""
    eng = _engine_of(model)
    q = predicted.shape[0]
    start, stop, per = _my_rows(q)
    ex = None if exclude is None else torch.as_tensor(exclude[start:stop], dtype=torch.int32)
    if stop > start:
        # the gallery is ranked against once per evaluation, like the reference builds its index once (test_fiq.py:45-46): the
        # prepared form (bf16 pre-filter copy + its certificate) lets the engine pick the cheapest exact form of the stage
        prepared = eng.prepare_gallery(index_fused) if hasattr(eng, "prepare_gallery") and torch.is_tensor(index_fused) else index_fused
        _, idx = eng.sim_topk(predicted[start:stop], prepared, k, exclude_idx=ex, **_filter_kw(row_filter, start, stop))
    else:
        idx = torch.empty((0, k), dtype=torch.int32, device=predicted.device)
    if hasattr(eng, "sync"):
        eng.sync()
    if fd.world_info()[1] > 1:
        block = torch.full((per, k), -1, dtype=torch.int32, device=idx.device)
        block[: stop - start] = idx
        idx = fd.all_gather_shards(block, q)
    return idx.cpu().numpy()


def _pct(count: int, total: int) -> float:
    return (torch.tensor(int(count)) / total).item() * 100          # float32 tensor, like test_fiq.py:59


def _unique_rows(index_names: Sequence[str], wanted: Sequence[str], what: str) -> np.ndarray:
    counts = Counter(index_names)
    row = {n: i for i, n in enumerate(index_names)}
    for n in wanted:
        # the reference asserts exactly one ground-truth hit per ranking (test_fiq.py:56)
        assert counts.get(n, 0) == 1, f"{what} {n!r} occurs {counts.get(n, 0)} times in the index (expected exactly once)"
    return np.array([row[n] for n in wanted], dtype=np.int64)


def recalls_unique(model, predicted, index_fused, index_names, target_names, ks, row_filter=None):
    """FashionIQ / Shoes / VAL: R@k = % of queries whose (unique) target is ranked < k (`row_filter`: among the eligible rows)."""
    q = len(target_names)
    tgt = _unique_rows(index_names, target_names, "target")
    hit = _ranked(model, predicted, index_fused, max(ks), row_filter=row_filter) == tgt[:, None]
    return tuple(_pct(hit[:, :k].sum(), q) for k in ks)


def merge_galleries(index_features: Sequence[torch.Tensor], index_local_features: Sequence[torch.Tensor]):
    """Several galleries (FashionIQ's three categories, run/test/test_fiq.py:157-177) as ONE store: features and local features
    concatenated in the order given, tag of a row = the ordinal of its gallery, and the row each segment starts at."""
    sizes = [int(f.shape[0]) for f in index_features]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    tags = torch.cat([torch.full((n,), c, dtype=torch.int32) for c, n in enumerate(sizes)]) if sizes else torch.zeros(0, dtype=torch.int32)
    return torch.cat(list(index_features)), torch.cat(list(index_local_features)), tags, starts


def recalls_merged(model, predicted: Sequence[torch.Tensor], index_fused, tags: torch.Tensor, starts, index_names: Sequence[Sequence[str]],
                   target_names: Sequence[Sequence[str]], ks):
    """`recalls_unique` of every category against the MERGED, fused gallery of `merge_galleries`: all queries are ranked in one
    call, each only among the rows of its own category (tag == ordinal) -- the per-category rankings of test_fiq.py:157-177, bit for
    bit.  A target is looked up inside its category's segment, so a name may repeat across categories.  One recall tuple per category."""
    from ..engine import RowFilter
    sizes = [int(p.shape[0]) for p in predicted]
    tgt = np.concatenate([starts[c] + _unique_rows(index_names[c], target_names[c], "target") for c in range(len(sizes))]) if sizes else np.zeros(0, np.int64)
    value = torch.cat([torch.full((n,), c, dtype=torch.int32) for c, n in enumerate(sizes)])
    flt = RowFilter(tags.to(predicted[0].device), -1, value.to(predicted[0].device))      # mask: all 32 bits
    hit = _ranked(model, torch.cat(list(predicted)), index_fused, max(ks), row_filter=flt) == tgt[:, None]
    out, o = [], 0
    for n in sizes:
        out.append(tuple(_pct(hit[o:o + n, :k].sum(), n) for k in ks))
        o += n
    return out


def recalls_anyhit(model, predicted, index_fused, index_names, target_names, ks):
    """Fashion200k: gallery names are caption ids with duplicates; a hit is ANY of the top-k rows (test_200k.py:59-60)."""
    q = len(target_names)
    idx = _ranked(model, predicted, index_fused, max(ks))
    names = np.array(index_names)[idx.clip(min=0)]
    hit = (names == np.array(target_names)[:, None]) & (idx >= 0)
    return tuple(_pct((hit[:, :k].sum(1) > 0).sum(), q) for k in ks)


def items_of_names(index_names: Sequence[str]):
    """Gallery rows that share a name are one item: (int32 item id per row, the distinct names in order of first appearance)."""
    ids: Dict[str, int] = {}
    rows = np.fromiter((ids.setdefault(n, len(ids)) for n in index_names), dtype=np.int32, count=len(index_names))
    return rows, list(ids)


def recalls_items(model, predicted, index_fused, index_names, target_names, ks) -> Dict[str, float]:
    """Fashion200k at ITEM level: the items are the distinct `index_names` (many rows share a caption, test_200k.py:52-60), a query's
    ranking holds every item once, represented by its best row (FernEngine.item_rank_of), and the target item's 0-based place in it is the
    number of ITEMS in front -- not the number of rows, which `recalls_anyhit` and `target_ranks` count.  `retrieval_metrics` of those
    places: {"recall@k" ..., "median_rank", "mean_rank", "mrr"}; a target name that is not in the gallery is a miss.  Query slices go per
    rank and the places are gathered, as in `target_ranks`."""
    from ..engine import ItemMap
    eng = _engine_of(model)
    rows, names = items_of_names(index_names)
    item_of = {n: i for i, n in enumerate(names)}
    tgt = np.array([item_of.get(n, -1) for n in target_names], dtype=np.int32)
    q = len(target_names)
    start, stop, per = _my_rows(q)
    if stop > start:
        items = ItemMap(torch.from_numpy(rows).to(predicted.device), max(len(names), 1))
        places = eng.item_rank_of(predicted[start:stop], index_fused, items, torch.from_numpy(tgt[start:stop, None]))
    else:
        places = torch.empty((0, 1), dtype=torch.int32, device=predicted.device)
    if hasattr(eng, "sync"):
        eng.sync()
    if fd.world_info()[1] > 1:
        block = torch.full((per, 1), -1, dtype=torch.int32, device=places.device)
        block[: stop - start] = places
        places = fd.all_gather_shards(block, q)
    return retrieval_metrics(places.cpu().numpy(), ks)


_cirr_subset = "gather"      # set by `cirr_subset` (the CIRR driver's --subset-candidates)


@contextlib.contextmanager
def cirr_subset(mode: str):
    """While active, `recalls_cirr` calls that do not name `subset` themselves use `mode` ("gather" or "candidates")."""
    global _cirr_subset
    if mode not in ("gather", "candidates"):
        raise ValueError(f"subset must be 'gather' or 'candidates', got {mode!r}")
    saved, _cirr_subset = _cirr_subset, mode
    try:
        yield
    finally:
        _cirr_subset = saved


def recalls_cirr(model, predicted, index_fused, index_names, reference_names, target_names, group_members, subset=None):
    """CIRR: reference image removed from each ranking; global R@1/5/10/50 + subset R@1/2/3 (test_cirr.py:55-80).  `subset`: how the
    target is ranked among the query's img_set members -- "gather" (the default): the members' scores are gathered and sorted on the host,
    fp32 galleries only; "candidates": the members are the query's candidate list and the target's rank is its place in the candidate
    ranking (FernEngine.sim_topk_candidates: the ranking's own score bits, any gallery form, nothing sorted on the host)."""
    subset = _cirr_subset if subset is None else subset
    if subset not in ("gather", "candidates"):
        raise ValueError(f"subset must be 'gather' or 'candidates', got {subset!r}")
    q = len(target_names)
    eng = _engine_of(model)
    tgt = _unique_rows(index_names, target_names, "target")
    ref = _unique_rows(index_names, reference_names, "reference")
    hit = _ranked(model, predicted, index_fused, TOPK, exclude=ref) == tgt[:, None]
    glob = tuple(_pct(hit[:, :k].sum(), q) for k in (1, 5, 10, 50))
    # subset: rank the target among the query's img_set members (reference excluded) by the same scores
    row = {n: i for i, n in enumerate(index_names)}
    width = max(len(m) for m in group_members)
    member_rows = np.full((q, width), -1, dtype=np.int64)
    for i, mem in enumerate(group_members):
        rows = [row[m] for m in mem if m in row and m != reference_names[i]]
        assert rows.count(tgt[i]) == 1, "target must appear exactly once among the group members (test_cirr.py:69)"
        member_rows[i, :len(rows)] = rows
    start, stop, per = _my_rows(q)
    if subset == "candidates":
        pl = torch.full((per if fd.world_info()[1] > 1 else q, width), -1, dtype=torch.int32, device=predicted.device)
        if stop > start:
            pl[: stop - start] = eng.sim_topk_candidates(predicted[start:stop], index_fused, torch.as_tensor(member_rows[start:stop], dtype=torch.int32),
                                                         1, places=True)[2]
        pl = fd.all_gather_shards(pl, q).cpu().numpy()
        ranks = pl[member_rows == tgt[:, None]].astype(np.int64)      # the target appears exactly once among a query's members
        grp = tuple(_pct((ranks < k).sum(), q) for k in (1, 2, 3))
        return grp + glob
    sc = torch.zeros((per if fd.world_info()[1] > 1 else q, width), dtype=torch.float32, device=predicted.device)
    if stop > start:
        sc[: stop - start] = eng.gather_scores(predicted[start:stop], index_fused, torch.as_tensor(member_rows[start:stop], dtype=torch.int32))
    sc = fd.all_gather_shards(sc, q).cpu().numpy().astype(np.float64)
    ranks = np.empty(q, dtype=np.int64)
    for i in range(q):
        rows_i = np.where(member_rows[i] >= 0, member_rows[i], np.iinfo(np.int64).max)
        order = np.lexsort((rows_i, -sc[i]))                   # score desc, gallery index asc
        ranks[i] = int(np.where(member_rows[i][order] == tgt[i])[0][0])
    grp = tuple(_pct((ranks < k).sum(), q) for k in (1, 2, 3))
    return grp + glob                                          # (G@1,G@2,G@3,R@1,R@5,R@10,R@50) test_cirr.py:80


def target_ranks(model, predicted, index_fused, rows, exclude=None, row_filter=None) -> np.ndarray:
    """The 0-based place of gallery rows `rows` ([Q] or [Q, m]; -1 = no target) in every query's full ranking -- what the reference
    reads off its argsort (test_fiq.py:49-60) -- as a host int32 array [Q, m]; -1 where there is no target or the target is the
    query's excluded row.  No depth limit: the engine counts the rows that outrank each target (FernEngine.rank_of).  Query slices go
    per rank and the rows are gathered, as in `_ranked`.  `row_filter`: the place among the rows that are eligible for the query, -1 for
    a target that is not eligible itself."""
    eng = _engine_of(model)
    rows = np.asarray(rows)
    rows = (rows[:, None] if rows.ndim == 1 else rows).astype(np.int32)
    q, m = rows.shape
    start, stop, per = _my_rows(q)
    ex = None if exclude is None else torch.as_tensor(np.asarray(exclude)[start:stop], dtype=torch.int32)
    if stop > start:
        ranks = eng.rank_of(predicted[start:stop], index_fused, torch.as_tensor(rows[start:stop]), exclude_idx=ex, **_filter_kw(row_filter, start, stop))
    else:
        ranks = torch.empty((0, m), dtype=torch.int32, device=predicted.device)
    if hasattr(eng, "sync"):
        eng.sync()
    if fd.world_info()[1] > 1:
        block = torch.full((per, m), -1, dtype=torch.int32, device=ranks.device)
        block[: stop - start] = ranks
        ranks = fd.all_gather_shards(block, q)
    return ranks.cpu().numpy()


def ranking_to_depth(engine, pred, fused, depth: int, page: int = 1024, exclude_idx=None, row_filter=None) -> np.ndarray:
    """The first `depth` gallery rows of every query's full ranking as a host int32 array [Q, depth], -1 past the end of a ranking --
    the columns of the reference's argsort (test_fiq.py:49-50; what utils/visualize.py and sorted_index_names read) to any depth.
    Filled by CURSOR pages of at most `page` <= 1024 places (FernEngine.sim_topk_from + `engine.next_from`): every page continues
    where the previous one ended, nothing is sorted twice and no [Q, N] matrix is formed.  `exclude_idx` / `row_filter` as in `_ranked`."""
    if depth < 1 or not 1 <= page <= 1024:
        raise ValueError("ranking_to_depth needs depth >= 1 and 1 <= page <= 1024")
    q = pred.shape[0]
    out = np.full((q, depth), -1, dtype=np.int32)
    ex = None if exclude_idx is None else torch.as_tensor(exclude_idx, dtype=torch.int32)
    kw = {} if row_filter is None else {"row_filter": row_filter}
    cursor = torch.full((q,), -1, dtype=torch.int64)          # all ones: everything is eligible
    for lo in range(0, depth, page):
        k = min(page, depth - lo)
        scores, idx = engine.sim_topk_from(pred, fused, k, cursor, exclude_idx=ex, **kw)
        cursor = next_from(scores, idx)
        out[:, lo:lo + k] = idx.cpu().numpy()
    if hasattr(engine, "sync"):
        engine.sync()
    return out


def retrieval_metrics(ranks, ks) -> Dict[str, float]:
    """{"recall@k" ..., "median_rank", "mean_rank", "mrr"} of target ranks [Q] or [Q, m] (0-based, -1 = no target).  A query's rank is
    the best (minimum) of its valid targets -- Fashion200k's any-hit (test_200k.py:59-60); a query without a valid target is a miss
    everywhere.  Recalls are `_pct` of the queries ranked < k, i.e. bit for bit the tuples of the recall functions above.  median_rank
    and mean_rank count places from 1 over the queries that have a target; mrr is the mean of 1 / place over ALL queries."""
    r = np.asarray(ranks)
    r = (r[:, None] if r.ndim == 1 else r).astype(np.int64)
    q = r.shape[0]
    best = np.where(r >= 0, r, np.iinfo(np.int64).max).min(axis=1) if q else np.zeros(0, dtype=np.int64)
    found = best != np.iinfo(np.int64).max
    out = {f"recall@{k}": _pct(int((found & (best < k)).sum()), q) for k in ks}
    place = best[found].astype(np.float64) + 1.0
    out["median_rank"] = float(np.median(place)) if place.size else float("nan")
    out["mean_rank"] = float(place.mean()) if place.size else float("nan")
    out["mrr"] = float((1.0 / place).sum() / q) if q else float("nan")
    return out

"""Live gallery: a gallery store whose rows change in place while everything that ranks against it keeps its addresses.

The reference builds its index once per evaluation (run/test/test_fiq.py:45-46).  A serving process keeps one store for its lifetime
and its catalogue changes a few hundred rows at a time; re-preparing a million rows for that -- and re-capturing every lane graph,
whose key holds the gallery's address and shape (pipeline.py: _replay) -- is what this module avoids:

* `SlotTable`   pure host bookkeeping: which slots (rows of the store) are live, the high-water mark, lowest-free-first allocation,
                the compaction plan.  No torch device, no engine.
* `LiveGallery` the device arrays (fp32 rows, bf16 copy, the three norms, tags, item ids), allocated once, and the update calls
                (include/fern.h: fern_gallery_upsert / fern_gallery_move / fern_scatter_u32).

A slot that is free or withdrawn is hidden from every ranking by a LIVE BIT in its tag (engine.RowFilter): its row stays finite and is
never eligible.  Every result is bit for bit what a freshly prepared gallery of the same contents gives: an upserted row's bf16 copy
and norms come from fern_gallery_prepare's own device code, and the norms are folded into `meta` by maximum -- a bound that is only
ever raised stays a bound, so the certificate of the bf16 pre-filter keeps holding (`refresh()` makes it tight again).

ORDERING.  Updates and rankings are stream-ordered, never concurrent: everything here runs on the current stream, so rankings issued
on that stream afterwards see the update.  Before updating a store that pipeline lanes may still be sweeping, call
`ComposedQueryPipeline.fence()`; `submit` already waits for the caller's stream.
"""
from __future__ import annotations

import heapq
from typing import Optional, Tuple

import numpy as np


class SlotTable:
    """Which of `capacity` slots are live.  Slots are GLOBAL indices, local + `slot_offset` (a shard's table starts at its shard's first
    row), in every argument and every result.  `n` is the high-water mark as a local count: every live slot is below slot_offset + n,
    and a ranking over the first n rows sees all of them.  Free slots are handed out LOWEST FIRST -- holes left by withdrawals before
    fresh slots -- so the live rows stay dense at the bottom of the store."""

    def __init__(self, capacity: int, slot_offset: int = 0):
        capacity, slot_offset = int(capacity), int(slot_offset)
        if capacity < 1 or slot_offset < 0 or slot_offset + capacity > 1 << 31:
            raise ValueError(f"need capacity >= 1, slot_offset >= 0 and slot_offset + capacity <= 2^31, got {capacity}, {slot_offset}")
        self.capacity, self.slot_offset = capacity, slot_offset
        self.n = 0
        self.n_live = 0
        self._live = np.zeros(capacity, dtype=bool)
        self._holes: list = []          # min-heap of the free local slots below n

    def _local(self, slots, what: str) -> np.ndarray:
        """Global slots -> local int64 [m]; raises on a slot outside the table or a slot given twice."""
        a = np.asarray(slots)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError(f"{what}: slots must be a 1-D integer array, got shape {a.shape} {a.dtype}")
        a = a.astype(np.int64) - self.slot_offset
        if a.size and (a.min() < 0 or a.max() >= self.capacity):
            raise IndexError(f"{what}: slot outside [{self.slot_offset}, {self.slot_offset + self.capacity})")
        if np.unique(a).size != a.size:
            raise ValueError(f"{what}: a slot is given twice in one call")
        return a

    def _global(self, local) -> np.ndarray:
        return (np.asarray(local, dtype=np.int64) + self.slot_offset).astype(np.int32)

    def is_live(self, slots) -> np.ndarray:
        return self._live[self._local(slots, "is_live")]

    def live_slots(self) -> np.ndarray:
        """The live slots, ascending."""
        return self._global(np.nonzero(self._live)[0])

    def allocate(self, m: int) -> np.ndarray:
        """m free slots, lowest first, now live.  A table without room for all m raises and changes nothing."""
        m = int(m)
        if m < 0:
            raise ValueError("m must be >= 0")
        if m > self.capacity - self.n_live:
            raise RuntimeError(f"the table is full: {m} slots wanted, {self.capacity - self.n_live} of {self.capacity} free")
        out = [heapq.heappop(self._holes) for _ in range(min(m, len(self._holes)))]
        fresh = m - len(out)
        out.extend(range(self.n, self.n + fresh))
        self.n += fresh
        local = np.asarray(out, dtype=np.int64)
        self._live[local] = True
        self.n_live += m
        return self._global(local)

    def check_live(self, slots, what: str = "replace") -> np.ndarray:
        """The slots as local indices; raises unless every one is live and none is given twice."""
        local = self._local(slots, what)
        if not self._live[local].all():
            raise KeyError(f"{what}: slot {int(local[~self._live[local]][0]) + self.slot_offset} is not live")
        return local

    def release(self, slots) -> None:
        """Withdraw live slots: they become holes that `allocate` hands out again.  Raises (and changes nothing) on a slot that is not live."""
        local = self.check_live(slots, "withdraw")
        self._live[local] = False
        self.n_live -= local.size
        for s in local.tolist():
            heapq.heappush(self._holes, s)

    def plan_compact(self) -> Tuple[np.ndarray, np.ndarray]:
        """(src, dst): the live slots above the first n_live, highest first, paired with the holes below, lowest first.  The two sets are
        disjoint; after the moves the live rows are exactly the first n_live.  Changes nothing: `apply_compact` does."""
        src = np.nonzero(self._live[self.n_live:self.n])[0][::-1] + self.n_live
        dst = np.nonzero(~self._live[:self.n_live])[0]
        assert src.size == dst.size
        return self._global(src), self._global(dst)

    def apply_compact(self, src, dst) -> None:
        """Record that the plan of `plan_compact` was carried out."""
        s, d = self.check_live(src, "compact"), self._local(dst, "compact")
        if s.size != d.size or self._live[d].any() or (d.size and (d.max() >= self.n_live or s.min() < self.n_live)):
            raise ValueError("compact: not a plan of this table")
        self._live[s] = False
        self._live[d] = True
        self.n = self.n_live
        self._holes = []


def live_mask(live_bit: int) -> int:
    if not 0 <= int(live_bit) <= 31:
        raise ValueError(f"live_bit must be in [0, 31], got {live_bit}")
    return 1 << int(live_bit)


def check_user_tags(tags, live_bit: int) -> np.ndarray:
    """User tags as uint32 bits [m]; raises when one of them sets the live bit (the store owns it)."""
    a = np.asarray(tags)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"tags must be integers, got {a.dtype}")
    a = a.astype(np.int64)
    if a.size and (a.min() < -(1 << 31) or a.max() >= 1 << 32):
        raise ValueError("tags do not fit 32 bits")
    a = (a & 0xFFFFFFFF).astype(np.uint32)
    if a.size and (a & np.uint32(live_mask(live_bit))).any():
        raise ValueError(f"a tag sets bit {live_bit}, the store's live bit: keep it clear")
    return a


def compose_filter(mask, value, live_bit: int):
    """The caller's (mask, value) -- Python ints or integer tensors [B] -- with the live bit added to both: a row is then eligible iff it
    is live AND passes the caller's filter.  Raises when the caller's mask or value touches the live bit."""
    import torch
    live = live_mask(live_bit)
    out = []
    for name, x in (("mask", mask), ("value", value)):
        if isinstance(x, (int, np.integer)):
            bits = int(x) & 0xFFFFFFFF
            if bits & live:
                raise ValueError(f"row filter {name} touches bit {live_bit}, the store's live bit")
            out.append(bits | live)
        else:
            t = torch.as_tensor(x)
            if t.dtype == torch.uint32:
                t = t.view(torch.int32)
            if t.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
                raise ValueError(f"row filter {name} must be an int or an integer tensor, got {t.dtype}")
            t64 = t.to(torch.int64) & 0xFFFFFFFF
            if bool((t64 & live).any()):
                raise ValueError(f"row filter {name} touches bit {live_bit}, the store's live bit")
            out.append(t64 | live)
    return out[0], out[1]


_FORMS = ("prepared", "f32", "bf16")


class LiveGallery:
    """A [capacity, dim] gallery store on `engine`'s device whose rows are appended, replaced, withdrawn and compacted in place.

    form      "prepared": fp32 rows + bf16 copy + the three norms (what `engine.prepare_gallery` builds; exact ranking through the
              certified pre-filter); "f32": the fp32 rows alone; "bf16": the bf16-similarity store alone.
    tags      True: one 32-bit tag per row; bit `live_bit` belongs to the store (set while the slot is live), the rest is the caller's.
              False: no tags -- no withdrawals, no `full=True` view.
    items     None, or the number of items: one int32 item id per row (`engine.ItemMap`).
    Every array is allocated once, zeroed, so its address is stable for the store's lifetime; prefix views share the storage.
    Slots are global indices (local row + `slot_offset`), as host int32 arrays."""

    def __init__(self, engine, capacity: int, dim: int, form: str = "prepared", tags: bool = True, items: Optional[int] = None,
                 live_bit: int = 31, slot_offset: int = 0):
        import torch
        if form not in _FORMS:
            raise ValueError(f"form must be one of {_FORMS}, got {form!r}")
        if int(dim) < 4 or int(dim) % 4:
            raise ValueError(f"dim must be a positive multiple of 4, got {dim}")
        self.engine, self.form, self.dim = engine, form, int(dim)
        self.table = SlotTable(capacity, slot_offset)
        self.live_bit, self._live = int(live_bit), live_mask(live_bit)
        dev = engine.device
        cap = self.table.capacity
        self.f32 = torch.zeros((cap, self.dim), dtype=torch.float32, device=dev) if form != "bf16" else None
        self.bf16 = torch.zeros((cap, self.dim), dtype=torch.bfloat16, device=dev) if form != "f32" else None
        self.meta = torch.zeros(4, dtype=torch.float32, device=dev) if form == "prepared" else None
        self.tags = torch.zeros(cap, dtype=torch.int32, device=dev) if tags else None
        self._user_tags = np.zeros(cap, dtype=np.uint32) if tags else None      # host mirror: withdraw is one scatter, nothing read back
        self.n_items = None if items is None else int(items)
        if self.n_items is not None and self.n_items < 1:
            raise ValueError(f"items must be None or >= 1, got {items}")
        self.items = torch.zeros(cap, dtype=torch.int32, device=dev) if self.n_items is not None else None

    # ---- bookkeeping -----------------------------------------------------------------------------------------------------------
    @property
    def capacity(self) -> int:
        return self.table.capacity

    @property
    def slot_offset(self) -> int:
        return self.table.slot_offset

    @property
    def n(self) -> int:
        """High-water mark: the prefix views cover rows [0, n)."""
        return self.table.n

    @property
    def n_live(self) -> int:
        return self.table.n_live

    def _dev_slots(self, local: np.ndarray):
        import torch
        return torch.from_numpy(np.ascontiguousarray(local, dtype=np.int32)).to(self.engine.device)

    def _check_rows(self, rows, tags, items):
        """(rows, user tags or None, item ids or None) validated BEFORE any slot is taken or any kernel runs."""
        import torch
        if not isinstance(rows, torch.Tensor):
            rows = torch.as_tensor(np.asarray(rows))
        if rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [m, {self.dim}], got {tuple(rows.shape)}")
        m = rows.shape[0]
        host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)      # noqa: E731
        if tags is not None:
            if self.tags is None:
                raise ValueError("this store has no tags (tags=False)")
            tags = check_user_tags(np.broadcast_to(host(tags), (m,)), self.live_bit)
        if items is not None:
            if self.items is None:
                raise ValueError("this store has no item ids (items=None)")
            items = np.broadcast_to(host(items), (m,))
            if items.size and (items.dtype.kind not in "iu" or items.min() < -(1 << 31) or items.max() >= 1 << 31):
                raise ValueError("item ids must be integers that fit int32")
            items = items.astype(np.int32)
        return rows, tags, items

    def _write(self, local: np.ndarray, rows, tags, items, normalize: bool) -> None:
        import torch
        if local.size == 0:
            return
        sl = self._dev_slots(local)
        self.engine.gallery_upsert(rows, sl, self.f32, self.bf16, self.meta, normalize=normalize)
        if tags is not None:
            self._user_tags[local] = tags
            self.engine.scatter_u32(torch.from_numpy((tags | np.uint32(self._live)).view(np.int32)), sl, self.tags)
        if items is not None:
            self.engine.scatter_u32(torch.from_numpy(items), sl, self.items)

    # ---- updates ---------------------------------------------------------------------------------------------------------------
    def append(self, rows, tags=None, items=None, normalize: bool = False) -> np.ndarray:
        """Add rows [m, dim]; returns their slots (host int32, global).  The lowest free slots are used first.  `tags` [m] (or one value;
        default 0) are the caller's tag bits, `items` [m] the item ids (required when the store has items).  A store without room raises
        and changes nothing."""
        rows, tags, items = self._check_rows(rows, tags, items)
        m = rows.shape[0]
        if self.items is not None and items is None:
            raise ValueError("this store has item ids: give items= for the new rows")
        if self.tags is not None and tags is None:
            tags = np.zeros(m, dtype=np.uint32)
        slots = self.table.allocate(m)
        self._write(slots.astype(np.int64) - self.slot_offset, rows, tags, items, normalize)
        return slots

    def replace(self, slots, rows, tags=None, items=None, normalize: bool = False) -> None:
        """New rows for live `slots`; their tags / item ids change only when given.  Raises on a slot that is not live or given twice."""
        rows, tags, items = self._check_rows(rows, tags, items)
        local = self.table.check_live(slots, "replace")
        if local.size != rows.shape[0]:
            raise ValueError(f"{rows.shape[0]} rows for {local.size} slots")
        self._write(local, rows, tags, items, normalize)

    def withdraw(self, slots) -> None:
        """Hide live `slots` from every ranking: one scatter clears their live bit; the rows' data stays until the slots are reused."""
        import torch
        if self.tags is None:
            raise ValueError("a store without tags (tags=False) cannot withdraw rows")
        local = self.table.check_live(slots, "withdraw")
        self.table.release(slots)
        if local.size:
            self.engine.scatter_u32(torch.from_numpy(self._user_tags[local].view(np.int32)), self._dev_slots(local), self.tags)

    def compact(self) -> Tuple[np.ndarray, np.ndarray]:
        """Move the highest live rows into the holes below so that the live rows are exactly [0, n_live); returns the (src, dst) slot
        pairs (global) so the caller can renumber what it keeps about those rows.  `meta` is untouched: a move changes no norm."""
        import torch
        src, dst = self.table.plan_compact()
        if src.size:
            s, d = src.astype(np.int64) - self.slot_offset, dst.astype(np.int64) - self.slot_offset
            sd = self._dev_slots(s)
            self.engine.gallery_move(sd, self._dev_slots(d), self.f32, self.bf16, self.tags, self.items)
            if self.tags is not None:                  # the sources are free now: their live bit goes (the destinations carry it already)
                self._user_tags[d] = self._user_tags[s]
                self.engine.scatter_u32(torch.from_numpy(self._user_tags[s].view(np.int32)), sd, self.tags)
        self.table.apply_compact(src, dst)
        return src, dst

    def refresh(self) -> None:
        """Prepared form: re-run fern_gallery_prepare over rows [0, n), which makes `meta` exact again (replacements only ever raise
        it).  Results do not depend on it -- a looser bound rescoring a few more rows is all a stale maximum costs."""
        if self.meta is not None:
            self.engine.prepare_gallery(self.f32[:self.n], out=self._prepared(self.n))

    # ---- views -----------------------------------------------------------------------------------------------------------------
    def _rows(self, full: bool) -> int:
        if full and self.tags is None:
            raise ValueError("the full view needs tags (the live bit hides free slots)")
        return self.capacity if full else self.n

    def _prepared(self, rows: int):
        from .engine import PreparedGallery
        return PreparedGallery(self.f32[:rows], self.bf16[:rows], self.meta)

    def gallery(self, full: bool = False):
        """What the ranking calls take: a `PreparedGallery` / fp32 tensor / bf16 tensor over rows [0, n), or over all `capacity` rows with
        `full` -- the graph-stable view: its shape and addresses never change, free and withdrawn slots are ineligible through
        `row_filter(full=True)`.  Prefix views share the store's memory: `data_ptr()` is the same for every n."""
        rows = self._rows(full)
        if self.form == "prepared":
            return self._prepared(rows)
        return (self.f32 if self.form == "f32" else self.bf16)[:rows]

    def row_filter(self, mask=0, value=0, full: bool = False):
        """The `RowFilter` that goes with `gallery(full)`: the caller's mask / value with the live bit added to both.  None -- the
        unfiltered fast path -- only when `full` is false, nothing below n is withdrawn and no mask was asked for."""
        from .engine import RowFilter
        rows = self._rows(full)
        plain = isinstance(mask, (int, np.integer)) and isinstance(value, (int, np.integer)) and int(mask) == 0 and int(value) == 0
        if self.tags is None:
            if not plain:
                raise ValueError("this store has no tags (tags=False)")
            return None
        m, v = compose_filter(mask, value, self.live_bit)      # raises on a collision with the live bit, whichever path follows
        if plain and not full and self.table.n_live == self.table.n:
            return None
        return RowFilter(self.tags[:rows], m, v)

    def item_map(self, full: bool = False):
        from .engine import ItemMap
        if self.items is None:
            raise ValueError("this store has no item ids (items=None)")
        return ItemMap(self.items[:self._rows(full)], self.n_items)

"""Thin torch-facing wrapper over the libfern C ABI.

torch is used for what it is good at here -- device memory, streams, process groups -- and nothing
else: every op below hands raw ``data_ptr()``s of caller/torch-allocated buffers to a HIP kernel
sequence in libfern.so on torch's current stream.  There is no eager/CPU fallback: constructing an
engine without a ROCm device or without the library raises.
"""
from __future__ import annotations

import ctypes as C
import sys
from typing import Dict, Mapping, Optional

import numpy as np
import torch

from . import _lib
from .synth import ClipConfig

COMBINER_TARGET, COMBINER_DVR_GLOBAL, COMBINER_DVR_LOCAL, COMBINER_DVR_FINAL = 0, 1, 2, 3
SR_TARGET, SR_DVR = 0, 1
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RELU, EPI_BIAS_RESIDUAL = 0, 1, 2, 3
EPI_BIAS_QUICKGELU = 4      # x * sigmoid(1.702 x): accepted wherever EPI_BIAS_GELU is (include/fern.h: fern_epilogue)
ACT_GELU, ACT_QUICK_GELU = 0, 1
PART_DVR, PART_TARGET_SR, PART_TARGET_COMBINER, PART_ALL = 1, 2, 4, 7
PREC_FP32, PREC_BF16, PREC_FP8, PREC_MX8, PREC_F32X3, PREC_MX8_MLP, PREC_MX8_IMG = 0, 1, 2, 3, 4, 5, 6
QFORM_BF16, QFORM_FP8, QFORM_MX8 = 0, 1, 2
_PREC_NAMES = {"fp32": PREC_FP32, "bf16": PREC_BF16, "fp8": PREC_FP8, "mx8": PREC_MX8, "f32x3": PREC_F32X3, "mx8mlp": PREC_MX8_MLP, "mx8img": PREC_MX8_IMG}
PATCH_NUM = 13


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class PreparedGallery:
    """An fp32 gallery [N, D] together with its certified bf16 pre-filter copy (include/fern.h: fern_gallery_prepare): what
    `FernEngine.sim_topk` takes to run the ranking stage as one HBM-bound pass over the bf16 rows + exact fp32 rescoring of the few
    rows that can still be in the top-K.  Results are those of the fp32 gallery, bit for bit.  Build it once per gallery
    (`FernEngine.prepare_gallery`), like the reference builds its index once per evaluation (run/test/test_fiq.py:45-46); rebuild
    it when the gallery's contents change -- or keep the store in a `live_gallery.LiveGallery`, which changes rows in place and hands out
    `PreparedGallery` views whose addresses never move."""

    __slots__ = ("f32", "bf16", "meta")

    def __init__(self, f32: torch.Tensor, bf16: torch.Tensor, meta: torch.Tensor):
        self.f32, self.bf16, self.meta = f32, bf16, meta

    @property
    def shape(self):
        return self.f32.shape

    @property
    def dtype(self):
        return self.f32.dtype

    def float(self):
        return self.f32

    def data_ptr(self) -> int:
        return self.f32.data_ptr()

    def is_contiguous(self) -> bool:
        return True


def _bits32(x, what: str) -> torch.Tensor:
    """An integer tensor (or Python int) as int32 BITS: uint32 is reinterpreted, wider integers must fit 32 bits (signed or unsigned)."""
    t = torch.as_tensor(x)
    if t.dtype == torch.int32:
        return t
    if t.dtype == torch.uint32:
        return t.view(torch.int32)
    if t.dtype in (torch.int64, torch.int16, torch.int8, torch.uint8):
        t = t.to(torch.int64)
        if t.numel() and (int(t.min()) < -(1 << 31) or int(t.max()) >= (1 << 32)):
            raise ValueError(f"{what} does not fit 32 bits")
        return (((t & 0xFFFFFFFF) + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)
    raise ValueError(f"{what} must be an integer tensor (int32 or uint32 bits), got {t.dtype}")


class RowFilter:
    """Per-query gallery row filter (include/fern.h: fern_sim_topk_filtered): gallery row n is eligible for query b iff
    ``(tags[n] & mask[b]) == value[b]``.  `tags` [N] is one 32-bit tag per gallery row (int32 or uint32, taken as bits); `mask` and
    `value` are [B] tensors or scalars that apply to every query.  mask = value = 0 accepts every row; a value with bits outside the
    mask matches nothing.  The reference's per-category FashionIQ indexes (run/test/test_fiq.py:157-177) are tag = category,
    mask = all ones, value = the query's category; CIRR's img_set (run/test/test_cirr.py:63-66) is a group id field."""

    __slots__ = ("tags", "mask", "value")

    def __init__(self, tags, mask=0, value=0):
        self.tags = _bits32(tags, "tags")
        if self.tags.dim() != 1:
            raise ValueError(f"tags must be [N], got {tuple(self.tags.shape)}")
        self.mask, self.value = _bits32(mask, "mask"), _bits32(value, "value")
        for name, t in (("mask", self.mask), ("value", self.value)):
            if t.dim() > 1:
                raise ValueError(f"{name} must be a scalar or [B], got {tuple(t.shape)}")
        if self.mask.dim() == 1 and self.value.dim() == 1 and self.mask.shape != self.value.shape:
            raise ValueError(f"mask {tuple(self.mask.shape)} and value {tuple(self.value.shape)} must have the same length")

    def rows(self, start: int, stop: int) -> "RowFilter":
        """The filter of the query slice [start, stop): per-query masks / values are sliced, scalars and the tags stay."""
        cut = lambda t: t[start:stop] if t.dim() == 1 else t      # noqa: E731
        return RowFilter(self.tags, cut(self.mask), cut(self.value))

    def resolve(self, b: int, n: int, device):
        """(tags [n], mask [b], value [b]) as contiguous int32 tensors on `device`; raises when the shapes do not fit the call."""
        if self.tags.shape[0] != n:
            raise ValueError(f"row_filter.tags has {self.tags.shape[0]} entries, the gallery has {n} rows")
        out = [self.tags.to(device).contiguous()]
        for name, t in (("mask", self.mask), ("value", self.value)):
            if t.dim() == 1 and t.shape[0] != b:
                raise ValueError(f"row_filter.{name} must be a scalar or [B = {b}], got {tuple(t.shape)}")
            out.append((t.to(device).expand(b) if t.dim() == 0 else t.to(device)).contiguous())
        return tuple(out)

    @staticmethod
    def eligible(tags: torch.Tensor, mask: torch.Tensor, value: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
        """bool [B,m]: whether the LOCAL gallery row rows[b][j] is eligible for query b, from the resolved (tags [n], mask [B],
        value [B]).  Rows are clamped into [0, n) -- the caller knows which ones lie outside -- and nothing is eligible when n == 0."""
        n = tags.shape[0]
        if n == 0:
            return torch.zeros(rows.shape, dtype=torch.bool, device=rows.device)
        return (tags[rows.to(torch.int64).clamp(0, n - 1)] & mask[:, None]) == value[:, None]


class ItemMap:
    """Which item every gallery row belongs to (include/fern.h: fern_sim_topk_items): `items` [N] holds one integer id per row, ids in
    [0, n_items) -- Fashion200k's captions (many gallery rows share one, run/test/test_200k.py:52-60), a product's photographs.  A row
    whose id is outside that range belongs to no item and is ignored by the item-level ranking.  `n_items` defaults to max id + 1,
    computed once here (one read-back, at construction and never per call)."""

    __slots__ = ("items", "n_items")

    def __init__(self, items, n_items: Optional[int] = None):
        t = torch.as_tensor(items)
        if t.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise ValueError(f"items must be an integer tensor, got {t.dtype}")
        if t.dim() != 1:
            raise ValueError(f"items must be [N], got {tuple(t.shape)}")
        if t.dtype != torch.int32:
            if t.numel() and (int(t.min()) < -(1 << 31) or int(t.max()) >= (1 << 31)):
                raise ValueError("item ids do not fit int32")
            t = t.to(torch.int32)
        if n_items is None:
            n_items = int(t.max()) + 1 if t.numel() else 1
        n_items = int(n_items)
        if n_items < 1:
            raise ValueError(f"n_items must be >= 1, got {n_items}")
        self.items, self.n_items = t.contiguous(), n_items

    def rows(self, start: int, stop: int) -> "ItemMap":
        """The map of the gallery rows [start, stop) (a shard): ids stay global, n_items stays."""
        return ItemMap(self.items[start:stop], self.n_items)

    def resolve(self, n: int, device) -> torch.Tensor:
        """The ids as a contiguous int32 tensor on `device`; raises when the gallery has another number of rows."""
        if self.items.shape[0] != n:
            raise ValueError(f"items has {self.items.shape[0]} entries, the gallery has {n} rows")
        return self.items.to(device).contiguous()


def ranking_keys(scores: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """int64 bits of the public 64-bit ranking key (include/fern.h: fern_rank_keys) of every slot of a top-K result:
    ``orderable(score) << 32 | (0xFFFFFFFF - idx)`` with `idx` the global row index -- score descending, index ascending as one unsigned
    compare.  An unfilled slot (idx < 0) gives 0.  Computed in torch on the result's device."""
    bits = scores.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    order = torch.where(bits >= 0x80000000, bits ^ 0xFFFFFFFF, bits | 0x80000000)
    gi = idx.to(torch.int64)
    keys = (order << 32) | (0xFFFFFFFF - gi.clamp(min=0))
    return torch.where(gi >= 0, keys, torch.zeros_like(keys))


def next_from(scores: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """int64 [B]: the cursor of the page that follows the result (scores, idx) [B,k] -- what `FernEngine.sim_topk_from` takes as
    `from_keys`: the key of the last FILLED place minus 1 (keys are unique per row, so nothing lies between them); 0, which makes
    nothing eligible, when the page has no filled place."""
    keys = ranking_keys(scores, idx)
    filled = (idx >= 0).sum(dim=1)
    last = keys.gather(1, (filled - 1).clamp(min=0)[:, None])[:, 0]
    return torch.where(filled > 0, last - 1, torch.zeros_like(last))


def per_query(t, b: int, dtype, what: str, device=None):
    """(t2, restore): a per-query argument given as [B] or [B,m] (`targets`, `places`, `keys`) as a contiguous [B,m] tensor of `dtype`
    (moved to `device` when one is given), and the function that gives a [B,m] result the caller's shape back (column 0 of it when `t`
    was flat)."""
    t = torch.as_tensor(t).to(device=device, dtype=dtype)
    flat = t.dim() == 1
    if flat:
        t = t[:, None]
    if t.dim() != 2 or t.shape[0] != b or t.shape[1] < 1:
        raise ValueError(f"{what} must be [B] or [B,m] with m >= 1, got {tuple(t.shape)}")
    return t.contiguous(), (lambda out: out[:, 0] if flat else out)


_NO_ITEMS = object()      # `_rank_call(items=...)` of a wrapper that takes no ItemMap: None is refused like any other non-ItemMap


class _RankCall:
    """What the arguments every ranking wrapper shares resolve to (`FernEngine._rank_call`): the fp32 queries and the gallery's forms,
    B / N / D, the converted `exclude_idx`, the resolved filter (`tags`, `mask`, `value`: all None without one) and, with an `ItemMap`,
    the resolved ids and `n_items` -- and the two argument runs the entry points of include/fern.h share."""

    __slots__ = ("eng", "q", "g32", "g16", "meta", "b", "n", "d", "ex", "tags", "mask", "value", "items", "n_items")

    def head(self, prepared: bool = False):
        """The leading (ctx, q, gallery, gallery_bf16, B, N, D).  An entry point without `meta` ranks a PreparedGallery on its fp32 rows
        and is not handed the bf16 copy; `prepared`: the (..., gallery_bf16, meta, B, N, D) of the entry points that take all three."""
        if prepared:
            return (self.eng._h, _ptr(self.q), _ptr(self.g32), _ptr(self.g16), _ptr(self.meta), self.b, self.n, self.d)
        return (self.eng._h, _ptr(self.q), _ptr(self.g32), _ptr(self.g16 if self.g32 is None else None), self.b, self.n, self.d)

    @property
    def tail(self):
        """The trailing (tags, mask, value, stream) of every entry point that takes a filter."""
        return (_ptr(self.tags), _ptr(self.mask), _ptr(self.value), _stream())


class FernEngine:
    """One native context on one GPU.  Not thread-safe (one per device per process)."""

    def __init__(self, device="cuda:0"):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("FernEngine needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"FernEngine runs on a GPU only, got device {device!r}")
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        h = C.c_void_p()
        _lib.check(self.lib.fern_ctx_create(index, C.byref(h)), "fern_ctx_create")
        self._h = h
        self.feature_dim: Optional[int] = None
        self.clip_cfg: Optional[ClipConfig] = None

    def fork(self) -> "FernEngine":
        """A context that shares this engine's finalised weights (no copy) but owns its workspace: use one per extra
        HIP stream.  Keep the parent alive (the fork holds a reference) and fork again after re-loading weights."""
        child = object.__new__(FernEngine)
        child.lib, child.device = self.lib, self.device
        child.feature_dim, child.clip_cfg = self.feature_dim, self.clip_cfg
        child._parent = self
        h = C.c_void_p()
        _lib.check(self.lib.fern_ctx_fork(self._h, C.byref(h)), "fern_ctx_fork")
        child._h = h
        return child

    def set_precision(self, precision) -> None:
        """Operand precision of the CLIP towers' token-level GEMMs: "fp32" (parity mode, default), "bf16", "fp8" (per-row
        scales), "mx8" (block-scaled fp8 on the scaled MFMA; "mx8mlp": only the image tower's MLP pair, "mx8img": the image tower's
        four GEMMs over the fp32 residual stream -- both with a bf16 text tower; bench.py's c5 default is "mx8img") -- or "f32x3": fp32 data, every large plain GEMM computed from three
        bf16 planes per operand (fp32-accurate, ~1.4x faster, not the bit-exact fma chain) -- include/fern.h:fern_precision."""
        prec = _PREC_NAMES[precision] if isinstance(precision, str) else int(precision)
        _lib.check(self.lib.fern_set_precision(self._h, prec), "fern_set_precision")

    @property
    def precision(self) -> str:
        return {v: k for k, v in _PREC_NAMES.items()}[self.lib.fern_get_precision(self._h)]

    def close(self):
        pipe = getattr(self, "_harness_pipe", None)      # forks of this context (run/_common.py keeps a query pipeline here) go first
        if pipe is not None:
            self._harness_pipe = None
            try:
                pipe.close()
            except Exception:
                pass
        if getattr(self, "_h", None):
            self.lib.fern_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        # At interpreter shutdown the HIP runtime (and a profiler's tool library) may already be finalised: calling
        # hipDeviceSynchronize / hipFree then can block forever.  The OS reclaims the context with the process.
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    # ---- tensors ------------------------------------------------------------------------------
    def _f32(self, t, shape=None) -> torch.Tensor:
        """The tensor as a contiguous fp32 tensor on this engine's device.  A tensor that already is one is passed through
        untouched (the hot path); anything else (host tensors as the reference's loaders yield them, other dtypes, numpy)
        is converted -- an H2D copy per call, which a caller on the hot path avoids by keeping its tensors on the device."""
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if not (t.device == self.device and t.dtype == torch.float32 and t.is_contiguous()):
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _empty(self, *shape, dtype=torch.float32) -> torch.Tensor:
        return torch.empty(*shape, dtype=dtype, device=self.device)

    # ---- weights ------------------------------------------------------------------------------
    def load_tensors(self, state_dict: Mapping[str, object], prefix: str = "") -> None:
        """Push a state dict (reference key names; torch tensors or numpy arrays) to the native side."""
        for key, val in state_dict.items():
            if isinstance(val, torch.Tensor):
                val = val.detach().cpu().numpy()
            arr = np.asarray(val)
            if arr.dtype.kind == "f":
                arr, dt = np.ascontiguousarray(arr, dtype=np.float32), 0
            else:
                arr, dt = np.ascontiguousarray(arr, dtype=np.int64), 1
            shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
            _lib.check(self.lib.fern_load_tensor(self._h, (prefix + key).encode(), arr.ctypes.data_as(C.c_void_p), dt,
                                                 arr.ndim, shape), f"fern_load_tensor({key})")

    def finalize_fusion(self, feature_dim: int, parts: int = PART_ALL) -> None:
        _lib.check(self.lib.fern_finalize_fusion(self._h, int(feature_dim), int(parts)), "fern_finalize_fusion")
        self.feature_dim = int(feature_dim)

    def finalize_clip(self, cfg: ClipConfig) -> None:
        cc = _lib.ClipConfigC(cfg.embed_dim, cfg.image_size, cfg.patch_size, cfg.v_width, cfg.v_layers, cfg.v_heads,
                              cfg.v_mlp, cfg.context_length, cfg.vocab_size, cfg.t_width, cfg.t_heads, cfg.t_layers, cfg.t_mlp,
                              1 if cfg.v_arch == "resnet" else 0, (C.c_int * 4)(*cfg.r_layers), cfg.r_width, cfg.r_heads)
        _lib.check(self.lib.fern_finalize_clip(self._h, C.byref(cc)), "fern_finalize_clip")
        self.set_clip_activation(ACT_QUICK_GELU if getattr(cfg, "quick_gelu", False) else ACT_GELU)
        self.clip_cfg = cfg

    def set_clip_activation(self, act: int) -> None:
        """MLP activation of both CLIP towers (ACT_GELU / ACT_QUICK_GELU); `finalize_clip` sets it from `cfg.quick_gelu`.  Forks follow."""
        _lib.check(self.lib.fern_clip_set_activation(self._h, int(act)), "fern_clip_set_activation")

    # ---- encoders -----------------------------------------------------------------------------
    def encode_image(self, images: torch.Tensor) -> torch.Tensor:
        cfg = self.clip_cfg
        if cfg is None:
            raise _lib.FernError("encode_image: CLIP weights not finalised")
        x = self._f32(images)
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, cfg.image_size, cfg.image_size):
            raise ValueError(f"images must be [b,3,{cfg.image_size},{cfg.image_size}], got {tuple(x.shape)}")
        out = self._empty(x.shape[0], cfg.embed_dim)
        _lib.check(self.lib.fern_vit_encode_image(self._h, _ptr(x), _ptr(out), x.shape[0], _stream()), "fern_vit_encode_image")
        return out

    def encode_text(self, tokens: torch.Tensor, want_global=True, want_seq=True, visual_emb: Optional[torch.Tensor] = None):
        """tokens int64 [B,ctx] -> (global [B,D] | None, seq [B,ctx,D] | None).  `visual_emb` [13,B,D] is the reference's
        argument of that name (models/clip_model.py:23-31): shape-checked by the library, values unused.  Token ids outside
        the vocabulary raise IndexError like nn.Embedding when the tokens are on the host (as the reference's tokenizer leaves
        them, test_fiq.py:98); for device tokens the library flags them at the next sync / encode_text (no sync here)."""
        cfg = self.clip_cfg
        if cfg is None:
            raise _lib.FernError("encode_text: CLIP weights not finalised")
        if tokens.dim() != 2 or tokens.shape[1] != cfg.context_length:
            raise ValueError(f"text must be int64 [B,{cfg.context_length}], got {tuple(tokens.shape)}")
        if not tokens.is_cuda and tokens.numel() and (int(tokens.min()) < 0 or int(tokens.max()) >= cfg.vocab_size):
            raise IndexError(f"token id out of range [0, {cfg.vocab_size}): min {int(tokens.min())}, max {int(tokens.max())}")
        t = tokens.to(device=self.device, dtype=torch.int64).contiguous()
        b = t.shape[0]
        ve, ve_shape = None, None
        if visual_emb is not None:
            if visual_emb.dim() != 3:
                raise ValueError(f"visual_emb must be [{PATCH_NUM}, B, {cfg.embed_dim}], got {tuple(visual_emb.shape)}")
            ve = visual_emb if visual_emb.is_cuda else visual_emb.to(self.device)      # only its address and shape cross the ABI
            ve_shape = (C.c_int64 * 3)(*visual_emb.shape)
        g = self._empty(b, cfg.embed_dim) if want_global else None
        s = self._empty(b, cfg.context_length, cfg.embed_dim) if want_seq else None
        _lib.check(self.lib.fern_text_encode(self._h, _ptr(t), _ptr(ve), ve_shape, _ptr(g), _ptr(s), b, _stream()), "fern_text_encode")
        return g, s

    def encode_pair(self, images: torch.Tensor, tokens: torch.Tensor, want_seq: bool = True):
        """`encode_image(images)` and `encode_text(tokens)` of the SAME query batch in one pass (include/fern.h: fern_encode_pair): the towers
        are walked layer by layer and the text layer's GEMMs ride in the image layer's launches.  Returns (image [B,D], text global [B,D],
        text seq [B,ctx,D] | None) -- bit-identical to the two calls; in a mode or with a tower the library does not pair, it makes them."""
        cfg = self.clip_cfg
        if cfg is None:
            raise _lib.FernError("encode_pair: CLIP weights not finalised")
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, cfg.image_size, cfg.image_size):
            raise ValueError(f"images must be [b,3,{cfg.image_size},{cfg.image_size}], got {tuple(images.shape)}")
        if tokens.dim() != 2 or tokens.shape[1] != cfg.context_length or tokens.shape[0] != images.shape[0]:
            raise ValueError(f"text must be int64 [{images.shape[0]},{cfg.context_length}], got {tuple(tokens.shape)}")
        if not tokens.is_cuda and tokens.numel() and (int(tokens.min()) < 0 or int(tokens.max()) >= cfg.vocab_size):
            raise IndexError(f"token id out of range [0, {cfg.vocab_size}): min {int(tokens.min())}, max {int(tokens.max())}")
        x = self._f32(images)
        t = tokens.to(device=self.device, dtype=torch.int64).contiguous()
        b = x.shape[0]
        out = self._empty(b, cfg.embed_dim)
        g = self._empty(b, cfg.embed_dim)
        s = self._empty(b, cfg.context_length, cfg.embed_dim) if want_seq else None
        _lib.check(self.lib.fern_encode_pair(self._h, _ptr(x), _ptr(t), _ptr(out), _ptr(g), _ptr(s), b, _stream()), "fern_encode_pair")
        return out, g, s

    # ---- fusion -------------------------------------------------------------------------------
    def _d(self) -> int:
        if self.feature_dim is None:
            raise _lib.FernError("fusion weights not finalised")
        return self.feature_dim

    def dvr_fuse(self, ref_global, ref_local, text_global, text_seq) -> torch.Tensor:
        d = self._d()
        rl = self._f32(ref_local)
        b = rl.shape[0]
        ts = self._f32(text_seq)
        if rl.dim() != 3 or rl.shape[1] != PATCH_NUM or rl.shape[2] != d:
            raise ValueError(f"ref_local_feats must be [B,{PATCH_NUM},{d}], got {tuple(rl.shape)}")
        if ts.dim() != 3 or ts.shape[0] != b or ts.shape[2] != d:
            raise ValueError(f"text_seq_feats must be [B,T,{d}], got {tuple(ts.shape)}")
        if ts.shape[1] < PATCH_NUM:      # fusion_model.py:47 keeps 13 text-query rows for BatchNorm1d(13)
            raise ValueError(f"text_seq_feats needs at least {PATCH_NUM} token rows, got {ts.shape[1]}")
        rg, tg = self._f32(ref_global, (b, d)), self._f32(text_global, (b, d))
        out = self._empty(b, d)
        _lib.check(self.lib.fern_dvr_fuse(self._h, _ptr(rg), _ptr(rl), _ptr(tg), _ptr(ts), _ptr(out), b, ts.shape[1],
                                          _stream()), "fern_dvr_fuse")
        return out

    def index_fuse(self, tar_feats, tar_local, normalize_input=False) -> torch.Tensor:
        d = self._d()
        tl = self._f32(tar_local)
        n = tl.shape[0]
        if tl.dim() != 3 or tl.shape[1] != PATCH_NUM or tl.shape[2] != d:
            raise ValueError(f"tar_local_feats must be [n,{PATCH_NUM},{d}], got {tuple(tl.shape)}")
        tf = self._f32(tar_feats, (n, d))
        out = self._empty(n, d)
        _lib.check(self.lib.fern_index_fuse(self._h, _ptr(tf), _ptr(tl), _ptr(out), n, int(bool(normalize_input)), _stream()),
                   "fern_index_fuse")
        return out

    def combiner(self, which: int, image, text) -> torch.Tensor:
        d = self._d()
        im = self._f32(image)
        if im.dim() != 2 or im.shape[1] != d:
            raise ValueError(f"image_features must be [n,{d}], got {tuple(im.shape)}")
        tx = self._f32(text, tuple(im.shape))
        out = self._empty(*im.shape)
        _lib.check(self.lib.fern_combiner(self._h, which, _ptr(im), _ptr(tx), _ptr(out), im.shape[0], _stream()), "fern_combiner")
        return out

    def visual_sr(self, which: int, local) -> torch.Tensor:
        d = self._d()
        x = self._f32(local)
        if x.dim() != 3 or x.shape[1] != PATCH_NUM or x.shape[2] != d:
            raise ValueError(f"local_feature must be [n,{PATCH_NUM},{d}], got {tuple(x.shape)}")
        out = self._empty(x.shape[0], d)
        _lib.check(self.lib.fern_visual_sr(self._h, which, _ptr(x), _ptr(out), x.shape[0], _stream()), "fern_visual_sr")
        return out

    def finalize_clip4cir(self) -> None:
        _lib.check(self.lib.fern_finalize_clip4cir(self._h), "fern_finalize_clip4cir")

    def combiner_clip4cir(self, image, text) -> torch.Tensor:
        im = self._f32(image)
        tx = self._f32(text, tuple(im.shape))
        out = torch.empty_like(im)
        _lib.check(self.lib.fern_combiner_clip4cir(self._h, _ptr(im), _ptr(tx), _ptr(out), im.shape[0], _stream()), "fern_combiner_clip4cir")
        return out

    def element_wise_sum(self, image, text) -> torch.Tensor:
        im = self._f32(image)
        tx = self._f32(text, tuple(im.shape))
        out = torch.empty_like(im)
        _lib.check(self.lib.fern_element_wise_sum(self._h, _ptr(im), _ptr(tx), _ptr(out), im.shape[0], im.shape[1], _stream()),
                   "fern_element_wise_sum")
        return out

    def l2_normalize(self, x) -> torch.Tensor:
        x = self._f32(x)
        out = torch.empty_like(x)
        _lib.check(self.lib.fern_l2_normalize(self._h, _ptr(x), _ptr(out), x.shape[0], x.shape[1], _stream()), "fern_l2_normalize")
        return out

    # ---- rank ---------------------------------------------------------------------------------
    def prepare_gallery(self, gallery, out: Optional[PreparedGallery] = None) -> PreparedGallery:
        """fp32 [N,D] -> PreparedGallery (the gallery itself, its bf16 copy, the three norms that certify the copy as a pre-filter).
        `out`: a PreparedGallery of the same shape to refill in place (a serving process's store)."""
        g = self._f32(gallery)
        if g.dim() != 2 or g.shape[1] % 4:
            raise ValueError(f"gallery must be [N,D] with D % 4 == 0, got {tuple(g.shape)}")
        if out is not None and tuple(out.bf16.shape) == tuple(g.shape):
            b16, meta = out.bf16, out.meta
        else:
            b16 = torch.empty(g.shape, dtype=torch.bfloat16, device=self.device)
            meta = torch.zeros(4, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fern_gallery_prepare(self._h, _ptr(g), g.shape[0], g.shape[1], _ptr(b16), _ptr(meta), _stream()), "fern_gallery_prepare")
        return PreparedGallery(g, b16, meta)

    def _exclude(self, exclude_idx, b: int):
        if exclude_idx is None:
            return None
        ex = torch.as_tensor(exclude_idx).to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(ex.shape) != (b,):
            raise ValueError("exclude_idx must be [B]")
        return ex

    def _gallery_forms(self, q, gallery, bf16_ok: bool = True):
        """(q, g32, g16, meta): the queries as fp32 [B,D] and the forms of `gallery` -- a `PreparedGallery` gives all three, a bf16
        device tensor g16 alone (`bf16_ok`; without it a bf16 tensor is converted like any other), anything else g32 alone.  q and
        the gallery share D."""
        q = self._f32(q)
        g32 = g16 = meta = None
        if isinstance(gallery, PreparedGallery):
            g32, g16, meta = gallery.f32, gallery.bf16, gallery.meta
        elif bf16_ok and isinstance(gallery, torch.Tensor) and gallery.dtype == torch.bfloat16:
            if not gallery.is_cuda or not gallery.is_contiguous():
                raise ValueError("a bf16 gallery must be a contiguous device tensor")
            g16 = gallery
        else:
            g32 = self._f32(gallery)
        g = g32 if g32 is not None else g16
        if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
            raise ValueError(f"q [B,D] and gallery [N,D] must share D, got {tuple(q.shape)} and {tuple(g.shape)}")
        return q, g32, g16, meta

    def _topk_out(self, b: int, k: int):
        """The (scores fp32, idx int32) [B,k] outputs of a top-K call."""
        return self._empty(b, k), self._empty(b, k, dtype=torch.int32)

    def _rank_call(self, q, gallery, exclude_idx=None, row_filter=None, items=_NO_ITEMS, bf16_ok: bool = True) -> _RankCall:
        """The arguments every ranking wrapper shares, resolved once (`_RankCall`): what is left to a wrapper is its own extra
        argument, its outputs and one library call.  The only place that checks the filter's (and the item map's) type."""
        if items is not _NO_ITEMS and not isinstance(items, ItemMap):
            raise TypeError("items must be an ItemMap")
        if row_filter is not None and not isinstance(row_filter, RowFilter):
            raise TypeError("row_filter must be a RowFilter")
        c = _RankCall()
        c.eng = self
        c.q, c.g32, c.g16, c.meta = self._gallery_forms(q, gallery, bf16_ok)
        c.b, (c.n, c.d) = c.q.shape[0], (c.g32 if c.g32 is not None else c.g16).shape
        c.items, c.n_items = (None, 0) if items is _NO_ITEMS else (items.resolve(c.n, self.device), items.n_items)
        c.tags, c.mask, c.value = (None, None, None) if row_filter is None else row_filter.resolve(c.b, c.n, self.device)
        c.ex = self._exclude(exclude_idx, c.b)
        return c

    def _sim_topk_filtered(self, q, gallery, k: int, idx_offset, exclude_idx, row_filter: RowFilter):
        """The filtered form of `sim_topk` / `sim_topk_deep` / `sim_topk_bf16` (include/fern.h: fern_sim_topk_filtered): the exact
        ranking of the rows that are eligible for each query, 1 <= k <= 1024, any gallery form."""
        c = self._rank_call(q, gallery, exclude_idx, row_filter)
        scores, idx = self._topk_out(c.b, k)
        _lib.check(self.lib.fern_sim_topk_filtered(*c.head(prepared=True), int(k), _ptr(scores), _ptr(idx), int(idx_offset), _ptr(c.ex),
                                                   *c.tail), "fern_sim_topk_filtered")
        return scores, idx

    def sim_topk(self, q, gallery, k: int, idx_offset: int = 0, exclude_idx=None, row_filter: Optional[RowFilter] = None):
        """Exact cosine top-K of q [B,D] against an fp32 gallery [N,D] (run/test/test_fiq.py:49-50).  `gallery` is a tensor -- the
        fp32-MFMA sweep -- or a `PreparedGallery` -- bf16 pre-filter + exact rescoring, same scores and ordering bit for bit.
        `row_filter`: rank only the rows that are eligible for each query (`RowFilter`)."""
        if row_filter is not None:
            return self._sim_topk_filtered(q, gallery, k, idx_offset, exclude_idx, row_filter)
        if isinstance(gallery, PreparedGallery):
            return self._sim_topk_prefiltered(q, gallery, k, idx_offset, exclude_idx)
        c = self._rank_call(q, gallery, exclude_idx, bf16_ok=False)
        scores, idx = self._topk_out(c.b, k)
        _lib.check(self.lib.fern_sim_topk(self._h, _ptr(c.q), _ptr(c.g32), c.b, c.n, c.d, int(k), _ptr(scores), _ptr(idx),
                                          int(idx_offset), _ptr(c.ex), _stream()), "fern_sim_topk")
        return scores, idx

    def sweep_bf16_scores(self, q, pg: "PreparedGallery", tile_max: bool = True):
        """The pre-filter's approximate scores [B,N] (bf16 operands, fp32 accumulation) and, with `tile_max`, the largest score of
        every 32 consecutive gallery rows [B, ceil(N/32)] -- what the dense form of the ranking stage selects on
        (include/fern.h: fern_sweep_bf16_scores)."""
        q = self._f32(q)
        n, d = pg.shape
        b = q.shape[0]
        scores = self._empty(b, n)
        nt = (n + 31) // 32
        tmax = self._empty(b, nt) if tile_max else None
        _lib.check(self.lib.fern_sweep_bf16_scores(self._h, _ptr(q), _ptr(pg.bf16), b, n, d, _ptr(scores), n, _ptr(tmax), nt, _stream()),
                   "fern_sweep_bf16_scores")
        return (scores, tmax) if tile_max else scores

    def set_rank_strategy(self, strategy) -> None:
        """Form of the PreparedGallery ranking stage: "auto" (cost model), "plain" (fp32 sweep), "lists", "dense" -- identical results
        (include/fern.h: fern_rank_strategy); a tuning / test knob."""
        code = {"auto": 0, "plain": 1, "lists": 2, "dense": 3}[strategy] if isinstance(strategy, str) else int(strategy)
        _lib.check(self.lib.fern_rank_set_strategy(self._h, code), "fern_rank_set_strategy")

    def _sim_topk_prefiltered(self, q, pg: PreparedGallery, k: int, idx_offset: int = 0, exclude_idx=None):
        c = self._rank_call(q, pg, exclude_idx)
        scores, idx = self._topk_out(c.b, k)
        _lib.check(self.lib.fern_sim_topk_prefiltered(*c.head(prepared=True), int(k), _ptr(scores), _ptr(idx), int(idx_offset), _ptr(c.ex),
                                                      _stream()), "fern_sim_topk_prefiltered")
        return scores, idx

    def sim_topk_deep(self, q, gallery, k: int, idx_offset: int = 0, exclude_idx=None, row_filter: Optional[RowFilter] = None):
        """Exact top-K for 1 <= k <= 1024 (include/fern.h: fern_sim_topk_deep); `sim_topk` stops at 64.  `gallery` is an fp32
        tensor (exact fp32-chain scores), a `PreparedGallery` (the same bits through the certified bf16 pre-filter) or a bf16
        tensor (the bf16 similarity of `sim_topk_bf16`).  For k' <= 64 the first k' columns equal those of the K <= 64 call.
        `row_filter`: rank only the rows that are eligible for each query (`RowFilter`)."""
        if row_filter is not None:
            return self._sim_topk_filtered(q, gallery, k, idx_offset, exclude_idx, row_filter)
        c = self._rank_call(q, gallery, exclude_idx)
        scores, idx = self._topk_out(c.b, k)
        _lib.check(self.lib.fern_sim_topk_deep(*c.head(prepared=True), int(k), _ptr(scores), _ptr(idx), int(idx_offset), _ptr(c.ex),
                                               _stream()), "fern_sim_topk_deep")
        return scores, idx

    def sim_topk_candidates(self, q, gallery, candidates, k: int, idx_offset: int = 0, exclude_idx=None,
                            row_filter: Optional[RowFilter] = None, places: bool = False):
        """(scores, idx) [B,k], with `places` also place int32 [B,M]: every query ranked inside its own list of gallery rows
        (include/fern.h: fern_sim_topk_candidates; run/test/test_cirr.py:55-69 ranks inside a named member set).  `candidates` [B,M]
        holds global row indices (a tensor, numpy array or list; 1 <= M <= 4096); an entry that is negative, outside this gallery
        (shard), the query's excluded row or ineligible under `row_filter` takes no place, a row named twice counts once.  Scores and
        order are those of `sim_topk_deep` on the same gallery form (fp32 tensor or `PreparedGallery`: the fp32 chain; bf16 tensor: the
        bf16 similarity); 1 <= k <= 1024, places past the list are -inf / -1.  place[b][j]: the 0-based place of entry j, -1 if none."""
        c = self._rank_call(q, gallery, exclude_idx, row_filter)
        cd = torch.as_tensor(candidates)
        if cd.dim() != 2 or cd.shape[0] != c.b or cd.dtype.is_floating_point or cd.dtype == torch.bool:
            raise ValueError(f"candidates must be an integer [B = {c.b}, M], got {tuple(cd.shape)} {cd.dtype}")
        cd = cd.to(device=self.device, dtype=torch.int32).contiguous()
        scores, idx = self._topk_out(c.b, k)
        place = self._empty(*cd.shape, dtype=torch.int32) if places else None
        _lib.check(self.lib.fern_sim_topk_candidates(*c.head(), _ptr(cd), cd.shape[1], int(k), _ptr(scores), _ptr(idx), _ptr(place),
                                                     int(idx_offset), _ptr(c.ex), *c.tail), "fern_sim_topk_candidates")
        return (scores, idx, place) if places else (scores, idx)

    # ---- exact target ranks ---------------------------------------------------------------------
    def _keys_of(self, c: _RankCall, tg: torch.Tensor, idx_offset) -> torch.Tensor:
        keys = self._empty(*tg.shape, dtype=torch.int64)
        _lib.check(self.lib.fern_rank_keys(*c.head(), _ptr(tg), tg.shape[1], int(idx_offset), _ptr(keys), _stream()), "fern_rank_keys")
        return keys

    def _count_of(self, c: _RankCall, ky: torch.Tensor, idx_offset) -> torch.Tensor:
        count = self._empty(*ky.shape, dtype=torch.int32)
        if c.tags is not None:
            _lib.check(self.lib.fern_rank_count_filtered(*c.head(), _ptr(ky), ky.shape[1], int(idx_offset), _ptr(c.ex), _ptr(count), *c.tail),
                       "fern_rank_count_filtered")
        else:
            _lib.check(self.lib.fern_rank_count(*c.head(), _ptr(ky), ky.shape[1], int(idx_offset), _ptr(c.ex), _ptr(count), _stream()),
                       "fern_rank_count")
        return count

    def rank_keys(self, q, gallery, targets, idx_offset: int = 0) -> torch.Tensor:
        """int64 [B,m]: the bits of the 64-bit ranking keys (include/fern.h: fern_rank_keys) of the gallery rows `targets` (global
        indices, [B] or [B,m]); 0 for a target < 0 or outside [idx_offset, idx_offset + N)."""
        c = self._rank_call(q, gallery)
        return self._keys_of(c, per_query(targets, c.b, torch.int32, "targets", self.device)[0], idx_offset)

    def rank_count(self, q, gallery, keys, idx_offset: int = 0, exclude_idx=None, row_filter: Optional[RowFilter] = None) -> torch.Tensor:
        """int32 [B,m]: per key the number of rows of `gallery` whose ranking key is greater (include/fern.h: fern_rank_count); the
        row `exclude_idx[b]` (global index) is not counted; -1 for a key of 0.  Counts of gallery shards add up.  `row_filter`: only
        the rows that are eligible for the query are counted (fern_rank_count_filtered)."""
        c = self._rank_call(q, gallery, exclude_idx, row_filter)
        return self._count_of(c, per_query(keys, c.b, torch.int64, "keys", self.device)[0], idx_offset)

    def rank_of(self, q, gallery, targets, idx_offset: int = 0, exclude_idx=None, row_filter: Optional[RowFilter] = None) -> torch.Tensor:
        """int32, shaped like `targets` ([B] or [B,m]): the 0-based position of each target row in the ordering `sim_topk` defines
        (score descending, gallery index ascending) -- what the reference reads off its full argsort (run/test/test_fiq.py:49-60) --
        at any depth.  -1 for a target that is < 0, outside the gallery, or the query's excluded row.  `row_filter`: the position
        among the rows that are eligible for the query; -1 for a target that is not eligible itself."""
        c = self._rank_call(q, gallery, exclude_idx, row_filter)      # everything is converted once: the two calls share it
        tg, restore = per_query(targets, c.b, torch.int32, "targets", self.device)
        keys = self._keys_of(c, tg, idx_offset)
        if c.ex is not None:
            keys = torch.where(tg == c.ex[:, None], torch.zeros_like(keys), keys)
        if c.tags is not None:          # ineligible targets lose their key on the device, like the excluded row
            ok = RowFilter.eligible(c.tags, c.mask, c.value, tg.to(torch.int64) - int(idx_offset))
            keys = torch.where(ok, keys, torch.zeros_like(keys))
        return restore(self._count_of(c, keys, idx_offset))

    # ---- ranking pages ----------------------------------------------------------------------------
    def rank_select(self, q, gallery, places, idx_offset: int = 0, exclude_idx=None, row_filter: Optional[RowFilter] = None) -> torch.Tensor:
        """int64 [B,m] ([B] for flat `places`): the bits of the ranking key of the row at each 0-based place of the ordering `sim_topk`
        defines, at any depth (include/fern.h: fern_rank_select) -- the inverse of `rank_count`; 0 for a place < 0 or past the rows that
        take a place.  `gallery`: an fp32 tensor or a `PreparedGallery` (exact fp32-chain scores) or a bf16 tensor."""
        c = self._rank_call(q, gallery, exclude_idx, row_filter)
        pl, restore = per_query(places, c.b, torch.int32, "places", self.device)
        keys = self._empty(*pl.shape, dtype=torch.int64)
        _lib.check(self.lib.fern_rank_select(*c.head(), _ptr(pl), pl.shape[1], int(idx_offset), _ptr(c.ex), _ptr(keys), *c.tail),
                   "fern_rank_select")
        return restore(keys)

    def sim_topk_from(self, q, gallery, k: int, from_keys, idx_offset: int = 0, exclude_idx=None, row_filter: Optional[RowFilter] = None):
        """(scores, idx) [B,k]: the exact top-K, 1 <= k <= 1024, among the rows whose ranking key is <= `from_keys` [B] (int64 bits; a
        cursor from `next_from`, -1 = everything, 0 = nothing) -- include/fern.h: fern_sim_topk_from.  The cursor carries a GLOBAL row
        index, so the same cursor continues the list on every shard of a gallery (`idx_offset`)."""
        c = self._rank_call(q, gallery, exclude_idx, row_filter)
        fk = torch.as_tensor(from_keys).to(device=self.device, dtype=torch.int64).contiguous()
        if tuple(fk.shape) != (c.b,):
            raise ValueError("from_keys must be [B]")
        scores, idx = self._topk_out(c.b, k)
        _lib.check(self.lib.fern_sim_topk_from(*c.head(), int(k), _ptr(fk), _ptr(scores), _ptr(idx), int(idx_offset), _ptr(c.ex), *c.tail),
                   "fern_sim_topk_from")
        return scores, idx

    def rank_page(self, q, gallery, offset, k: int, idx_offset: int = 0, exclude_idx=None, row_filter: Optional[RowFilter] = None):
        """(scores, idx) [B,k]: places [offset, offset + k) of every query's ranking, at any depth (include/fern.h: fern_sim_topk_page);
        `offset` an int or [B]; slots past the end -inf / -1.  offset 0 is `sim_topk_deep`."""
        c = self._rank_call(q, gallery, exclude_idx, row_filter)
        off = torch.as_tensor(offset).to(device=self.device, dtype=torch.int32)
        off = off.expand(c.b).contiguous() if off.dim() == 0 else off.contiguous()
        if tuple(off.shape) != (c.b,):
            raise ValueError("offset must be an int or [B]")
        scores, idx = self._topk_out(c.b, k)
        _lib.check(self.lib.fern_sim_topk_page(*c.head(), int(k), _ptr(off), _ptr(scores), _ptr(idx), int(idx_offset), _ptr(c.ex), *c.tail),
                   "fern_sim_topk_page")
        return scores, idx

    # ---- item-level ranking -----------------------------------------------------------------------
    def sim_topk_items(self, q, gallery, items: ItemMap, k: int, idx_offset: int = 0, exclude_idx=None, row_filter: Optional[RowFilter] = None):
        """Item-level exact top-K, 1 <= k <= 1024 (include/fern.h: fern_sim_topk_items): the row ranking of `sim_topk_deep` (exclude_idx
        and `row_filter` applied first) with every row but the first of its item removed.  Returns (scores, idx, item) [B,k]: the
        representative row's score, its global index and its item id; unfilled places -inf / -1 / -1.  `gallery`: an fp32 tensor or a
        `PreparedGallery` (exact fp32-chain scores) or a bf16 tensor (the bf16 similarity)."""
        c = self._rank_call(q, gallery, exclude_idx, row_filter, items)
        scores, idx = self._topk_out(c.b, k)
        item = self._empty(c.b, k, dtype=torch.int32)
        _lib.check(self.lib.fern_sim_topk_items(*c.head(), int(k), _ptr(c.items), c.n_items, _ptr(scores), _ptr(idx), _ptr(item),
                                                int(idx_offset), _ptr(c.ex), *c.tail), "fern_sim_topk_items")
        return scores, idx, item

    def item_rank_of(self, q, gallery, items: ItemMap, target_items, idx_offset: int = 0, exclude_idx=None,
                     row_filter: Optional[RowFilter] = None) -> torch.Tensor:
        """int32, shaped like `target_items` ([B] or [B,m]): the number of items that come before each target item in the ranking
        `sim_topk_items` defines, at any depth (include/fern.h: fern_item_rank); -1 for an id outside [0, n_items) or an item without
        an eligible row for the query."""
        c = self._rank_call(q, gallery, exclude_idx, row_filter, items)
        tg, restore = per_query(target_items, c.b, torch.int32, "target_items", self.device)
        ranks = self._empty(*tg.shape, dtype=torch.int32)
        _lib.check(self.lib.fern_item_rank(*c.head(), _ptr(c.items), c.n_items, _ptr(tg), tg.shape[1], int(idx_offset), _ptr(c.ex), _ptr(ranks),
                                           *c.tail), "fern_item_rank")
        return restore(ranks)

    def item_keys(self, q, gallery, items: ItemMap, target_items, idx_offset: int = 0, exclude_idx=None,
                  row_filter: Optional[RowFilter] = None) -> torch.Tensor:
        """int64 [B,m]: the bits of the ranking key of each target item's representative row in this gallery (shard); 0 when the shard
        holds no eligible row of the item (include/fern.h: fern_item_keys)."""
        c = self._rank_call(q, gallery, exclude_idx, row_filter, items)
        tg, _ = per_query(target_items, c.b, torch.int32, "target_items", self.device)
        keys = self._empty(*tg.shape, dtype=torch.int64)
        _lib.check(self.lib.fern_item_keys(*c.head(), _ptr(c.items), c.n_items, _ptr(tg), tg.shape[1], int(idx_offset), _ptr(c.ex), _ptr(keys),
                                           *c.tail), "fern_item_keys")
        return keys

    def item_count(self, q, gallery, items: ItemMap, keys, idx_offset: int = 0, exclude_idx=None,
                   row_filter: Optional[RowFilter] = None) -> torch.Tensor:
        """int32 [B,m]: per key the number of this gallery's (shard's) items whose representative's key is greater; -1 for a key of 0
        (include/fern.h: fern_item_count).  Counts of shards that share no item add up."""
        c = self._rank_call(q, gallery, exclude_idx, row_filter, items)
        ky, _ = per_query(keys, c.b, torch.int64, "keys", self.device)
        count = self._empty(*ky.shape, dtype=torch.int32)
        _lib.check(self.lib.fern_item_count(*c.head(), _ptr(c.items), c.n_items, _ptr(ky), ky.shape[1], int(idx_offset), _ptr(c.ex), _ptr(count),
                                            *c.tail), "fern_item_count")
        return count

    def gallery_to_bf16(self, gallery) -> torch.Tensor:
        """fp32 [N,D] -> bf16 [N,D] (round to nearest even) for `sim_topk_bf16`."""
        g = self._f32(gallery)
        out = torch.empty(g.shape, dtype=torch.bfloat16, device=self.device)
        _lib.check(self.lib.fern_gallery_to_bf16(self._h, _ptr(g), _ptr(out), g.shape[0], g.shape[1], _stream()), "fern_gallery_to_bf16")
        return out

    # ---- live gallery: rows of a store change in place (include/fern.h: fern_gallery_upsert; live_gallery.LiveGallery owns the slots) ----
    def _slots(self, slots, what: str = "slots") -> torch.Tensor:
        t = torch.as_tensor(slots).to(device=self.device, dtype=torch.int32).contiguous()
        if t.dim() != 1:
            raise ValueError(f"{what} must be [m], got {tuple(t.shape)}")
        return t

    @staticmethod
    def _store(f32, bf16):
        """(capacity, D) of a store given as its fp32 rows, its bf16 rows or both; the arrays are written in place, so they must already
        be contiguous device tensors of the right type."""
        for t, dt in ((f32, torch.float32), (bf16, torch.bfloat16)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.dim() == 2 and t.is_contiguous()):
                raise ValueError(f"a store array must be a contiguous [capacity, D] {dt} device tensor")
        if f32 is None and bf16 is None:
            raise ValueError("give the store's f32 rows, its bf16 rows or both")
        if f32 is not None and bf16 is not None and f32.shape != bf16.shape:
            raise ValueError(f"f32 {tuple(f32.shape)} and bf16 {tuple(bf16.shape)} must have one shape")
        return tuple((f32 if f32 is not None else bf16).shape)

    def gallery_upsert(self, rows, slots, f32=None, bf16=None, meta=None, normalize: bool = False) -> None:
        """Write rows [m, D] into slots [m] of a store IN PLACE: `f32` [capacity, D] gets the row (after `normalize`: F.normalize), `bf16` its
        round-to-nearest-even copy, and `meta` is raised to the rows' three norms (never reset) -- all forms in one launch, with the
        arithmetic of `prepare_gallery`.  A device fp32 `rows` with unit column stride is read through its row stride (no copy)."""
        cap, d = self._store(f32, bf16)
        if not (isinstance(rows, torch.Tensor) and rows.device == self.device and rows.dtype == torch.float32 and rows.dim() == 2
                and rows.stride(1) == 1 and rows.stride(0) >= rows.shape[1]):
            rows = self._f32(rows)
        if rows.dim() != 2 or rows.shape[1] != d:
            raise ValueError(f"rows must be [m, {d}], got {tuple(rows.shape)}")
        sl = self._slots(slots)
        if sl.shape[0] != rows.shape[0]:
            raise ValueError(f"{rows.shape[0]} rows for {sl.shape[0]} slots")
        _lib.check(self.lib.fern_gallery_upsert(self._h, _ptr(rows), rows.stride(0), _ptr(sl),
                                                sl.shape[0], _ptr(f32), _ptr(bf16), _ptr(meta), cap, d, int(bool(normalize)), _stream()),
                   "fern_gallery_upsert")

    def gallery_move(self, src, dst, f32=None, bf16=None, tags=None, items=None) -> None:
        """Copy row src[p] onto row dst[p] of every array given (compaction); `src` and `dst` are disjoint sets of slots."""
        cap, d = self._store(f32, bf16)
        s, t = self._slots(src, "src"), self._slots(dst, "dst")
        if s.shape != t.shape:
            raise ValueError("src and dst must have one length")
        _lib.check(self.lib.fern_gallery_move(self._h, _ptr(s), _ptr(t), s.shape[0], _ptr(f32), _ptr(bf16), _ptr(tags), _ptr(items), cap, d, _stream()),
                   "fern_gallery_move")

    def scatter_u32(self, src, slots, dst: torch.Tensor) -> None:
        """dst[slots[p]] = src[p] on 32-bit words (tags; item ids as bits); `dst` is an int32 device tensor written in place."""
        if not (isinstance(dst, torch.Tensor) and dst.is_cuda and dst.dtype == torch.int32 and dst.dim() == 1 and dst.is_contiguous()):
            raise ValueError("dst must be a contiguous int32 [capacity] device tensor")
        v = _bits32(src, "src").to(self.device).contiguous()
        sl = self._slots(slots)
        if v.shape != sl.shape:
            raise ValueError(f"{v.numel()} values for {sl.shape[0]} slots")
        _lib.check(self.lib.fern_scatter_u32(self._h, _ptr(v), _ptr(sl), sl.shape[0], _ptr(dst), dst.shape[0], _stream()), "fern_scatter_u32")

    def sim_topk_bf16(self, q, gallery_bf16: torch.Tensor, k: int, idx_offset: int = 0, exclude_idx=None, row_filter: Optional[RowFilter] = None):
        if row_filter is not None:
            return self._sim_topk_filtered(q, gallery_bf16, k, idx_offset, exclude_idx, row_filter)
        if not isinstance(gallery_bf16, torch.Tensor) or gallery_bf16.dtype != torch.bfloat16:
            raise ValueError("gallery must be a contiguous bf16 [N,D] device tensor sharing D with q")
        c = self._rank_call(q, gallery_bf16, exclude_idx)
        scores, idx = self._topk_out(c.b, k)
        _lib.check(self.lib.fern_sim_topk_bf16(self._h, _ptr(c.q), _ptr(c.g16), c.b, c.n, c.d, int(k), _ptr(scores), _ptr(idx),
                                               int(idx_offset), _ptr(c.ex), _stream()), "fern_sim_topk_bf16")
        return scores, idx

    def gather_scores(self, q, gallery, idx):
        q, g = self._f32(q), self._f32(gallery.f32 if isinstance(gallery, PreparedGallery) else gallery)
        ix = torch.as_tensor(idx).to(device=self.device, dtype=torch.int32).contiguous()
        out = self._empty(*ix.shape)
        _lib.check(self.lib.fern_gather_scores(self._h, _ptr(q), _ptr(g), _ptr(ix), _ptr(out), ix.shape[0], ix.shape[1],
                                               q.shape[1], _stream()), "fern_gather_scores")
        return out

    def topk_merge(self, scores, idx):
        s = self._f32(scores)
        ix = torch.as_tensor(idx).to(device=self.device, dtype=torch.int32).contiguous()
        r, b, k = s.shape
        os_, oi = self._empty(b, k), self._empty(b, k, dtype=torch.int32)
        _lib.check(self.lib.fern_topk_merge(self._h, _ptr(s), _ptr(ix), _ptr(os_), _ptr(oi), r, b, k, _stream()), "fern_topk_merge")
        return os_, oi

    # ---- building blocks ----------------------------------------------------------------------
    def gemm(self, a, w, bias=None, residual=None, epilogue=EPI_BIAS) -> torch.Tensor:
        a, w = self._f32(a), self._f32(w)
        m, k = a.shape
        n = w.shape[0]
        bias = None if bias is None else self._f32(bias, (n,))
        residual = None if residual is None else self._f32(residual, (m, n))
        out = self._empty(m, n)
        _lib.check(self.lib.fern_gemm(self._h, _ptr(a), k, _ptr(w), k, _ptr(bias), _ptr(residual), _ptr(out), n, m, n, k,
                                      int(epilogue), _stream()), "fern_gemm")
        return out

    def batch_classification_loss(self, predicted, target) -> torch.Tensor:
        """losses/loss.py:10-14: cross_entropy(100 * predicted @ target.T, arange(B)); returns a 0-dim device tensor."""
        p = self._f32(predicted)
        t = self._f32(target, tuple(p.shape))
        out = self._empty(1)
        _lib.check(self.lib.fern_batch_classification_loss(self._h, _ptr(p), _ptr(t), p.shape[0], p.shape[1], _ptr(out), _stream()),
                   "fern_batch_classification_loss")
        return out[0]

    def to_bf16(self, x) -> torch.Tensor:
        """fp32 [R,C] -> bf16 [R,C], round to nearest even (the conversion every bf16 operand of libfern goes through)."""
        return self.gallery_to_bf16(x)

    def gemm_bf16(self, a, w, bias=None, residual=None, epilogue=EPI_BIAS, out_bf16=False) -> torch.Tensor:
        """bf16 x bf16 -> fp32-accumulate GEMM; a [M,K] / w [N,K] are bf16 tensors (fp32 inputs are rounded first)."""
        a = a if a.dtype == torch.bfloat16 else self.to_bf16(a)
        w = w if w.dtype == torch.bfloat16 else self.to_bf16(w)
        a, w = a.to(self.device).contiguous(), w.to(self.device).contiguous()
        m, k = a.shape
        n = w.shape[0]
        bias = None if bias is None else self._f32(bias, (n,))
        residual = None if residual is None else self._f32(residual, (m, n))
        out = torch.empty(m, n, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=self.device)
        _lib.check(self.lib.fern_gemm_bf16(self._h, _ptr(a), k, _ptr(w), k, _ptr(bias), _ptr(residual), _ptr(out), n, m, n, k,
                                           int(epilogue), int(bool(out_bf16)), _stream()), "fern_gemm_bf16")
        return out

    def quantize_rows_fp8(self, x):
        """[R,C] fp32 or bf16 -> (fp8 e4m3fn bytes [R,C] as uint8, per-row scales [R]); scale = max|row| / 448."""
        x = x.to(self.device).contiguous() if x.dtype == torch.bfloat16 else self._f32(x)
        rows, d = x.shape
        y = torch.empty(rows, d, dtype=torch.uint8, device=self.device)
        sc = self._empty(rows)
        _lib.check(self.lib.fern_quantize_rows_fp8(self._h, _ptr(x), int(x.dtype == torch.bfloat16), d, _ptr(y), d, _ptr(sc), rows, d,
                                                   _stream()), "fern_quantize_rows_fp8")
        return y, sc

    def gemm_fp8(self, a8, sa, w8, sw, bias=None, residual=None, epilogue=EPI_BIAS, out_bf16=False) -> torch.Tensor:
        m, k = a8.shape
        n = w8.shape[0]
        bias = None if bias is None else self._f32(bias, (n,))
        residual = None if residual is None else self._f32(residual, (m, n))
        out = torch.empty(m, n, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=self.device)
        _lib.check(self.lib.fern_gemm_fp8(self._h, _ptr(a8), k, _ptr(sa), _ptr(w8), k, _ptr(sw), _ptr(bias), _ptr(residual), _ptr(out), n,
                                          m, n, k, int(epilogue), int(bool(out_bf16)), _stream()), "fern_gemm_fp8")
        return out

    def _mx_scales(self, d, rows, scale_rows=None, scales=None) -> torch.Tensor:
        """The uint8 [d/128, scale_rows, 4] array an MX producer writes its E8M0 bytes into: `scales` when given (written in place;
        bytes of rows >= `rows` are left as they are), else a new one with scale_rows (default: rows) rows."""
        if scales is None:
            return torch.empty(d // 128, rows if scale_rows is None else int(scale_rows), 4, dtype=torch.uint8, device=self.device)
        if (scales.dtype != torch.uint8 or scales.device != self.device or not scales.is_contiguous() or scales.dim() != 3 or
                scales.shape[0] != d // 128 or scales.shape[2] != 4 or (scale_rows is not None and scales.shape[1] != scale_rows)):
            raise ValueError(f"scales must be a contiguous uint8 [{d // 128}, scale_rows, 4] tensor on {self.device}")
        return scales

    def quantize_mx8(self, x, scale_rows=None, scales=None):
        """[R,C] fp32 or bf16 (C % 128 == 0) -> (e4m3fn bytes [R,C] as uint8, E8M0 block scales as uint8 [C/128, scale_rows, 4]):
        scale byte of (row r, 32-k block b) = scales[b // 4, r, b % 4] (include/fern.h: fern_quantize_mx8).  scale_rows >= R (default
        R); `scales`: an existing array to write into."""
        x = x.to(self.device).contiguous() if x.dtype == torch.bfloat16 else self._f32(x)
        rows, d = x.shape
        y = torch.empty(rows, d, dtype=torch.uint8, device=self.device)
        sc = self._mx_scales(d, rows, scale_rows, scales)
        _lib.check(self.lib.fern_quantize_mx8(self._h, _ptr(x), int(x.dtype == torch.bfloat16), d, _ptr(y), d, _ptr(sc), sc.shape[1], rows, d,
                                              _stream()), "fern_quantize_mx8")
        return y, sc

    def gemm_mx8(self, a8, sa, w8, sw, bias=None, residual=None, epilogue=EPI_BIAS, out_bf16=False, scale_rows_a=None,
                 scale_rows_w=None) -> torch.Tensor:
        """Block-scaled fp8 GEMM on v_mfma_scale_f32_32x32x64_f8f6f4; operands and scales as quantize_mx8 returns them.  The scale
        layouts' row counts default to the arrays' middle dimension; a smaller count (>= M / N) reads a prefix of the array."""
        m, k = a8.shape
        n = w8.shape[0]
        scale_rows_a = sa.shape[1] if scale_rows_a is None else int(scale_rows_a)
        scale_rows_w = sw.shape[1] if scale_rows_w is None else int(scale_rows_w)
        if sa.numel() < k // 128 * scale_rows_a * 4 or sw.numel() < k // 128 * scale_rows_w * 4:
            raise ValueError("a scale array is smaller than its scale_rows layout")
        bias = None if bias is None else self._f32(bias, (n,))
        if residual is not None and out_bf16:      # the bf16 residual-stream form (include/fern.h: fern_gemm_mx8)
            if residual.dtype != torch.bfloat16 or tuple(residual.shape) != (m, n):
                raise ValueError("out_bf16 with a residual takes a bf16 [M, N] residual stream")
            residual = residual.to(self.device).contiguous()
        else:
            residual = None if residual is None else self._f32(residual, (m, n))
        out = torch.empty(m, n, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=self.device)
        _lib.check(self.lib.fern_gemm_mx8(self._h, _ptr(a8), k, _ptr(sa), scale_rows_a, _ptr(w8), k, _ptr(sw), scale_rows_w, _ptr(bias),
                                          _ptr(residual), _ptr(out), n, m, n, k, int(epilogue), int(bool(out_bf16)), _stream()), "fern_gemm_mx8")
        return out

    def gemm_mx8_quant(self, a8, sa, w8, sw, bias=None, epilogue=EPI_BIAS):
        """gemm_mx8 with the output quantised in the epilogue: returns (e4m3fn bytes [M,N], block scales [N/128, M, 4])."""
        m, k = a8.shape
        n = w8.shape[0]
        bias = None if bias is None else self._f32(bias, (n,))
        out = torch.empty(m, n, dtype=torch.uint8, device=self.device)
        sc = torch.empty(n // 128, m, 4, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.fern_gemm_mx8_quant(self._h, _ptr(a8), k, _ptr(sa), sa.shape[1], _ptr(w8), k, _ptr(sw), sw.shape[1], _ptr(bias),
                                                _ptr(out), n, _ptr(sc), m, m, n, k, int(epilogue), _stream()), "fern_gemm_mx8_quant")
        return out, sc

    def layernorm(self, x, gamma, beta, eps: float, residual=None) -> torch.Tensor:
        x = self._f32(x)
        rows, d = x.shape
        residual = None if residual is None else self._f32(residual, (rows, d))
        gamma, beta = self._f32(gamma, (d,)), self._f32(beta, (d,))   # keep alive until the launch is queued
        out = torch.empty_like(x)
        _lib.check(self.lib.fern_layernorm(self._h, _ptr(x), _ptr(residual), _ptr(gamma), _ptr(beta), _ptr(out), rows, d,
                                           float(eps), _stream()), "fern_layernorm")
        return out

    def attention(self, q, k, v, heads: int, causal=False, scale=None) -> torch.Tensor:
        """q [B,Sq,W], k/v [B,Sk,W] -> [B,Sq,W] (W = heads * head_dim)."""
        q, k, v = self._f32(q), self._f32(k), self._f32(v)
        b, sq, w = q.shape
        sk = k.shape[1]
        hd = w // heads
        out = torch.empty_like(q)
        sc = float(scale) if scale is not None else hd ** -0.5
        _lib.check(self.lib.fern_attention(self._h, _ptr(q), w, _ptr(k), w, _ptr(v), w, _ptr(out), w, b, heads, hd, sq, sk,
                                           int(bool(causal)), sc, _stream()), "fern_attention")
        return out

    def pooled_attention(self, q, tokens, wk, wv, bv, heads: int) -> torch.Tensor:
        """One query per (image, head) over unprojected tokens (include/fern.h: fern_pooled_attention): q [B,E] (projected, bias
        included), tokens [B,S,E], wk / wv [E,E] in [out, in] layout, bv [E] -> [B,E]."""
        q, tokens = self._f32(q), self._f32(tokens)
        b, s, e = tokens.shape
        wk, wv, bv = self._f32(wk, (e, e)), self._f32(wv, (e, e)), self._f32(bv, (e,))
        out = torch.empty_like(q)
        _lib.check(self.lib.fern_pooled_attention(self._h, _ptr(q), e, _ptr(tokens), e, s * e, _ptr(wk), _ptr(wv), _ptr(bv), _ptr(out), e,
                                                  b, heads, e // heads, s, _stream()), "fern_pooled_attention")
        return out

    def _b16(self, x) -> torch.Tensor:
        """A [B,S,W] attention operand as a contiguous bf16 device tensor; anything but bf16 is rounded from fp32 first."""
        if x.dtype != torch.bfloat16:
            x3 = self._f32(x)
            return self.to_bf16(x3.reshape(-1, x3.shape[-1])).reshape(x3.shape)
        return x.to(self.device).contiguous()

    def attention_bf16(self, q, k, v, heads: int, causal=False, scale=None) -> torch.Tensor:
        """bf16 operand form of `attention`: q/k/v bf16 [B,S,W] (fp32 inputs are rounded first) -> bf16 [B,Sq,W]."""
        q, k, v = self._b16(q), self._b16(k), self._b16(v)
        b, sq, w = q.shape
        sk = k.shape[1]
        hd = w // heads
        out = torch.empty_like(q)
        sc = float(scale) if scale is not None else hd ** -0.5
        _lib.check(self.lib.fern_attention_bf16(self._h, _ptr(q), w, _ptr(k), w, _ptr(v), w, _ptr(out), w, b, heads, hd, sq, sk,
                                                int(bool(causal)), sc, _stream()), "fern_attention_bf16")
        return out

    def layernorm_q(self, x, gamma, beta, eps: float, out_form=QFORM_MX8, scale_rows=None, scales=None):
        """LayerNorm written in a GEMM operand form through the towers' own launchers (include/fern.h: fern_layernorm_q).  x: [R, d]
        fp32 (or bf16, MX form only) on the device; a view with a row stride (x.stride(0) % 4 == 0) is read in place.  Returns the bf16
        [R, d] tensor (QFORM_BF16), (e4m3fn bytes [R, d] as uint8, fp32 row scales [R]) (QFORM_FP8) or (e4m3fn bytes, E8M0 scales
        [d/128, scale_rows, 4]) (QFORM_MX8; `scales`: an existing array to write into, see quantize_mx8)."""
        if not (isinstance(x, torch.Tensor) and x.device == self.device and x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 2 and
                x.stride(1) == 1):
            x = self._f32(x)
        rows, d = x.shape
        gamma, beta = self._f32(gamma, (d,)), self._f32(beta, (d,))
        bf16_in = x.dtype == torch.bfloat16
        if out_form == QFORM_BF16:
            y, sc, srows = torch.empty(rows, d, dtype=torch.bfloat16, device=self.device), None, 0
        elif out_form == QFORM_FP8:
            y, sc, srows = torch.empty(rows, d, dtype=torch.uint8, device=self.device), self._empty(rows), 0
        elif out_form == QFORM_MX8:
            y = torch.empty(rows, d, dtype=torch.uint8, device=self.device)
            sc = self._mx_scales(d, rows, scale_rows, scales)
            srows = sc.shape[1]
        else:
            raise ValueError(f"unknown operand form {out_form}")
        _lib.check(self.lib.fern_layernorm_q(self._h, _ptr(x), int(bf16_in), x.stride(0), _ptr(gamma), _ptr(beta), int(out_form), _ptr(y), d,
                                             _ptr(sc), srows, rows, d, float(eps), _stream()), "fern_layernorm_q")
        return y if out_form == QFORM_BF16 else (y, sc)

    def attention_mx8(self, q, k, v, heads: int, causal=False, scale=None, out=None, scale_rows=None, scales=None):
        """attention_bf16 with the block-scaled output of FERN_PREC_MX8 / _MX8_IMG (include/fern.h: fern_attention_mx8): q/k/v bf16
        [B,S,W] (fp32 inputs are rounded first) -> (e4m3fn bytes [B*Sq, ldo] as uint8, E8M0 scales [W/128, scale_rows, 4]).  `out`: an
        existing uint8 [B*Sq, ldo] array to write into (columns >= W are not written), `scales` as in quantize_mx8."""
        q, k, v = self._b16(q), self._b16(k), self._b16(v)
        b, sq, w = q.shape
        sk = k.shape[1]
        hd = w // heads
        if out is None:
            out = torch.empty(b * sq, w, dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or out.device != self.device or out.dim() != 2 or out.shape[0] != b * sq or out.shape[1] < w or out.stride(1) != 1:
            raise ValueError(f"out must be a uint8 [{b * sq}, ldo >= {w}] tensor on {self.device}")
        sc = self._mx_scales(w, b * sq, scale_rows, scales)
        scl = float(scale) if scale is not None else hd ** -0.5
        _lib.check(self.lib.fern_attention_mx8(self._h, _ptr(q), w, _ptr(k), w, _ptr(v), w, _ptr(out), out.stride(0), _ptr(sc), sc.shape[1],
                                               b, heads, hd, sq, sk, int(bool(causal)), scl, _stream()), "fern_attention_mx8")
        return out, sc

    def im2col_q(self, images, patch: int, out_form=QFORM_MX8, scale_rows=None, scales=None):
        """Patch rows of [b, 3, img, img] fp32 images in the patch embedding's operand form (include/fern.h: fern_im2col_q): the bf16
        [b * (img/patch)^2, 3 * patch^2] tensor (QFORM_BF16) or (e4m3fn bytes as uint8, E8M0 scales [d/128, scale_rows, 4]) (QFORM_MX8)."""
        x = self._f32(images)
        b, _, img, _ = x.shape
        rows, d = b * (img // patch) ** 2, 3 * patch * patch
        if out_form == QFORM_BF16:
            y, sc, srows = torch.empty(rows, d, dtype=torch.bfloat16, device=self.device), None, 0
        elif out_form == QFORM_MX8:
            y = torch.empty(rows, d, dtype=torch.uint8, device=self.device)
            sc = self._mx_scales(d, rows, scale_rows, scales)
            srows = sc.shape[1]
        else:
            raise ValueError(f"unknown operand form {out_form}")
        _lib.check(self.lib.fern_im2col_q(self._h, _ptr(x), b, img, patch, int(out_form), _ptr(y), _ptr(sc), srows, _stream()), "fern_im2col_q")
        return y if out_form == QFORM_BF16 else (y, sc)

    # ---- the ModifiedResNet's kernels through the tower's launchers (include/fern.h: fern_conv3x3_nhwc ...) ----
    def conv3x3_nhwc(self, x, w, bias) -> torch.Tensor:
        """relu(conv3x3(x, stride 1, zero padding 1) + bias): x [b,H,W,cin] NHWC, w [cout, 9*cin] in (ky, kx, c) order -> [b,H,W,cout]."""
        x = self._f32(x)
        b, h, wd, cin = x.shape
        w = self._f32(w)
        cout = w.shape[0]
        w, bias = self._f32(w, (cout, 9 * cin)), self._f32(bias, (cout,))
        out = self._empty(b, h, wd, cout)
        _lib.check(self.lib.fern_conv3x3_nhwc(self._h, _ptr(x), _ptr(w), _ptr(bias), _ptr(out), b, h, wd, cin, cout, _stream()),
                   "fern_conv3x3_nhwc")
        return out

    def conv1x1_nhwc(self, x, w, bias, residual=None, relu=True) -> torch.Tensor:
        """x [M,cin] w [cout,cin]^T + bias over pixel rows; relu(.) when `relu`, relu(. + residual [M,cout]) with a residual."""
        x, w = self._f32(x), self._f32(w)
        m, cin = x.shape
        cout = w.shape[0]
        w, bias = self._f32(w, (cout, cin)), self._f32(bias, (cout,))
        residual = None if residual is None else self._f32(residual, (m, cout))
        out = self._empty(m, cout)
        _lib.check(self.lib.fern_conv1x1_nhwc(self._h, _ptr(x), _ptr(w), _ptr(bias), _ptr(residual), _ptr(out), m, cin, cout, int(bool(relu)),
                                              _stream()), "fern_conv1x1_nhwc")
        return out

    def stem_conv(self, images, w, bias) -> torch.Tensor:
        """relu(conv3x3(images, stride 2, zero padding 1) + bias): images [b,3,S,S] NCHW, w [cout_pad, 27] in (c, ky, kx) order ->
        [b,S/2,S/2,cout_pad] NHWC."""
        x = self._f32(images)
        b, _, s, _ = x.shape
        w = self._f32(w)
        cp = w.shape[0]
        w, bias = self._f32(w, (cp, 27)), self._f32(bias, (cp,))
        out = self._empty(b, s // 2, s // 2, cp)
        _lib.check(self.lib.fern_stem_conv(self._h, _ptr(x), _ptr(w), _ptr(bias), _ptr(out), b, s, cp, _stream()), "fern_stem_conv")
        return out

    def avgpool_nhwc(self, x, k: int) -> torch.Tensor:
        """Mean over k x k windows (stride k) of x [b,H,W,C] NHWC -> [b,H/k,W/k,C]."""
        x = self._f32(x)
        b, h, wd, ch = x.shape
        out = self._empty(b, h // k, wd // k, ch)
        _lib.check(self.lib.fern_avgpool_nhwc(self._h, _ptr(x), _ptr(out), b, h, wd, ch, int(k), _stream()), "fern_avgpool_nhwc")
        return out

    def attnpool_tokens(self, x, pos):
        """The attention pool's token rows: x [b,HW,C], pos [HW+1,C] -> (T [b,HW+1,C] = [mean(x) + pos[0]; x + pos[1:]], T0 [b,C] = T[:,0])."""
        x = self._f32(x)
        b, hw, ch = x.shape
        pos = self._f32(pos, (hw + 1, ch))
        t, t0 = self._empty(b, hw + 1, ch), self._empty(b, ch)
        _lib.check(self.lib.fern_attnpool_tokens(self._h, _ptr(x), _ptr(pos), _ptr(t), _ptr(t0), b, hw, ch, _stream()), "fern_attnpool_tokens")
        return t, t0

    # ---- profiling ----------------------------------------------------------------------------
    def prof_enable(self, on: bool) -> None:
        _lib.check(self.lib.fern_prof_enable(self._h, int(on)), "fern_prof_enable")

    def prof_collect(self) -> Dict[str, float]:
        st = _lib.ProfStats()
        _lib.check(self.lib.fern_prof_collect(self._h, C.byref(st)), "fern_prof_collect")
        return {f: getattr(st, f) for f, _ in st._fields_}

    def tuner_export(self) -> str:
        """The GEMM tuner's per-shape tile choices so far (text; a file of it named by FERN_GEMM_TILES pins them)."""
        n = self.lib.fern_tuner_export(None, 0)
        buf = C.create_string_buffer(int(n) + 1)
        self.lib.fern_tuner_export(buf, int(n) + 1)
        return buf.value.decode()

    def ws_generation(self) -> int:
        """Changes whenever this context has freed workspace memory an earlier call used (include/fern.h: fern_ws_generation):
        a hipGraph captured from this engine's calls is stale once the value moves."""
        return int(self.lib.fern_ws_generation(self._h))

    def tuner_import(self, text: str) -> None:
        """Adopt another process's `tuner_export()` for the shapes it lists (all tile choices are bit-identical: speed only)."""
        _lib.check(self.lib.fern_tuner_import(text.encode()), "fern_tuner_import")

    def tuner_set_concurrency(self, lanes: int) -> None:
        """Tell the GEMM tuner how many batches are kept in flight on separate streams (include/fern.h:
        fern_tuner_set_concurrency): shapes tuned afterwards are scored for pipeline throughput, not stand-alone latency."""
        _lib.check(self.lib.fern_tuner_set_concurrency(int(lanes)), "fern_tuner_set_concurrency")

    def tuner_force_config(self, family: str, cfg: int) -> None:
        """Force one tile configuration of a GEMM family ("f32", "f32x3", "bf16", "fp8", "mx8") process-wide; cfg < 0 releases it
        (include/fern.h: fern_tuner_force_config).  Results never depend on it."""
        _lib.check(self.lib.fern_tuner_force_config(family.encode(), int(cfg)), "fern_tuner_force_config")

    def sync(self) -> None:
        _lib.check(self.lib.fern_sync(self._h, _stream()), "fern_sync")

"""CLIP encoder object and the ImageCLIP / TextCLIP wrappers, behind the reference's call surface.

Reference interface: the external ``clip_model`` object the reference builds with
``open_clip.create_model_and_transforms`` (/root/reference/run/test/test_fiq.py:141-146) and calls as
``clip_model.encode_image(images)`` (/root/reference/utils/utils.py:64) and
``clip_model.encode_text(text, mode=, visual_emb=)`` (/root/reference/run/test/test_fiq.py:102-103), plus the
two thin wrappers of /root/reference/models/clip_model.py:5-31.

``encode_text`` semantics are *defined* here because the reference's private text encoder is unreleased
(SURVEY.md 8c): one text-tower pass; ``seq = ln_final(h) @ text_projection``; ``global = seq[EOT]``;
default/"global" returns ``(global, seq)``; "seq" returns ``seq``; ``visual_emb`` [13,B,D] is shape-checked
and ignored ("vanilla CLIP single branch", README.md:41).
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Union

import numpy as np
import torch

from . import synth
from .engine import PATCH_NUM, FernEngine
from .synth import CLIP_CONFIGS, ClipConfig


class FernCLIP:
    """CLIP ViT image tower + text tower running as HIP kernels on one MI355X."""

    def __init__(self, model_name: Union[str, ClipConfig] = "ViT-B-16", device="cuda:0", engine=None, precision: str = "fp32",
                 force_quick_gelu: bool = False):
        """``force_quick_gelu`` mirrors open_clip's argument of the same name: both towers' MLPs use QuickGELU, x * sigmoid(1.702 x),
        instead of exact-erf GELU.  open_clip sets it for ``pretrained="openai"``; pass it (or a ``*-quickgelu`` config name) whenever
        the weights that follow through ``load_state_dict`` are OpenAI's -- RN50x4's only public weights are."""
        if not isinstance(model_name, ClipConfig) and model_name not in CLIP_CONFIGS:
            raise ValueError(f"unknown CLIP model {model_name!r}; known: {sorted(CLIP_CONFIGS)}")
        self.cfg = synth.resolve_clip_config(model_name, force_quick_gelu)
        self.engine = engine if engine is not None else FernEngine(device)
        self.device = self.engine.device
        self._state: Dict[str, np.ndarray] = {}
        self._ready = False
        self._text_cache = None
        if precision != "fp32":
            self.set_precision(precision)

    def set_precision(self, precision: str):
        """"fp32": parity mode (default, the reference's arithmetic).  "bf16": perf mode of the transformer towers --
        bf16 operands / fp32 accumulation on the block GEMMs and attention; "fp8": e4m3fn operands on those GEMMs
        with per-token / per-channel scales; "mx8": e4m3fn operands with one power-of-two scale per 32-element block on the
        block-scaled MFMA (BASELINE config 5); "f32x3": fp32 data, the large plain GEMMs computed from three bf16 planes per operand
        (fp32-accurate, not the bit-exact chain; every tower incl. RN50x4's 1x1 convolutions) -- include/fern.h:fern_precision; no reference counterpart (the reference evaluates in fp32, test_fiq.py:141-149)."""
        if precision not in ("fp32", "f32x3") and self.cfg.v_arch == "resnet":
            raise ValueError("reduced precisions cover the transformer towers; RN50x4's image tower has no bf16 / fp8 path")
        self.engine.set_precision(precision)
        self._text_cache = None
        return self

    # -- nn.Module-like surface used by the reference scripts (test_fiq.py:142-145) ---------------
    def load_state_dict(self, state_dict: Mapping[str, object], strict: bool = True):
        sd = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in state_dict.items()}
        self.engine.load_tensors(sd)
        self.engine.finalize_clip(self.cfg)      # raises FernError naming the first missing/mis-shaped key
        self._state = sd
        self._ready = True
        self._text_cache = None
        return self

    def init_random(self, seed: int = 0):
        return self.load_state_dict(synth.clip_state_dict(self.cfg, seed))

    def state_dict(self):
        return {k: torch.from_numpy(np.array(v)) for k, v in self._state.items()}

    def eval(self):
        return self

    def float(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def parameters(self):
        return iter(())

    # -- encoders --------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_image(self, images: torch.Tensor) -> torch.Tensor:
        """[b,3,S,S] f32 -> [b,embed_dim] un-normalised (utils/utils.py:64)."""
        return self.engine.encode_image(images)

    @torch.no_grad()
    def encode_text(self, text: torch.Tensor, mode: str = "global", visual_emb: Optional[torch.Tensor] = None):
        if visual_emb is not None:
            ve = tuple(visual_emb.shape)
            if len(ve) != 3 or ve[0] != PATCH_NUM or ve[1] != text.shape[0] or ve[2] != self.cfg.embed_dim:
                raise ValueError(f"visual_emb must be [{PATCH_NUM}, B, {self.cfg.embed_dim}], got {ve}")
        if not text.is_cuda and text.numel() and (int(text.min()) < 0 or int(text.max()) >= self.cfg.vocab_size):
            raise IndexError(f"token id out of range [0, {self.cfg.vocab_size})")      # nn.Embedding's error in the reference
        # the reference calls encode_text twice on the same tokens (global, then seq: test_fiq.py:102-103); one tower pass
        # serves both.  "The same tokens" is decided WITHOUT a device sync: host tokens (what the reference's tokenizer yields)
        # are compared on the host; device tokens ONLY by object identity + torch's in-place version counter, with the cache
        # holding a strong reference to the tensor (a freed block handed out again at the same address with version 0 and the
        # same shape must not hit: ADVICE r3).  `visual_emb` is part of the key as well
        # (by identity AND in-place version -- a preallocated buffer refilled with `copy_` is a different argument: ADVICE r4).
        # The entry is dropped once the "seq" call has been served: the pair of calls it exists for is over, and the cache must not
        # keep the caller's device tensors (tokens, visual_emb, a [B,77,D] output) alive until some later miss.
        c = self._text_cache
        hit = False
        ve_version = None if visual_emb is None else visual_emb._version
        if c is not None and c["visual_emb"] is visual_emb and c["ve_version"] == ve_version:
            if text.is_cuda:
                hit = c["tensor"] is text and c["version"] == text._version
            else:
                h = c["host"]
                hit = h is not None and h.shape == text.shape and h.dtype == text.dtype and torch.equal(h, text)
        if hit:
            g, s = c["global"], c["seq"]
            if mode == "seq":
                self._text_cache = None
        else:
            t = text.to(device=self.device, dtype=torch.int64)
            g, s = self.engine.encode_text(t, visual_emb=visual_emb)
            self._text_cache = None if mode == "seq" else {
                "tensor": text if text.is_cuda else None, "version": text._version, "host": None if text.is_cuda else text.clone(),
                "visual_emb": visual_emb, "ve_version": ve_version, "global": g, "seq": s}
        return s if mode == "seq" else (g, s)


def create_model(model_name="ViT-B-16", device="cuda:0", seed: Optional[int] = None, engine=None, precision: str = "fp32",
                 force_quick_gelu: bool = False) -> FernCLIP:
    """Counterpart of ``open_clip.create_model_and_transforms(name, device=)`` (test_fiq.py:141): random-init when
    ``seed`` is given, otherwise weights must follow through ``load_state_dict(saved["CLIP"])``.  ``force_quick_gelu`` is
    open_clip's argument: what ``pretrained="openai"`` turns on there (QuickGELU in both towers) is requested here with
    ``force_quick_gelu=True`` or a ``*-quickgelu`` model name."""
    m = FernCLIP(model_name, device, engine=engine, precision=precision, force_quick_gelu=force_quick_gelu)
    if seed is not None:
        m.init_random(seed)
    return m


class ImageCLIP:
    """models/clip_model.py:5-15."""

    def __init__(self, clip_model):
        self.clip_model = clip_model

    def __call__(self, images, mode="eval"):
        self.clip_model.eval()
        with torch.no_grad():
            return self.clip_model.encode_image(images)

    forward = __call__


class TextCLIP:
    """models/clip_model.py:18-31."""

    def __init__(self, clip_model):
        self.clip_model = clip_model

    def __call__(self, text, mode="global", visual_emb=None):
        self.clip_model.eval()
        with torch.no_grad():
            if mode == "seq":
                return self.clip_model.encode_text(text, mode="seq", visual_emb=visual_emb)
            return self.clip_model.encode_text(text, visual_emb=visual_emb)

    forward = __call__

"""The CPU oracle of the QuickGELU CLIP towers, without a second copy of oracle/clip.py.  TEST INFRASTRUCTURE.

``oracle.clip`` states every tower -- fp32 and each reduced-precision restatement -- with ``F.gelu`` in the MLP.  ``quick_gelu()``
below is a context manager that replaces the name ``F`` INSIDE ``oracle.clip`` by a proxy: every attribute is forwarded to
``torch.nn.functional`` except ``gelu``, which becomes ``x * sigmoid(1.702 x)`` (open_clip's QuickGELU, HF's ``quick_gelu``).
``F`` is restored in ``finally``; ``oracle.fusion`` (the fusion BERT keeps exact-erf GELU) is never touched.

The patched oracle is pinned by tests/golden/clip_quickgelu*.npz (tools/make_goldens.py:clip_quickgelu_goldens: the in-tree
statement of CLIP run with hidden_act="quick_gelu"), see tests/test_quickgelu_cpu.py.
"""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch
import torch.nn.functional as _F

from oracle import clip as oclip

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def quick_gelu_fn(x, approximate="none"):
    """x * sigmoid(1.702 x); ``approximate`` is accepted (and ignored) so that every ``F.gelu`` call form goes through."""
    return x * torch.sigmoid(1.702 * x)


class _QuickGeluFunctional:
    """torch.nn.functional with ``gelu`` replaced."""

    gelu = staticmethod(quick_gelu_fn)

    def __getattr__(self, name):
        return getattr(_F, name)


@contextlib.contextmanager
def quick_gelu():
    saved = oclip.F
    oclip.F = _QuickGeluFunctional()
    try:
        yield oclip
    finally:
        oclip.F = saved


def load_goldens() -> dict:
    """The QuickGELU fixture: clip.npz's keys.  (Two files on disk: fp32 outputs do not compress and one file would pass 1 MiB.)"""
    out = {}
    for name in ("clip_quickgelu.npz", "clip_quickgelu_vitb16.npz"):
        with np.load(os.path.join(GOLD, name)) as z:
            out.update({k: z[k] for k in z.files})
    return out

"""What the GPU test files share and none of them owns: seeded inputs, bit and fp64 comparers, the near-tie rule, engine builders, the
gallery forms, the place table and device pointers.  One statement of each, so that a new test sees the data and is held to the check its
family has always had.  The GEMM families' operands, references and bounds (and the MX byte rules) are tests/gemm_refs.py; the oracles
inside the ranking test files are independent statements and stay there.

A plain module on tests/'s import path.  It imports without a GPU and without the library: the engine helpers import `FernEngine` when
called.  tests/test_support_cpu.py pins the inputs' digests and the comparers' behaviour."""
import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def rand(*shape, seed=0, scale=1.0):
    """fp32 normal values of `shape` from a generator of its own seeded with `seed` (a keyword: a third positional is a dimension)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def int_unit(n, d, seed):
    """[n, d] rows with entries in {-1, 0, 1} / 8: every dot product is exact in fp32 in any summation order, and ties abound."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, (n, d), generator=g).float() / 8.0


def unit(n, d, seed):
    """[n, d] unit-length rows of rand(n, d, seed=seed)."""
    return F.normalize(rand(n, d, seed=seed), dim=-1)


def t(a):
    """A numpy array as a tensor (a contiguous copy if the array is not contiguous)."""
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- bit-equality comparers ----------------------------------------------------------------------------------------------------------
_INT = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


def bits(x):
    """The bytes of a tensor or array as a host integer array of the same shape: bf16 as int16, 4-byte types as int32 (NaN == NaN,
    -0.0 != 0.0)."""
    if torch.is_tensor(x):
        x = x.detach().cpu().contiguous()
        return x.view(getattr(torch, _INT[x.element_size()])).numpy()
    x = np.asarray(x)
    return (x if x.flags.c_contiguous else x.copy()).view(_INT[x.itemsize])


def _dtype(x):
    return str(x.dtype).replace("torch.", "") if torch.is_tensor(x) else np.asarray(x).dtype.name


def _difference(got, want, what):
    """None, or the sentence that says where `got` and `want` part."""
    several = [isinstance(x, (tuple, list)) for x in (got, want)]
    if any(several):
        if not all(several) or len(got) != len(want):
            return f"{what}: {len(got) if several[0] else 'one array'} against {len(want) if several[1] else 'one array'}"
        for j, (g, w) in enumerate(zip(got, want)):
            d = _difference(g, w, f"{what}[{j}]")
            if d:
                return d
        return None
    if tuple(got.shape) != tuple(want.shape) or _dtype(got) != _dtype(want):
        return f"{what}: {tuple(got.shape)} {_dtype(got)} vs {tuple(want.shape)} {_dtype(want)}"
    a, b = bits(got), bits(want)
    if np.array_equal(a, b):
        return None
    bad = np.argwhere(a != b)
    at = tuple(bad[0].tolist())
    host = lambda x: x.detach().cpu() if torch.is_tensor(x) else np.asarray(x)      # noqa: E731
    return f"{what}: {len(bad)} element(s) differ, the first at {at}: got {host(got)[at].item()!r}, want {host(want)[at].item()!r}"


def assert_same_bits(got, want, what=""):
    """Tensors or numpy arrays, singly or as tuples of them: the same shape, the same dtype and the same bits.  A failure names the
    number of differing elements and the first differing position."""
    d = _difference(got, want, what or "bits")
    if d:
        raise AssertionError(d)


def same_bits(got, want):
    """assert_same_bits as a boolean, for `assert same_bits(...) and ...` and for counting mismatches."""
    return _difference(got, want, "bits") is None


# ---- fp64 comparers ------------------------------------------------------------------------------------------------------------------
def maxerr(got, ref):
    """max |got - ref| in fp64."""
    return (got.detach().cpu().double() - ref.double()).abs().max().item()


def cos_err(a, b):
    """max over rows of |1 - cos(a, b)| in fp64 ([B, D], or [B, ...] flattened per row)."""
    a, b = a.cpu().double(), b.double()
    return (1 - F.cosine_similarity(a.flatten(-1 if a.dim() == 2 else 1), b.flatten(-1 if b.dim() == 2 else 1), dim=-1)).abs().max().item()


def close(got, ref, rel=2e-5):
    """The fp32 kernels' bound: max abs error <= rel x the largest reference magnitude.  Prints the figures before it asserts."""
    got, ref = got.detach().cpu().double(), ref.double()
    err = (got - ref).abs().max().item()
    print(f"max abs err {err:.3e} vs scale {ref.abs().max().item():.3e} (bound {rel * max(ref.abs().max().item(), 1e-6):.3e})")
    assert err <= rel * max(ref.abs().max().item(), 1e-6), f"max abs err {err} vs scale {ref.abs().max().item()}"


# ---- near-ties -----------------------------------------------------------------------------------------------------------------------
def assert_same_order_up_to_near_ties(full_scores, idx, ref_idx, gap):
    """Two rankings `idx` / `ref_idx` [B, K] may name different rows at a place only where the reference's own scores of the two rows,
    full_scores[r][row] (a [B, N] matrix, or a mapping of the differing queries to their score rows), are closer than `gap`.  The gap has
    no default: it is the fp32 rounding of the scores compared, and each site states the number it has always used."""
    host = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)      # noqa: E731
    idx, ref_idx = host(idx), host(ref_idx)
    assert idx.shape == ref_idx.shape, (idx.shape, ref_idx.shape)
    for r, p in zip(*np.nonzero(idx != ref_idx)):
        a, b = int(idx[r, p]), int(ref_idx[r, p])
        d = abs(float(full_scores[r][a]) - float(full_scores[r][b]))
        assert d < gap, f"query {r} rank {p}: rows {a} / {b} differ by {d:.3e} in score (gap {gap:g})"


# ---- engines -------------------------------------------------------------------------------------------------------------------------
def fresh_engine():
    """The generator behind a file's module-scoped engine fixture: an engine of the file's own (it sets strategies and precisions on it),
    closed when the fixture goes."""
    from fashionern_aaai2024_amd.engine import FernEngine
    e = FernEngine("cuda:0")
    yield e
    e.close()


def tower_engine(name_or_cfg, seed, edit=None, quick=None):
    """(cfg, numpy state dict, engine) of a CLIP config with synthetic weights of `seed`.  `edit(cfg, sd)` changes the weights before
    they are loaded; `quick` True forces QuickGELU on, False / None leave the config's own activation."""
    from fashionern_aaai2024_amd import synth
    from fashionern_aaai2024_amd.engine import FernEngine
    cfg = synth.resolve_clip_config(name_or_cfg, force_quick_gelu=bool(quick))
    sd = synth.clip_state_dict(cfg, seed=seed)
    if edit:
        edit(cfg, sd)
    eng = FernEngine("cuda:0")
    eng.load_tensors(sd)
    eng.finalize_clip(cfg)
    return cfg, sd, eng


@functools.lru_cache(maxsize=None)
def fusion_engine(d, seed):
    """(engine, torch state dict) with the synthetic fusion weights of width `d`; one per (d, seed), kept for the session."""
    from fashionern_aaai2024_amd import synth
    from fashionern_aaai2024_amd.engine import FernEngine
    from oracle import fusion as ofusion
    eng = FernEngine("cuda:0")
    sd = synth.fusion_state_dict(d, seed=seed)
    eng.load_tensors(sd)
    eng.finalize_fusion(d)
    return eng, ofusion.as_torch(sd)


# ---- gallery forms -------------------------------------------------------------------------------------------------------------------
def gallery(eng, g, form):
    """The fp32 rows `g` as the gallery argument of `form`: "fp32" (the device tensor), "prepared" (PreparedGallery) or "bf16"."""
    g = g.cuda()
    return g if form == "fp32" else eng.prepare_gallery(g) if form == "prepared" else eng.prepare_gallery(g).bf16


def strategy_forms(eng, g):
    """[(label, gallery argument, rank strategy to set or None)]: the fp32 tensor, the prepared gallery under each strategy, the bf16 rows."""
    pg = eng.prepare_gallery(g)
    return [("fp32", g.cuda(), None), ("prepared-auto", pg, "auto"), ("prepared-plain", pg, "plain"), ("prepared-lists", pg, "lists"),
            ("prepared-dense", pg, "dense"), ("bf16", pg.bf16, None)]


# ---- ranking arithmetic --------------------------------------------------------------------------------------------------------------
def places(scores):
    """[B,N] int64: the place of every row in the stable ranking of `scores` (numpy [B,N]): score descending, index ascending."""
    order = np.argsort(-scores, axis=1, kind="stable")
    place = np.empty_like(order)
    np.put_along_axis(place, order, np.broadcast_to(np.arange(scores.shape[1]), order.shape), axis=1)
    return place


# ---- pointers ------------------------------------------------------------------------------------------------------------------------
def ptr(x, byte_offset=0):
    """Device pointer of a Framed view / tensor as a c_void_p (None stays NULL)."""
    return None if x is None else C.c_void_p(x.data_ptr() + byte_offset)

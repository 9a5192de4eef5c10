"""CPU: the shared test support (tests/support.py, the MX byte rules of tests/gemm_refs.py, tests/_dump.py) does what the GPU files
rely on.  The digests were computed with the per-file helpers this module replaced: an edit that moves them moves every test's data."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_refs
import support as S

TESTS = os.path.dirname(os.path.abspath(__file__))


def _digest(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def test_inputs_reproduce_their_digests():
    assert _digest(S.rand(3, 5, seed=7, scale=0.5)) == "a03661ea82e138c44911d6693eea519416490781db148119b7791722cc0f22a1"
    assert _digest(S.rand(4, 6)) == "46e82db66fbd8858a214e26cf7f8be3ab5639ef7cedd23f405c7c149f05b1539"
    assert _digest(S.rand(4, 6, seed=3, scale=0.25)) == "546b72ad9684737db1aff5fe9f8b459c6460d80abf079e602bbbc71f5e931998"
    assert _digest(S.int_unit(5, 8, 3)) == "8fe773362bc089d3ac2cb6efa5aa0fb4ecd1dac0d0ce8f3213a3b0eade068333"
    assert _digest(S.unit(4, 16, 11)) == "9417fb08fc065f0b1f6dfcd256d8cebb79611d1e5945e3096369add9ce70ae59"
    assert gemm_refs.rand is S.rand and gemm_refs.close is S.close
    assert S.rand(4, 6).dtype == torch.float32 and set((S.int_unit(50, 8, 1) * 8).flatten().tolist()) == {-1.0, 0.0, 1.0}
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    assert S.t(a.T).is_contiguous() and torch.equal(S.t(a.T), torch.from_numpy(a).T)


# ---- bit-equality comparers ----------------------------------------------------------------------------------------------------------
def test_same_bits_tells_signed_zeros_and_nan_payloads_apart():
    pz, nz = torch.tensor([[0.0, 1.0]]), torch.tensor([[-0.0, 1.0]])
    assert pz.equal(nz) and not S.same_bits(pz, nz) and S.same_bits(nz, nz.clone())
    nan_a = np.array([0x7FC00000, 0x3F800000], dtype=np.uint32).view(np.float32)
    nan_b = np.array([0x7FC00001, 0x3F800000], dtype=np.uint32).view(np.float32)
    assert S.same_bits(nan_a, nan_a.copy()) and not S.same_bits(nan_a, nan_b)          # NaN == NaN here, payload for payload
    assert S.same_bits(torch.from_numpy(nan_a), nan_a)                                    # a tensor against an array
    h = torch.tensor([1.0, -0.0]).bfloat16()
    assert S.bits(h).dtype == np.int16 and S.bits(pz).dtype == np.int32 and S.same_bits(h, h.clone()) and not S.same_bits(h, -h)


def test_same_bits_refuses_another_dtype_or_shape():
    i = np.arange(6, dtype=np.int32).reshape(2, 3)
    assert not S.same_bits(i, i.view(np.float32))                                         # the same bytes under another dtype
    assert not S.same_bits(i, i.reshape(3, 2)) and not S.same_bits(i, i.astype(np.int64))
    assert not S.same_bits((i, i), (i,)) and not S.same_bits((i, i), i)
    with pytest.raises(AssertionError, match=r"case 7: \(2, 3\) int32 vs \(3, 2\) int32"):
        S.assert_same_bits(torch.from_numpy(i), i.reshape(3, 2), "case 7")
    with pytest.raises(AssertionError, match="int32 vs .*float32"):
        S.assert_same_bits(i, i.view(np.float32))


def test_assert_same_bits_names_the_first_differing_position():
    want = np.zeros((3, 4), dtype=np.float32)
    got = want.copy()
    got[1, 2], got[2, 0] = 5.0, -0.0
    with pytest.raises(AssertionError, match=r"scores: 2 element\(s\) differ, the first at \(1, 2\): got 5.0, want 0.0"):
        S.assert_same_bits(torch.from_numpy(got), want, "scores")
    idx = np.arange(12, dtype=np.int32).reshape(3, 4)
    S.assert_same_bits((torch.from_numpy(want), idx), (want, torch.from_numpy(idx)))
    with pytest.raises(AssertionError, match=r"pair\[1\]: 1 element\(s\) differ, the first at \(0, 3\)"):
        S.assert_same_bits((want, idx), (want, np.where(idx == 3, -1, idx).astype(np.int32)), "pair")


# ---- fp64 comparers ------------------------------------------------------------------------------------------------------------------
def test_fp64_comparers(capsys):
    ref = torch.tensor([[3.0, 4.0], [1.0, 0.0]], dtype=torch.float64)
    got = ref.float() + torch.tensor([[0.0, 1e-3], [0.0, 0.0]])
    assert abs(S.maxerr(got, ref) - 1e-3) < 1e-6
    assert S.cos_err(ref.float(), ref) < 1e-15 and abs(S.cos_err(torch.tensor([[1.0, 0.0]]), torch.tensor([[0.0, 1.0]])) - 1.0) < 1e-15
    S.close(got, ref, rel=3e-4)
    assert "max abs err" in capsys.readouterr().out
    with pytest.raises(AssertionError):
        S.close(got, ref)                                   # the default is gemm_refs' 2e-5 of the largest magnitude: 8e-5 here


# ---- near-ties -----------------------------------------------------------------------------------------------------------------------
def test_near_tie_rule():
    full = torch.tensor([[1.0, 0.5, 0.5 + 5e-7, 0.2, 0.6]], dtype=torch.float64)
    ref = torch.tensor([[0, 4, 2, 1, 3]])
    same, swapped = ref.clone().int(), torch.tensor([[0, 4, 1, 2, 3]], dtype=torch.int32)
    S.assert_same_order_up_to_near_ties(full, same, ref, gap=2e-6)
    S.assert_same_order_up_to_near_ties(full, swapped, ref, gap=2e-6)                     # rows 1 and 2 are 5e-7 apart
    S.assert_same_order_up_to_near_ties({0: full[0].numpy()}, swapped.numpy(), ref.numpy(), gap=2e-6)      # score rows of the differing queries
    with pytest.raises(AssertionError, match="query 0 rank 2: rows 1 / 2"):
        S.assert_same_order_up_to_near_ties(full, swapped, ref, gap=1e-7)                 # the same swap outside the gap
    with pytest.raises(AssertionError, match="rows 2 / 4"):
        S.assert_same_order_up_to_near_ties(full, torch.tensor([[0, 2, 4, 1, 3]]), ref, gap=2e-6)      # a swap of rows 0.1 apart
    with pytest.raises(AssertionError, match="rows 3 / 4"):
        S.assert_same_order_up_to_near_ties(full, torch.tensor([[0, 3, 2, 1, 3]]), ref, gap=2e-6)      # not a swap at all: a far row named twice
    with pytest.raises(TypeError):
        S.assert_same_order_up_to_near_ties(full, same, ref)                              # the gap is stated at every site


# ---- MX byte rules -------------------------------------------------------------------------------------------------------------------
def _f32(u):
    return torch.tensor(u, dtype=torch.int64).to(torch.int32).view(torch.float32)


def test_e8m0_byte_on_hand_values():
    """byte = biased exponent - 8, one more past the 0x600000 mantissa (1.75 x 2^e = 448 x 2^(e-8)): the block maximum lands in (224, 448]
    of its scale 2^(byte - 127)."""
    e8 = gemm_refs.e8m0_byte
    assert e8(torch.tensor([1.0, 2.0, 0.5, 256.0, 2.0 ** -100, 2.0 ** 100])).tolist() == [119, 120, 118, 127, 19, 219]
    assert e8(torch.tensor([448.0, 1.75, 3.5])).tolist() == [127, 119, 120]                # mantissa 0x600000 itself stays
    assert e8(_f32([0x43E00000, 0x43E00001, 0x3FE00001, 0x43DFFFFF])).tolist() == [127, 128, 120, 127]      # 448, the next float, 1.75's next, 448's previous
    assert e8(torch.tensor([0.0, 2.0 ** -126, 2.0 ** -118, 2.0 ** -117])).tolist() == [1, 1, 1, 2]      # the lower clamp end
    # the upper clamp end 253 is beyond fp32 maxima: the largest finite value and inf give 247, and nothing exceeds 253
    top = e8(torch.tensor([torch.finfo(torch.float32).max, float("inf")]))
    assert top.tolist() == [247, 247] and int(top.max()) <= 253
    m = S.rand(1000, seed=1).abs() * torch.logspace(-30, 30, 1000)
    scaled = m.double() / torch.ldexp(torch.ones((), dtype=torch.float64), e8(m) - 127)
    assert (scaled > 224).all() and (scaled <= 448).all()


def test_e4m3_code_on_hand_values():
    code = gemm_refs.e4m3_code
    b, o = code(torch.tensor([0.0, -0.0, 1.0, 2.0, 0.5, 1.125, 448.0, -448.0, 2.0 ** -9, -1.0]))
    assert b.tolist() == [0x00, 0x80, 0x38, 0x40, 0x30, 0x39, 0x7E, 0xFE, 0x01, 0xB8]
    assert o.tolist() == [0, 0, 56, 64, 48, 57, 126, -126, 1, -56]                          # the signed position on the code line
    b, _ = code(torch.tensor([1.0625, 1.1875, -1.0625]))                                    # midpoints: to the even mantissa
    assert b.tolist() == [0x38, 0x3A, 0xB8]
    line = code(torch.linspace(-448, 448, 2001))[1]
    assert (line[1:] >= line[:-1]).all()                                                    # the code line is monotone in the value


# ---- ranking arithmetic --------------------------------------------------------------------------------------------------------------
def test_places_on_a_tie():
    scores = np.array([[0.5, 0.9, 0.5, 0.1], [1.0, 1.0, 1.0, 1.0]], dtype=np.float32)
    assert S.places(scores).tolist() == [[1, 0, 2, 3], [0, 1, 2, 3]]                        # tied rows keep their index order


def test_pointers():
    x = torch.arange(8, dtype=torch.float32)
    assert S.ptr(None) is None and S.ptr(x).value == x.data_ptr() and S.ptr(x, 12).value == x.data_ptr() + 12


# ---- dump and compare ----------------------------------------------------------------------------------------------------------------
def _diff(a, b):
    r = subprocess.run([sys.executable, os.path.join(TESTS, "_dump.py"), "diff", str(a), str(b)], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout


def test_dump_diff(tmp_path):
    import _dump
    base = {"a.s": np.arange(6, dtype=np.uint32), "a.i": np.arange(6, dtype=np.int32).reshape(2, 3), "digest": np.zeros(32, dtype=np.uint8)}
    for name, arrays in (("one", base), ("same", base), ("moved", dict(base, **{"a.s": np.where(np.arange(6) == 4, 9, base["a.s"]).astype(np.uint32)})),
                         ("short", {k: v for k, v in base.items() if k != "a.i"}), ("retyped", dict(base, **{"a.i": base["a.i"].view(np.float32)}))):
        np.savez(tmp_path / f"{name}.npz", **arrays)
    p = lambda name: tmp_path / f"{name}.npz"  # noqa: E731
    rc, out = _diff(p("one"), p("same"))
    assert rc == 0 and "3 arrays in" in out and "3 equal bit for bit" in out and "differ: 0" in out and "a.s" not in out
    rc, out = _diff(p("one"), p("moved"))
    assert rc == 1 and "differ: 1\n  a.s" in out and "a.i" not in out and "2 equal bit for bit" in out
    rc, out = _diff(p("one"), p("short"))
    assert rc == 1 and f"only in {p('one')}: 1\n  a.i" in out and f"only in {p('short')}: 0" in out and "differ: 0" in out
    rc, out = _diff(p("short"), p("one"))
    assert rc == 1 and f"only in {p('one')}: 1\n  a.i" in out
    rc, out = _diff(p("one"), p("retyped"))
    assert rc == 1 and "differ: 1\n  a.i" in out                                            # the same bytes under another dtype
    assert subprocess.run([sys.executable, os.path.join(TESTS, "_dump.py"), "diff", str(p("one"))], capture_output=True).returncode != 0
    small, large = torch.arange(16384, dtype=torch.float32), torch.arange(16385, dtype=torch.float32)
    assert _dump.raw(small).shape == (65536,) and _dump.raw(small).tobytes() == small.numpy().tobytes()
    assert _dump.raw(large).tobytes() == hashlib.sha256(large.numpy().tobytes()).digest()

"""tests/framed.py on CPU tensors: the detector must be able to fail.  A torch "kernel" that writes one element outside the view -- a gap
column, row `rows`, the element before the view -- makes assert_intact raise and name the place; a correct one does not; the view aliases
the body at the offsets the ABI's (pointer, ld) pair describes."""
import pytest
import torch

from framed import BAND_ROWS, E8M0_HUGE, FP8_NAN, NAN, SENTINEL, Framed, framed_like, framed_vec

DTYPES = [torch.float32, torch.bfloat16, torch.uint8, torch.int32]


def _value(dtype):
    return torch.tensor(3, dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("gap", [0, 1, 32])
def test_view_aliases_the_body_at_the_right_offsets(dtype, gap):
    rows, cols = 5, 7
    ld = cols + gap
    f = Framed(rows, cols, ld, dtype, SENTINEL)
    assert f.view.shape == (rows, cols) and f.view.stride() == (ld, 1)
    assert f.view.data_ptr() % 16 == 0
    assert f.band >= BAND_ROWS * ld and (f.band * f.itemsize) % 16 == 0
    assert f.flat.numel() == 2 * f.band + rows * ld
    assert f.view.data_ptr() == f.flat.data_ptr() + f.band * f.itemsize
    t = torch.arange(rows * cols).reshape(rows, cols).to(dtype)
    f.load(t)
    for r in (0, 2, rows - 1):
        for c in (0, 3, cols - 1):
            assert f.flat[f.band + r * ld + c] == t[r, c]             # element (r, c) sits at pointer + r * ld + c
    assert torch.equal(f.contiguous(), t) and f.contiguous().is_contiguous()
    f.assert_intact("after load")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_correct_kernel_leaves_the_frame_intact(dtype):
    f = Framed(4, 6, 9, dtype, SENTINEL)
    f.view.fill_(_value(dtype))                                       # every element of the view, nothing else
    f.view[3, 5] = _value(dtype) + 1
    f.assert_intact()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["gap column", "row rows", "before the view", "last gap column of the last row", "first band element",
                                   "last band element"])
def test_one_stray_element_is_reported(dtype, where):
    rows, cols, ld = 4, 6, 9
    f = Framed(rows, cols, ld, dtype, SENTINEL)
    f.view.fill_(_value(dtype))
    at = {"gap column": (1, cols), "row rows": (rows, 0), "before the view": (-1, ld - 1), "last gap column of the last row": (rows - 1, ld - 1)}
    if where == "first band element":
        idx = 0
    elif where == "last band element":
        idx = f.total - 1
    else:
        idx = f.band + at[where][0] * ld + at[where][1]
    f.flat[idx] = _value(dtype)
    with pytest.raises(AssertionError) as e:
        f.assert_intact("stray")
    first = idx - f.band
    assert f"(row {first // ld}, column {first % ld})" in str(e.value) and "stray" in str(e.value)


def test_the_comparison_is_on_bytes_not_on_floats():
    """A NaN moat compares unequal to itself as a float, and -0.0 equals 0.0: neither may confuse the detector."""
    f = Framed(3, 4, 8, torch.float32, NAN)
    assert torch.isnan(f.flat[:f.band]).all() and torch.isnan(f.flat[f.band + 4:f.band + 8]).all()
    f.view.fill_(1.0)
    f.assert_intact()                                                 # NaN != NaN as floats; the bytes are the pattern
    assert f.flat[:1].view(torch.int32).item() == 0x7FC00000
    f.flat[f.band + 5:f.band + 6].view(torch.int32).fill_(0x7FC00001)  # another NaN: a float compare with NaN-awareness would pass it
    with pytest.raises(AssertionError, match=r"row 0, column 5"):
        f.assert_intact()
    z = Framed(2, 2, 3, torch.float32, 0x00)
    z.flat[z.band + 2] = -0.0                                          # equal to the 0.0 fill as a float, one bit apart
    with pytest.raises(AssertionError, match=r"row 0, column 2"):
        z.assert_intact()
    h = Framed(2, 2, 3, torch.bfloat16, NAN)
    assert h.flat[:1].view(torch.int16).item() == 0x7FC0 and torch.isnan(h.flat[0])
    h.flat[h.band + 2:h.band + 3].view(torch.uint8)[0] = 0xC1         # ONE byte of a two-byte element
    with pytest.raises(AssertionError, match=r"row 0, column 2"):
        h.assert_intact()


def test_fill_bytes_of_the_operand_forms():
    assert torch.isnan(Framed(1, 1, 1, torch.uint8, FP8_NAN).flat[:1].view(torch.float8_e4m3fn).float()).all()
    assert Framed(1, 1, 1, torch.uint8, E8M0_HUGE).flat[0].item() == 0xFE
    assert Framed(1, 1, 1, torch.float32, SENTINEL).flat[:1].view(torch.int32).item() == -0x5A5A5A5B      # 0xA5A5A5A5
    with pytest.raises(ValueError):
        Framed(1, 1, 1, torch.uint8, NAN)
    with pytest.raises(ValueError):
        Framed(2, 4, 3, torch.float32, SENTINEL)                      # ld < cols is not a frame


def test_vectors_and_copies():
    b = torch.arange(5, dtype=torch.float32)
    v = framed_vec(b, NAN)
    assert torch.equal(v.view[0], b) and torch.isnan(v.flat[v.band + 5:v.band + 5 + 64]).all() and torch.isnan(v.flat[v.band - 64:v.band]).all()
    v.assert_intact()
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    f = framed_like(t, 6, SENTINEL)
    assert torch.equal(f.view, t) and f.view.stride() == (6, 1)
    with pytest.raises(TypeError):
        f.load(t.double())

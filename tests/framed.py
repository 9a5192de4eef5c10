"""Framed buffers for kernel-ABI tests: a strided [rows, cols] view (leading dimension ld >= cols) inside ONE flat allocation laid out as

    guard band | body of rows * ld elements | guard band

Every byte outside the view -- both bands and the gap columns cols .. ld of every body row -- holds a known pattern, so a kernel that writes
outside its logical output changes a byte `assert_intact` looks at, and a kernel that reads outside its logical input reads the pattern.
Each band is at least 256 rows of ld elements (one full workgroup tile of the largest GEMM configuration), so a kernel that ignores an M
or N tail scribbles on pattern inside the allocation: the test fails, nothing unmapped is touched.

Fill patterns:
    SENTINEL (byte 0xA5)   output frames (the suite's sentinel: tests/test_gpu_quant_producers.py)
    NAN                    input moats of fp32 / bf16 operands: the quiet NaN of the element type
    FP8_NAN (byte 0x7F)    input moats of e4m3fn bytes (S.1111.111 is e4m3fn's NaN)
    E8M0_HUGE (byte 0xFE)  input moats of E8M0 scale bytes: 2^127, far outside every tolerance if it is ever applied

A plain module (no fixtures): works on CPU tensors too (tests/test_framed_cpu.py shows that the detector can fail).
"""
import torch

SENTINEL = 0xA5
FP8_NAN = 0x7F
E8M0_HUGE = 0xFE
NAN = "nan"
BAND_ROWS = 256

_QNAN_BYTES = {torch.float32: (0x00, 0x00, 0xC0, 0x7F), torch.bfloat16: (0xC0, 0x7F)}      # little endian


class Framed:
    def __init__(self, rows, cols, ld, dtype, fill, device="cpu"):
        if rows < 1 or cols < 1 or ld < cols:
            raise ValueError(f"need rows >= 1, 1 <= cols <= ld, got rows {rows} cols {cols} ld {ld}")
        self.rows, self.cols, self.ld, self.dtype = int(rows), int(cols), int(ld), dtype
        self.itemsize = torch.empty(0, dtype=dtype).element_size()
        if fill == NAN:
            if dtype not in _QNAN_BYTES:
                raise ValueError(f"no NaN pattern for {dtype}: give a fill byte")
            pattern = _QNAN_BYTES[dtype]
        else:
            pattern = (int(fill) & 0xFF,) * self.itemsize
        per16 = 16 // self.itemsize                                       # bands are a multiple of 16 bytes: the view starts 16-byte aligned
        self.band = (BAND_ROWS * self.ld + per16 - 1) // per16 * per16      # elements per band
        self.total = 2 * self.band + self.rows * self.ld
        self._pattern = torch.tensor(pattern, dtype=torch.uint8, device=device)
        self._bytes = self._pattern.repeat(self.total)                    # flat uint8 storage, [total * itemsize]
        self.flat = self._bytes.view(dtype)                               # the same storage as `total` elements
        self.view = torch.as_strided(self.flat, (self.rows, self.cols), (self.ld, 1), self.band)
        assert self.view.data_ptr() % 16 == 0

    def load(self, t):
        """Copy `t` ([rows, cols], or anything that reshapes to it) into the view; returns self."""
        t = torch.as_tensor(t)
        if t.dtype != self.dtype:
            raise TypeError(f"expected {self.dtype}, got {t.dtype}")
        self.view.copy_(t.reshape(self.rows, self.cols).to(self.view.device))
        return self

    def contiguous(self):
        """An unframed, contiguous copy of the view's contents."""
        return self.view.contiguous().clone()

    def data_ptr(self):
        return self.view.data_ptr()

    def assert_intact(self, what="frame"):
        """Every BYTE outside the view still holds the fill pattern: both bands and columns cols .. ld of every body row."""
        bad = (self._bytes.view(self.total, self.itemsize) != self._pattern).any(dim=1)       # per element
        body = bad[self.band:self.band + self.rows * self.ld].view(self.rows, self.ld)
        body[:, :self.cols] = False                                                         # the view itself is the kernel's to write
        if bool(bad.any()):
            first = int(torch.nonzero(bad)[0, 0]) - self.band
            row, col = first // self.ld, first % self.ld
            n_bad = int(bad.sum())
            raise AssertionError(f"{what}: {n_bad} element(s) outside the [{self.rows}, {self.cols}] view (ld {self.ld}) were written; "
                                 f"the first is (row {row}, column {col})")


def framed_like(t, ld, fill, device=None):
    """A frame around a copy of the 2-D tensor `t` with leading dimension `ld`."""
    return Framed(t.shape[0], t.shape[1], ld, t.dtype, fill, t.device if device is None else device).load(t)


def framed_vec(t, fill, device=None):
    """A 1-D operand (bias [N], scale [M]) with a moat on both sides (>= 256 elements, the issue asks for >= 64 after the last one);
    `.view[0]` is the vector."""
    t = torch.as_tensor(t).reshape(1, -1)
    return Framed(1, t.shape[1], t.shape[1], t.dtype, fill, t.device if device is None else device).load(t)

"""The key-streaming attention kernels (csrc/attn.hip: attn_f32_stream_kernel / attn_bf16_stream_kernel), which take over past 224 keys:
accuracy against fp64 softmax attention under the budgets of the resident kernels' tests, bit identity with the resident kernels on
the shapes both take (FERN_ATTN_STREAM=1 in one child process), and batch invariance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gemm_refs import attn_ref, e4m3_code, e8m0_byte, mx_scales_by_block
from oracle.clip import mx8_dequantize
from support import close, rand

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


LONG_CASES = [  # batch, heads, hd, s_q, s_k (non-causal)
    (2, 16, 64, 257, 257), (1, 16, 64, 577, 577), (2, 4, 32, 290, 290), (1, 2, 96, 300, 300), (2, 8, 80, 290, 290),
    (2, 3, 64, 40, 1030), (1, 2, 64, 1000, 257), (1, 2, 64, 225, 225), (1, 2, 80, 1, 300), (1, 1, 32, 33, 4096)]


@pytest.mark.parametrize("b,heads,hd,sq,sk", LONG_CASES)
def test_attention_long(engine, b, heads, hd, sq, sk):
    w = heads * hd
    q, k, v = rand(b, sq, w, seed=1), rand(b, sk, w, seed=2), rand(b, sk, w, seed=3)
    scale = hd ** -0.5
    close(engine.attention(q, k, v, heads, scale=scale), attn_ref(q, k, v, heads, False, scale), rel=2e-5)


def test_attention_long_sharp_softmax(engine):
    """Large logits at 577 keys: the running-max rescale must be exact when the maximum moves between key tiles and across the
    staged chunks -- one spike in the first chunk, one in the last."""
    b, heads, hd, s = 1, 2, 64, 577
    w = heads * hd
    q, k, v = rand(b, s, w, seed=4), rand(b, s, w, seed=5), rand(b, s, w, seed=6)
    k[:, 570] = q[:, 5] * 4.0          # query 5 sees a huge score at key 570 (the last chunk) after small ones
    k[:, 3] = q[:, 400] * 4.0          # and query 400 at key 3 (the first chunk)
    close(engine.attention(q, k, v, heads, scale=1.0), attn_ref(q, k, v, heads, False, 1.0), rel=5e-5)


def test_attention_refuses_more_than_4096_keys(engine):
    from fashionern_aaai2024_amd._lib import FernError
    q, k = torch.zeros(1, 4, 64), torch.zeros(1, 4097, 64)
    with pytest.raises(FernError):
        engine.attention(q, k, k, 1)
    with pytest.raises(FernError, match="bad shape"):
        engine.attention_mx8(torch.zeros(1, 4, 128).bfloat16().cuda(), torch.zeros(1, 4097, 128).bfloat16().cuda(),
                             torch.zeros(1, 4097, 128).bfloat16().cuda(), 4)


@pytest.mark.parametrize("b,heads,hd,sq,sk", [c for c in LONG_CASES if c[2] % 8 == 0])
def test_attention_bf16_long(engine, b, heads, hd, sq, sk):
    """bf16 operand attention against fp64 softmax attention on the SAME bf16-rounded q, k, v (test_attention_bf16's budget)."""
    g = torch.Generator().manual_seed(b * 100 + heads * 10 + hd + sq)
    w = heads * hd
    q, k, v = (torch.randn(b, s, w, generator=g).bfloat16() for s in (sq, sk, sk))
    got = engine.attention_bf16(q.cuda(), k.cuda(), v.cuda(), heads)
    assert got.dtype == torch.bfloat16
    ref = attn_ref(q, k, v, heads, False, hd ** -0.5)
    err = (got.float().cpu().double() - ref).abs().max().item()
    print(f"bf16 attention err {err:.3e} (bound {2 ** -7 * max(1.0, ref.abs().max().item()):.3e})")
    assert err < 2 ** -7 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("b,heads,hd,s", [(2, 16, 64, 257), (1, 4, 32, 577)])
def test_attention_mx8_output_long(engine, b, heads, hd, s):
    """The streaming kernel's block-scaled output under the two assertions of test_attention_mx8_output: (a) consistent with the
    bf16 output of the same call shape (the same kernel instance, another store), (b) within the bf16 budget plus half an e4m3 step of
    fp64 attention.  Written with ldo > width and scale_rows > rows: the gap columns and padding rows stay untouched."""
    g = torch.Generator().manual_seed(b * 100 + heads * 10 + hd + s)
    w = heads * hd
    q, k, v = (torch.randn(b, s, w, generator=g).bfloat16() for _ in range(3))
    v[..., :32] *= 30.0                                                     # an outlier block of the output
    rows = b * s
    ldo = w + 32
    out = torch.full((rows, ldo), SENTINEL, dtype=torch.uint8, device="cuda")
    scales = torch.full((w // 128, rows + 3, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    y8, sc = engine.attention_mx8(q.cuda(), k.cuda(), v.cuda(), heads, out=out, scales=scales)
    yb = engine.attention_bf16(q.cuda(), k.cuda(), v.cuda(), heads).cpu().reshape(rows, w)
    y8 = y8.cpu()
    assert (y8[:, w:] == SENTINEL).all(), "bytes beyond the width were written"
    y8 = y8[:, :w].int()
    sc = sc.cpu()
    assert (sc[:, rows:] == SENTINEL).all(), "scale bytes beyond `rows` were written"
    e = mx_scales_by_block(sc[:, :rows]).int()
    # (a) consistency with the bf16 output of the same kernel
    nb = w // 32
    bb = yb.double().reshape(rows, nb, 32)
    half = lambda t: torch.ldexp(torch.ones((), dtype=torch.float64), torch.frexp(t.float())[1] - 9)   # half a bf16 ulp of |t|
    m = bb.abs().amax(-1)
    e_lo, e_hi = e8m0_byte(m - half(m)), e8m0_byte(m + half(m))
    sure = e_lo == e_hi
    assert torch.equal(e[sure], e8m0_byte(m)[sure]), "scale byte differs from the bf16 output's block maximum"
    assert ((e >= e_lo) & (e <= e_hi)).all()
    scl = torch.ldexp(torch.ones((), dtype=torch.float64), 127 - e).unsqueeze(-1)
    hb = half(bb.abs())
    c_ref, _ = e4m3_code(bb * scl)
    c_lo, o_lo = e4m3_code((bb - hb) * scl)
    c_hi, o_hi = e4m3_code((bb + hb) * scl)
    got = y8.reshape(rows, nb, 32)
    o_got = torch.where(got >= 128, -(got & 0x7F), got)
    excused = c_lo != c_hi
    assert torch.equal(got[~excused], c_ref[~excused]), "element byte differs from e4m3 of the bf16 output"
    assert ((o_got >= torch.minimum(o_lo, o_hi)) & (o_got <= torch.maximum(o_lo, o_hi)))[excused].all()
    frac = (excused & (got != c_ref)).sum().item() / got.numel()
    print(f"attention mx8 b={b} heads={heads} hd={hd} s={s}: excused fraction {frac:.3%}")
    assert frac < 0.05
    # (b) against fp64 attention on the same bf16 operands
    ref = attn_ref(q, k, v, heads, False, hd ** -0.5).reshape(rows, w)
    dq = mx8_dequantize(y8.to(torch.uint8).view(torch.float8_e4m3fn), e.to(torch.uint8), torch.float64)
    step = 2.0 ** -4 * torch.maximum(dq.abs(), ref.abs()) + torch.ldexp(torch.ones((), dtype=torch.float64), e - 137).repeat_interleave(32, -1)
    budget = 2 ** -7 * max(1.0, ref.abs().max().item())
    assert ((dq - ref).abs() <= budget + step).all(), ((dq - ref).abs() - step).max().item()


def test_streaming_kernels_are_bit_identical_to_the_resident_ones(engine, tmp_path):
    """FERN_ATTN_STREAM=1 (read once per process: one fresh child) sends the shapes of the resident / chunked kernels through the
    streaming form; the bits must equal this process's, which runs them on the kernels they always had."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _attn_stream_dump as dump
    assert os.environ.get("FERN_ATTN_STREAM", "0") != "1", "the parent must run the resident kernels"
    path = str(tmp_path / "stream.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_attn_stream_dump.py"), path], cwd=ROOT,
                       env=dict(os.environ, FERN_ATTN_STREAM="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child, mine = np.load(path), dump.compute(engine)
    assert bool(child["stream_switch"][0]), "the child did not see FERN_ATTN_STREAM=1"
    assert sorted(f for f in child.files if f != "stream_switch") == sorted(mine)
    assert len(mine) == len(dump.F32_SHAPES) + len(dump.BF16_SHAPES) + 2 * len(dump.MX_SHAPES)      # MX: bytes and scale bytes
    assert (len(dump.F32_SHAPES), len(dump.BF16_SHAPES), len(dump.MX_SHAPES)) == (7, 6, 3)
    for name, bits in mine.items():
        assert torch.equal(torch.from_numpy(child[name].astype(np.int64)), torch.from_numpy(bits.astype(np.int64))), name


def test_streaming_attention_is_batch_invariant(engine):
    """(3, 16, 64, 257, 257): batch row 1 computed alone equals row 1 of the full call, bit for bit, fp32 and bf16."""
    b, heads, hd, s = 3, 16, 64, 257
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(b, s, heads * hd, generator=g) for _ in range(3))
    full = engine.attention(q, k, v, heads)
    assert torch.equal(engine.attention(q[1:2], k[1:2], v[1:2], heads), full[1:2])
    qb, kb, vb = (t.bfloat16().cuda() for t in (q, k, v))
    fullb = engine.attention_bf16(qb, kb, vb, heads)
    oneb = engine.attention_bf16(qb[1:2].contiguous(), kb[1:2].contiguous(), vb[1:2].contiguous(), heads)
    assert torch.equal(oneb.view(torch.int16), fullb[1:2].view(torch.int16))

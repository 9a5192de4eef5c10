"""The GEMM families' test operands, fp64 references and bounds, shared by tests/test_gpu_kernels.py (contiguous calls through the
engine wrappers) and tests/test_gpu_frames.py (framed, strided calls through the ABI).  One statement of each, so that a new shape
is held to the bound the family has always been held to.

Each `*_case` returns the operands and `base` = the fp64 value of A W^T + bias on the operands the kernel actually multiplies (rounded /
quantised ones for the reduced families); `epi_ref` applies the epilogue."""
import torch
import torch.nn.functional as F

from support import close, rand  # noqa: F401  (the shared inputs and the fp32 kernels' bound: re-exported, the families below use them)

EPI_BIAS, EPI_GELU, EPI_RELU, EPI_RESIDUAL, EPI_QUICKGELU = 0, 1, 2, 3, 4


def epi_ref(base, epi, r=None):
    """fp64: the epilogue applied to `base` (r: the residual, any float dtype)."""
    if epi == EPI_GELU:
        return F.gelu(base)
    if epi == EPI_RELU:
        return F.relu(base)
    if epi == EPI_RESIDUAL:
        return base + r.double()
    if epi == EPI_QUICKGELU:
        return base * torch.sigmoid(1.702 * base)
    return base


# ---- fp32 ------------------------------------------------------------------------------------------------------------------------
def f32_case(M, N, K):
    a, w, b, r = rand(M, K, seed=1), rand(N, K, seed=2, scale=K ** -0.5), rand(N, seed=3), rand(M, N, seed=4)
    return a, w, b, r, a.double() @ w.double().T + b.double()


# ---- bf16 operands ---------------------------------------------------------------------------------------------------------------
def bf16_case(m, n, k, epi):
    """fp64 math on the SAME rounded operands: only the fp32 accumulation order differs."""
    g = torch.Generator().manual_seed(m * 7 + n + k + epi)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) * k ** -0.5
    b = torch.randn(n, generator=g)
    r = torch.randn(m, n, generator=g)
    ab, wb = a.bfloat16(), w.bfloat16()
    return a, ab, wb, b, r, ab.double() @ wb.double().T + b.double()


def check_fp8_family(got, ref, out_bf16):
    """Per-row and block-scaled fp8 operands.  bf16 output: <= 1 bf16 ulp, as the bf16 family.  fp32 output: 1e-4 relative --
    v_mfma_f32_32x32x16_fp8_fp8 is exact on integer data but does not sum its 16 products as a plain fp32 FMA chain: on random
    operands it sits ~1.4e-5 (rms, relative) from the exact sum, independent of K."""
    if out_bf16:
        assert got.dtype == torch.bfloat16 and torch.allclose(got.float().cpu().double(), ref, rtol=2 ** -7, atol=1e-3)
    else:
        assert got.dtype == torch.float32
        assert (got.cpu().double() - ref).abs().max().item() < 1e-4 * max(1.0, ref.abs().max().item())


def check_bf16_family(got, ref, out_bf16):
    """bf16 output: one bf16 rounding of a value the fp32 accumulation may have moved across a rounding boundary: <= 1 bf16 ulp."""
    assert got.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
    if out_bf16:
        assert torch.allclose(got.float().cpu().double(), ref, rtol=2 ** -7, atol=1e-3)
    else:
        assert torch.allclose(got.cpu().double(), ref, rtol=1e-5, atol=2e-5)


# ---- fp8 operands, per-row scales ------------------------------------------------------------------------------------------------
def fp8_case(engine, m, n, k, epi):
    """fp64 math on the SAME quantised operands and scales (the engine's own quantiser, pinned bit-exactly elsewhere)."""
    g = torch.Generator().manual_seed(m + n + k + epi)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) * k ** -0.5
    b = torch.randn(n, generator=g)
    r = torch.randn(m, n, generator=g)
    a8, sa = engine.quantize_rows_fp8(a)
    w8, sw = engine.quantize_rows_fp8(w)
    qa, qw = a8.cpu().view(torch.float8_e4m3fn).double(), w8.cpu().view(torch.float8_e4m3fn).double()
    base = (qa @ qw.T) * (sa.cpu().double().unsqueeze(1) * sw.cpu().double().unsqueeze(0)) + b.double()
    return a8, sa, w8, sw, b, r, base, g


# ---- block-scaled fp8 operands -----------------------------------------------------------------------------------------------------
def mx_scales_by_block(sc):
    """engine.quantize_mx8's [D/128, R, 4] scale array -> [R, D/32] (block b = k // 32)."""
    return sc.permute(1, 0, 2).reshape(sc.shape[1], -1)


def e8m0_byte(m):
    """E8M0 scale byte of fp32 block maxima, as the kernels compute it (csrc/kernels.h: mx_scale_byte): the exponent that brings the
    maximum under 448, one more past the 0x600000 mantissa (1.75 x 2^e > 448 x 2^(e-8)), clamped to [1, 253]."""
    u = m.float().contiguous().view(torch.int32)
    return ((u >> 23) - 8 + ((u & 0x7FFFFF) > 0x600000).int()).clamp(1, 253)


def e4m3_code(v):
    """e4m3fn bytes of fp32 values (round to nearest even) as int, and their signed position on the code line."""
    b = v.float().to(torch.float8_e4m3fn).view(torch.uint8).int()
    return b, torch.where(b >= 128, -(b & 0x7F), b)


def mx8_case(engine, m, n, k, epi):
    from oracle.clip import mx8_dequantize
    g = torch.Generator().manual_seed(m + n + k + epi)
    a = torch.randn(m, k, generator=g) * torch.logspace(-1, 1, k // 32).repeat_interleave(32)     # blocks of different magnitude
    w = torch.randn(n, k, generator=g) * k ** -0.5
    b = torch.randn(n, generator=g)
    r = torch.randn(m, n, generator=g)
    a8, sa = engine.quantize_mx8(a)
    w8, sw = engine.quantize_mx8(w)
    qa = mx8_dequantize(a8.cpu().view(torch.float8_e4m3fn), mx_scales_by_block(sa.cpu()), torch.float64)
    qw = mx8_dequantize(w8.cpu().view(torch.float8_e4m3fn), mx_scales_by_block(sw.cpu()), torch.float64)
    return a8, sa, w8, sw, b, r, qa @ qw.T + b.double(), g


# ---- attention ---------------------------------------------------------------------------------------------------------------------
def attn_ref(q, k, v, heads, causal, scale):
    """fp64 softmax attention: q [B,Sq,W], k / v [B,Sk,W] (any float dtype: the values as given) -> [B,Sq,W]."""
    b, sq, w = q.shape
    sk, hd = k.shape[1], w // heads
    qh = q.double().view(b, sq, heads, hd).transpose(1, 2) * scale
    kh = k.double().view(b, sk, heads, hd).transpose(1, 2)
    vh = v.double().view(b, sk, heads, hd).transpose(1, 2)
    att = qh @ kh.transpose(-1, -2)
    if causal:
        att = att + torch.full((sq, sk), float("-inf"), dtype=torch.float64).triu(1)
    return (torch.softmax(att, -1) @ vh).transpose(1, 2).reshape(b, sq, w)

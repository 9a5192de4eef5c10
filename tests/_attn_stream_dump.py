"""Helper of test_streaming_kernels_are_bit_identical_to_the_resident_ones: computes a fixed set of attention shapes from seeded inputs
with whatever FERN_ATTN_STREAM selects and saves the raw results.  Usage: python tests/_attn_stream_dump.py out.npz

`--builds out.npz` saves compute() plus compute_builds(): a second list for comparing two BUILDS of the library (a change to
csrc/attn.hip that must not move a bit), with the shapes the resident-vs-stream comparison cannot take: causal, one query tile
of 13, the chunked kernel's 197, s_q != s_k on the streaming form."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

F32_SHAPES = [(2, 12, 64, 197, 197), (1, 12, 64, 224, 224), (2, 8, 80, 91, 91), (2, 2, 16, 5, 40)]
BF16_SHAPES = [(3, 12, 64, 197, 197), (2, 2, 64, 224, 224), (1, 2, 80, 91, 91)]
# 257 keys: only the streaming form takes it, in either process -- the child's streaming kernels are seen to run and to agree with the parent's
F32_SHAPES.append((1, 4, 64, 257, 257))
BF16_SHAPES.append((1, 4, 64, 257, 257))
# every head_dim padding (32, 64, 96), s_q != s_k, one key tile and several
F32_SHAPES += [(1, 2, 96, 70, 70), (1, 3, 32, 33, 33)]
BF16_SHAPES += [(1, 2, 32, 40, 100), (1, 2, 96, 65, 65)]
# attention_mx8: e4m3 bytes and E8M0 scale bytes (heads * hd is a multiple of 128 on this entry, so head_dim 32 comes with four heads)
MX_SHAPES = [(2, 4, 64, 197, 197), (1, 4, 32, 91, 91), (1, 4, 64, 257, 257)]

# build-against-build list: batch, heads, hd, s_q, s_k[, causal]
BUILD_F32_SHAPES = [(3, 8, 64, 77, 77, True), (1, 1, 32, 33, 33, True), (2, 2, 96, 70, 70, True), (2, 8, 80, 13, 13), (2, 12, 64, 197, 197),
                    (1, 2, 64, 1000, 257)]
BUILD_BF16_SHAPES = [c for c in BUILD_F32_SHAPES if c[2] % 8 == 0]
BUILD_MX_SHAPES = MX_SHAPES


def _run(eng, prefix, f32, bf16, mx, seed):
    out = {}
    for i, (b, heads, hd, sq, sk, *causal) in enumerate(f32):
        g = torch.Generator().manual_seed(seed + 100 + i)
        q, k, v = (torch.randn(b, s, heads * hd, generator=g) for s in (sq, sk, sk))
        got = eng.attention(q, k, v, heads, causal=bool(causal and causal[0]))
        out[f"{prefix}f32_{b}_{heads}_{hd}_{sq}_{sk}"] = got.cpu().numpy().view(np.uint32)
    for i, (b, heads, hd, sq, sk, *causal) in enumerate(bf16):
        g = torch.Generator().manual_seed(seed + 200 + i)
        q, k, v = (torch.randn(b, s, heads * hd, generator=g).bfloat16() for s in (sq, sk, sk))
        got = eng.attention_bf16(q.cuda(), k.cuda(), v.cuda(), heads, causal=bool(causal and causal[0]))
        out[f"{prefix}bf16_{b}_{heads}_{hd}_{sq}_{sk}"] = got.view(torch.int16).cpu().numpy()
    for i, (b, heads, hd, sq, sk) in enumerate(mx):
        g = torch.Generator().manual_seed(seed + 300 + i)
        q, k, v = (torch.randn(b, s, heads * hd, generator=g).bfloat16() for s in (sq, sk, sk))
        y8, sc = eng.attention_mx8(q.cuda(), k.cuda(), v.cuda(), heads)
        out[f"{prefix}mx_{b}_{heads}_{hd}_{sq}_{sk}"] = y8.view(torch.uint8).cpu().numpy()
        out[f"{prefix}mxscales_{b}_{heads}_{hd}_{sq}_{sk}"] = sc.view(torch.uint8).cpu().numpy()
    return out


def compute(eng):
    """{name: int array of the raw output bits}; the same seeded inputs in every process."""
    return _run(eng, "", F32_SHAPES, BF16_SHAPES, MX_SHAPES, 0)


def compute_builds(eng):
    """The build-against-build list, in the same form."""
    return _run(eng, "build_", BUILD_F32_SHAPES, BUILD_BF16_SHAPES, BUILD_MX_SHAPES, 1000)


def _everything(eng):
    arrays = dict(stream_switch=np.array([os.environ.get("FERN_ATTN_STREAM") == "1"]), **compute(eng))
    if sys.argv[1] == "--builds":
        arrays.update(compute_builds(eng))
    return arrays


if __name__ == "__main__":
    import _dump
    _dump.main(_everything)

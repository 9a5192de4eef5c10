"""Helper of test_streaming_kernels_are_bit_identical_to_the_resident_ones: computes a fixed set of attention shapes from seeded inputs
with whatever FERN_ATTN_STREAM selects and saves the raw results.  Usage: python tests/_attn_stream_dump.py out.npz"""
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


def compute(eng):
    """{name: int array of the raw output bits}; the same seeded inputs in every process."""
    out = {}
    for i, (b, heads, hd, sq, sk) in enumerate(F32_SHAPES):
        g = torch.Generator().manual_seed(100 + i)
        q, k, v = (torch.randn(b, s, heads * hd, generator=g) for s in (sq, sk, sk))
        out[f"f32_{b}_{heads}_{hd}_{sq}_{sk}"] = eng.attention(q, k, v, heads).cpu().numpy().view(np.uint32)
    for i, (b, heads, hd, sq, sk) in enumerate(BF16_SHAPES):
        g = torch.Generator().manual_seed(200 + i)
        q, k, v = (torch.randn(b, s, heads * hd, generator=g).bfloat16() for s in (sq, sk, sk))
        got = eng.attention_bf16(q.cuda(), k.cuda(), v.cuda(), heads)
        out[f"bf16_{b}_{heads}_{hd}_{sq}_{sk}"] = got.view(torch.int16).cpu().numpy()
    return out


if __name__ == "__main__":
    from fashionern_aaai2024_amd.engine import FernEngine
    np.savez(sys.argv[1], stream_switch=np.array([os.environ.get("FERN_ATTN_STREAM") == "1"]), **compute(FernEngine("cuda:0")))

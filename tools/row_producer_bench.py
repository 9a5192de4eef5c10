#!/usr/bin/env python
"""The row producers of csrc/elem.hip alone at the towers' shapes (LayerNorm into every operand form, the two plain quantisers, im2col):
time per launch from stream events around `iters` launches after a warm-up.  python tools/row_producer_bench.py [iters 100]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fashionern_aaai2024_amd.engine import FernEngine, QFORM_BF16, QFORM_FP8, QFORM_MX8  # noqa: E402

eng = FernEngine("cuda:0")
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 100
EPS = 1e-5


def timed(name, fn):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print(f"{name:44s}: {e0.elapsed_time(e1) / iters * 1e3:7.1f} us/launch", flush=True)


for rows, d in ((12608, 768), (4928, 512), (16448, 1024)):
    x = torch.randn(rows, d, device="cuda")
    xb = eng.to_bf16(x)
    gamma, beta = torch.rand(d, device="cuda") + 0.5, torch.randn(d, device="cuda")
    sc = torch.empty(d // 128, rows, 4, dtype=torch.uint8, device="cuda")
    timed(f"layernorm {rows} x {d} fp32 -> fp32", lambda: eng.layernorm(x, gamma, beta, EPS))
    timed(f"layernorm {rows} x {d} fp32 -> bf16", lambda: eng.layernorm_q(x, gamma, beta, EPS, QFORM_BF16))
    timed(f"layernorm {rows} x {d} fp32 -> fp8", lambda: eng.layernorm_q(x, gamma, beta, EPS, QFORM_FP8))
    timed(f"layernorm {rows} x {d} fp32 -> mx8", lambda: eng.layernorm_q(x, gamma, beta, EPS, QFORM_MX8, scales=sc))
    timed(f"layernorm {rows} x {d} bf16 -> mx8", lambda: eng.layernorm_q(xb, gamma, beta, EPS, QFORM_MX8, scales=sc))
x, res = torch.randn(5824, 512, device="cuda"), torch.randn(5824, 512, device="cuda")      # the fusion BERT's post-LN: 64 x 91 tokens
gamma, beta = torch.rand(512, device="cuda") + 0.5, torch.randn(512, device="cuda")
timed("layernorm 5824 x 512 fp32 + residual -> fp32", lambda: eng.layernorm(x, gamma, beta, 1e-12, residual=res))
for rows, d in ((12608, 768), (12608, 3072)):
    xb = eng.to_bf16(torch.randn(rows, d, device="cuda"))
    sc = torch.empty(d // 128, rows, 4, dtype=torch.uint8, device="cuda")
    timed(f"quantize_rows_fp8 {rows} x {d} bf16", lambda: eng.quantize_rows_fp8(xb))
    timed(f"quantize_mx8 {rows} x {d} bf16", lambda: eng.quantize_mx8(xb, scales=sc))
img = torch.randn(64, 3, 224, 224, device="cuda")
sc = torch.empty(768 // 128, 64 * 196, 4, dtype=torch.uint8, device="cuda")
timed("im2col 64 x 224 / 16 -> bf16", lambda: eng.im2col_q(img, 16, QFORM_BF16))
timed("im2col 64 x 224 / 16 -> mx8", lambda: eng.im2col_q(img, 16, QFORM_MX8, scales=sc))
# for the record: rows the half-wave kernel does not take (a stride with ldx % 8 == 4) go to the one-row kernel; no tower has such rows
rows, d = 12608, 768
xs = torch.randn(rows, d + 4, device="cuda")[:, :d]
gamma, beta = torch.rand(d, device="cuda") + 0.5, torch.randn(d, device="cuda")
sc = torch.empty(d // 128, rows, 4, dtype=torch.uint8, device="cuda")
timed(f"layernorm {rows} x {d} fp32 -> mx8, ldx = d + 4", lambda: eng.layernorm_q(xs, gamma, beta, EPS, QFORM_MX8, scales=sc))

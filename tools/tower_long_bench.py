#!/usr/bin/env python
"""ViT-L/14 against ViT-B/16 on one GPU: (1) the attention kernels at the towers' shapes, timed by the dispatches' own timestamps
(fern_prof_*), as TFLOP/s = 4 b heads s_q s_k hd / time -- the streaming forms at 257 / 577 keys beside the resident / chunked kernels at
197; (2) encode_image images/s at b = 64, 20 timed calls after 5 warm-up calls (the mean of one timed window), with the GEMM rate of
one profiled call.  profiles/tower_long_bench.txt holds a run on an MI355X; DESIGN.md 4 reads it.
Usage: python tools/tower_long_bench.py [--batch 64]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fashionern_aaai2024_amd import synth  # noqa: E402
from fashionern_aaai2024_amd.clip_model import create_model  # noqa: E402
from fashionern_aaai2024_amd.engine import FernEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
a = ap.parse_args()

eng = FernEngine("cuda:0")
for label, b, heads, hd, s in (("ViT-B/16 197", 64, 12, 64, 197), ("ViT-L/14 257", 49, 16, 64, 257), ("ViT-L/14@336 577", 21, 16, 64, 577)):
    g = torch.Generator().manual_seed(s)
    q, k, v = (torch.randn(b, s, heads * hd, generator=g).cuda() for _ in range(3))
    qb, kb, vb = (t.bfloat16() for t in (q, k, v))
    for form, fn in (("fp32", lambda: eng.attention(q, k, v, heads)), ("bf16", lambda: eng.attention_bf16(qb, kb, vb, heads)),
                     ("bf16 -> mx8", lambda: eng.attention_mx8(qb, kb, vb, heads))):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        eng.prof_enable(True)
        for _ in range(20):
            fn()
        st = eng.prof_collect()
        eng.prof_enable(False)
        us = st["attn_ms"] / st["attn_launches"] * 1e3
        print(f"attention {label:18s} b={b:2d} {form:12s}: {us:7.1f} us per launch, {st['attn_flops'] / st['attn_ms'] / 1e9:6.1f} TFLOP/s")
eng.close()

for name, precision in (("ViT-B-16", "fp32"), ("ViT-B-16", "mx8img"), ("ViT-L-14", "fp32"), ("ViT-L-14", "mx8img")):
    cfg = synth.CLIP_CONFIGS[name]
    clip = create_model(cfg, device="cuda:0", seed=0, precision=precision)
    e = clip.engine
    imgs = torch.from_numpy(synth.images(a.batch, cfg)).cuda()
    for _ in range(5):
        e.encode_image(imgs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        e.encode_image(imgs)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 20
    e.prof_enable(True)
    e.encode_image(imgs)
    st = e.prof_collect()
    e.prof_enable(False)
    gf = st["gemm_flops"] + st["gemm_bf16_flops"] + st["gemm_mx8_flops"]
    gms = st["gemm_ms"] + st["gemm_bf16_ms"] + st["gemm_mx8_ms"]
    print(f"{name} {precision:7s}: {a.batch / dt:8.1f} images/s ({dt * 1e3:.2f} ms per {a.batch}); GEMM {gf / 1e9:.0f} GFLOP in {gms:.2f} ms = "
          f"{gf / max(gms, 1e-9) / 1e9:.1f} TFLOP/s; attention {st['attn_ms']:.2f} ms in {st['attn_launches']} launches, {st['attn_flops'] / max(st['attn_ms'], 1e-9) / 1e9:.1f} TFLOP/s")
    e.close()

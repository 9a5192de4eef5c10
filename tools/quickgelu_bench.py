#!/usr/bin/env python
"""GELU against QuickGELU on one GPU: the c_fc GEMM of the ViT-B/16 image tower (12608 x 3072 x 768) in the fp32, bf16 and
block-scaled quantising forms, and `encode_image` at b = 64 for ViT-B/16 in fp32 and mx8img (profiles/quickgelu_bench.txt).

Method: every shape is warmed up first (the tuner times its candidates on the first calls of a key); GEMM times are
the dispatches' own begin -> end timestamps summed by the library's profiler (fern_prof_collect), tower times are device events
around `--iters` calls; the two activations ALTERNATE inside one process, `--rounds` (default 3) times, so that a drift of the
box lands on both.  The yardstick is the GELU figure of the same run.
Usage: python tools/quickgelu_bench.py [--rounds 3] [--iters 20] [--skip-towers]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fashionern_aaai2024_amd import synth  # noqa: E402
from fashionern_aaai2024_amd.engine import EPI_BIAS_GELU, EPI_BIAS_QUICKGELU, FernEngine  # noqa: E402

M, N, K = 12608, 3072, 768
ACTS = (("gelu", EPI_BIAS_GELU), ("quick_gelu", EPI_BIAS_QUICKGELU))


def kernel_us(eng, run, iters, field):
    eng.prof_enable(True)
    for _ in range(iters):
        run()
    st = eng.prof_collect()
    eng.prof_enable(False)
    return st[field] * 1e3 / iters


def gemm_section(args):
    eng = FernEngine("cuda:0")
    g = torch.Generator().manual_seed(0)
    a = torch.randn(M, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    ab, wb = eng.to_bf16(a), eng.to_bf16(w)
    (a8, sa), (w8, sw) = eng.quantize_mx8(a), eng.quantize_mx8(w)
    forms = (("fp32", "gemm_ms", lambda epi: eng.gemm(a, w, b, epilogue=epi)),
             ("bf16 (bf16 out)", "gemm_bf16_ms", lambda epi: eng.gemm_bf16(ab, wb, b, epilogue=epi, out_bf16=True)),
             ("mx8 quantising", "gemm_mx8_ms", lambda epi: eng.gemm_mx8_quant(a8, sa, w8, sw, b, epilogue=epi)))
    print(f"c_fc GEMM {M} x {N} x {K}: kernel time per launch (dispatch timestamps), us; {args.rounds} alternating rounds of {args.iters} launches")
    for label, field, fn in forms:
        for _, epi in ACTS:      # warm-up: tuner trials of both keys, code objects
            for _ in range(6):
                fn(epi)
        torch.cuda.synchronize()
        res = {name: [] for name, _ in ACTS}
        for _ in range(args.rounds):
            for name, epi in ACTS:
                res[name].append(kernel_us(eng, lambda: fn(epi), args.iters, field))
        ge, qu = res["gelu"], res["quick_gelu"]
        fl = 2.0 * M * N * K
        print(f"  {label:16s} gelu {' '.join(f'{x:8.1f}' for x in ge)}   quick_gelu {' '.join(f'{x:8.1f}' for x in qu)}   "
              f"median ratio quick/gelu {sorted(qu)[len(qu) // 2] / sorted(ge)[len(ge) // 2]:.3f}   "
              f"({fl / sorted(ge)[len(ge) // 2] / 1e6:.0f} / {fl / sorted(qu)[len(qu) // 2] / 1e6:.0f} TFLOP/s)", flush=True)
    plans = [ln for ln in eng.tuner_export().splitlines() if f" {M} {N} {K} " in ln and not ln.startswith("pair")]
    print("  tuned plans (epi 1 = GELU, 11 = QuickGELU):")
    for ln in plans:
        print("    " + ln)
    eng.close()


def tower_section(args):
    base = synth.CLIP_CONFIGS["ViT-B-16"]
    sd = synth.clip_state_dict(base, seed=0)
    imgs = torch.from_numpy(synth.images(64, base)).cuda()
    print(f"ViT-B/16 encode_image, b = 64: images/s (device events around {args.tower_iters} calls); {args.rounds} alternating rounds")
    for prec in ("fp32", "mx8img"):
        engs = {}
        for name, quick in (("gelu", False), ("quick_gelu", True)):
            eng = FernEngine("cuda:0")
            eng.load_tensors(sd)
            eng.finalize_clip(synth.resolve_clip_config(base, quick))
            eng.set_precision(prec)
            for _ in range(4):
                eng.encode_image(imgs)
            engs[name] = eng
        torch.cuda.synchronize()
        res = {name: [] for name in engs}
        for _ in range(args.rounds):
            for name, eng in engs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.tower_iters):
                    eng.encode_image(imgs)
                e1.record()
                torch.cuda.synchronize()
                res[name].append(64 * args.tower_iters / (e0.elapsed_time(e1) * 1e-3))
        ge, qu = res["gelu"], res["quick_gelu"]
        print(f"  {prec:7s} gelu {' '.join(f'{x:9.1f}' for x in ge)}   quick_gelu {' '.join(f'{x:9.1f}' for x in qu)}   "
              f"median ratio quick/gelu {sorted(qu)[len(qu) // 2] / sorted(ge)[len(ge) // 2]:.3f}", flush=True)
        for eng in engs.values():
            eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20, help="GEMM launches per timed window")
    ap.add_argument("--tower-iters", type=int, default=10, help="encode_image calls per timed window")
    ap.add_argument("--skip-towers", action="store_true")
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}")
    gemm_section(args)
    if not args.skip_towers:
        tower_section(args)


if __name__ == "__main__":
    main()

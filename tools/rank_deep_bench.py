#!/usr/bin/env python
"""Deep-ranking micro-benchmark: fern_sim_topk_deep (K = 100, 1000) beside the K <= 64 stage at K = 50, for the three gallery forms
(fp32 exact, PreparedGallery = certified bf16 pre-filter, bf16 similarity), at 64 x 46 000 x 512 (BASELINE C2) and 64 x 1 000 000 x 512.
Stage time = libfern's own instrumentation (fern_prof_collect: sweep + rest of the stage, dispatch timestamps); wall = back-to-back calls.
Asserts that the pre-filtered form returns the exact form's bits and that the deep lists begin with the K = 50 lists.

    python tools/rank_deep_bench.py [--reps 10] [--only c2,1M]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fashionern_aaai2024_amd.engine import FernEngine  # noqa: E402

SHAPES = [("c2", 64, 46_000, 512), ("1M", 64, 1_000_000, 512)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=str, default=None)
    args = ap.parse_args()
    eng = FernEngine("cuda:0")
    dev = eng.device
    bad = []
    for name, b, n, d in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        g = torch.Generator(device=dev).manual_seed(n + d)
        gal = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device=dev), dim=-1)
        q = torch.nn.functional.normalize(torch.randn(b, d, generator=g, device=dev), dim=-1)
        pg = eng.prepare_gallery(gal)
        forms = (("fp32", gal), ("prefiltered", pg), ("bf16", pg.bf16))
        for k in (50, 100, 1000):
            rec = {"B": b, "N": n, "D": d, "K": k}
            res = {}
            for label, gg in forms:
                if k <= 64:
                    fn = (lambda gg=gg: eng.sim_topk_bf16(q, gg, k)) if label == "bf16" else (lambda gg=gg: eng.sim_topk(q, gg, k))
                else:
                    fn = lambda gg=gg: eng.sim_topk_deep(q, gg, k)
                for _ in range(3):
                    res[label] = fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) / args.reps * 1e6
                eng.prof_enable(True)
                for _ in range(args.reps):
                    fn()
                st = eng.prof_collect()
                eng.prof_enable(False)
                rec[label] = {"stage_us": round((st["sweep_ms"] + st["topk_ms"]) / args.reps * 1e3, 1), "wall_us_per_call": round(wall, 1)}
            if not (torch.equal(res["fp32"][0], res["prefiltered"][0]) and torch.equal(res["fp32"][1], res["prefiltered"][1])):
                bad.append((name, k, "prefiltered != exact"))
            if k == 50:
                k50 = res
            else:
                for label in res:
                    if not torch.equal(res[label][1][:, :50], k50[label][1]):
                        bad.append((name, k, label, "prefix != K=50"))
            print(name, json.dumps(rec), flush=True)
        del gal, pg
        torch.cuda.empty_cache()
    if bad:
        raise SystemExit(f"deep ranking mismatches: {bad}")


if __name__ == "__main__":
    main()

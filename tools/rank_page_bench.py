#!/usr/bin/env python
"""Ranking-pages micro-benchmark: fern_sim_topk_page at offsets 0, 1 024, N / 2 and N - K, fern_rank_select (m = 1) and one cursor
continuation (fern_sim_topk_from), for the fp32 and the bf16 gallery forms at K = 50 and 1 000, at 64 x 46 000 x 512 (BASELINE C2) and
64 x 1 000 000 x 512.  The same process times the two yardsticks on the same gallery: fern_sim_topk_deep at the same K (a page is about
one deep call plus the select passes) and rank_of with m = 1 (a select is about one rank_of).
Stage time = libfern's own instrumentation (fern_prof_collect: sweep + rest of the stage, dispatch timestamps); wall = back-to-back calls.
Asserts that offset 0 returns the deep call's bits and that consecutive cursor pages equal one page at the matching offset.

    python tools/rank_page_bench.py [--reps 10] [--only c2,1M]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fashionern_aaai2024_amd.engine import FernEngine, next_from  # noqa: E402

SHAPES = [("c2", 64, 46_000, 512), ("1M", 64, 1_000_000, 512)]


def timed(eng, fn, reps):
    for _ in range(3):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps * 1e6
    eng.prof_enable(True)
    for _ in range(reps):
        fn()
    st = eng.prof_collect()
    eng.prof_enable(False)
    return out, {"stage_us": round((st["sweep_ms"] + st["topk_ms"]) / reps * 1e3, 1), "wall_us_per_call": round(wall, 1)}


def same(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


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
        gal16 = eng.gallery_to_bf16(gal)
        targets = torch.randint(0, n, (b,), generator=g, device=dev).to(torch.int32)
        for label, gg in (("fp32", gal), ("bf16", gal16)):
            _, rank_of = timed(eng, lambda: eng.rank_of(q, gg, targets), args.reps)
            place = torch.full((b,), n // 2, dtype=torch.int32, device=dev)
            _, select = timed(eng, lambda: eng.rank_select(q, gg, place), args.reps)
            select["vs_rank_of"] = round(select["stage_us"] / rank_of["stage_us"], 2)
            print(name, json.dumps({"B": b, "N": n, "D": d, "form": label, "rank_of_m1": rank_of, "rank_select_m1": select}), flush=True)
            for k in (50, 1000):
                rec = {"B": b, "N": n, "D": d, "form": label, "K": k}
                deep, rec["sim_topk_deep"] = timed(eng, lambda: eng.sim_topk_deep(q, gg, k), args.reps)
                pages = {}
                for off in (0, 1024, n // 2, n - k):
                    pages[off], t = timed(eng, lambda: eng.rank_page(q, gg, off, k), args.reps)
                    t["vs_deep"] = round(t["stage_us"] / rec["sim_topk_deep"]["stage_us"], 2)
                    rec[f"page@{off}"] = t
                cursor = next_from(*pages[n // 2])
                nxt, t = timed(eng, lambda: eng.sim_topk_from(q, gg, k, cursor), args.reps)
                t["vs_deep"] = round(t["stage_us"] / rec["sim_topk_deep"]["stage_us"], 2)
                rec["from_cursor"] = t
                if not same(pages[0], deep):
                    bad.append((name, label, k, "page at offset 0 != sim_topk_deep"))
                if not same(nxt, eng.rank_page(q, gg, n // 2 + k, k)):
                    bad.append((name, label, k, "cursor page != page at the matching offset"))
                first = eng.sim_topk_from(q, gg, k, torch.full((b,), -1, dtype=torch.int64, device=dev))
                second = eng.sim_topk_from(q, gg, k, next_from(*first))
                if not (same(first, deep) and same(second, eng.rank_page(q, gg, k, k))):
                    bad.append((name, label, k, "consecutive cursor pages != pages at offsets 0, K"))
                print(name, json.dumps(rec), flush=True)
        del gal, gal16
        torch.cuda.empty_cache()
    if bad:
        raise SystemExit(f"ranking page mismatches: {bad}")


if __name__ == "__main__":
    main()

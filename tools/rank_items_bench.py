#!/usr/bin/env python
"""Item-level ranking micro-benchmark: FernEngine.sim_topk_items (fern_sim_topk_items, fp32 form) beside fern_sim_topk_deep (exact fp32
form, the same K) -- the stage it is built on, whose code path this feature leaves as it was -- measured in the same process on the same
box.  The item stage adds two reads and one write of the [B, N] score rows and a pass over the [B, G] table to the deep stage.

Stage time = libfern's own instrumentation (fern_prof_enable / fern_prof_collect: the stage interval and, inside it, the score kernel by
its dispatch timestamps), one run of 5 warm-up and 20 timed calls per measurement.  Items are contiguous runs of four rows.  Every list is
checked against the de-duplicated K' = 1024 row list where that list is long enough, and item_rank_of against the list.

    python tools/rank_items_bench.py [--reps 20] [--warmup 5] [--only c2,200k] [--out profiles/rank_items_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fashionern_aaai2024_amd.engine import FernEngine, ItemMap  # noqa: E402

SHAPES = [("c2", 64, 46_000, 512, 50, 11_500), ("200k", 64, 200_000, 640, 50, 50_000)]


def timed(eng, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    eng.prof_enable(True)
    for _ in range(reps):
        fn()
    st = eng.prof_collect()
    eng.prof_enable(False)
    return {"stage_us": round((st["sweep_ms"] + st["topk_ms"]) / reps * 1e3, 1), "sweep_us": round(st["sweep_ms"] / reps * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    eng = FernEngine("cuda:0")
    dev = eng.device
    lines, bad = [], []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# rank_items_bench: {torch.cuda.get_device_name(0)}, {args.warmup} warm-up + {args.reps} timed calls, stage (score kernel) time in us")
    say("# shape                 K       G   sim_topk_items stage (scores)   sim_topk_deep stage (scores)   ratio   item_rank_of m=1 stage")
    for name, b, n, d, k, g_items in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        g = torch.Generator(device=dev).manual_seed(n + d)
        gal = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device=dev), dim=-1)
        q = torch.nn.functional.normalize(torch.randn(b, d, generator=g, device=dev), dim=-1)
        items = ItemMap((torch.arange(n, device=dev, dtype=torch.int64) * g_items // n).to(torch.int32), g_items)
        s, i, t = eng.sim_topk_items(q, gal, items, k)
        # check: the first k distinct items of the K' = 1024 row list (k items need at most 4 k rows here)
        ds, di = eng.sim_topk_deep(q, gal, 1024)
        dt = items.items[di.long()]
        for r in range(b):
            seen, rows = set(), []
            for idx, it in zip(di[r].tolist(), dt[r].tolist()):
                if it not in seen:
                    seen.add(it)
                    rows.append(idx)
                if len(rows) == k:
                    break
            if rows != i[r].tolist():
                bad.append((name, r, "list != the de-duplicated K' = 1024 row list"))
                break
        ranks = eng.item_rank_of(q, gal, items, t[:, ::7].contiguous())
        if not torch.equal(ranks, torch.arange(0, k, 7, device=dev, dtype=torch.int32).repeat(b, 1)):
            bad.append((name, "item_rank_of != place in the list"))
        it_ = timed(eng, lambda: eng.sim_topk_items(q, gal, items, k), args.warmup, args.reps)
        deep = timed(eng, lambda: eng.sim_topk_deep(q, gal, k), args.warmup, args.reps)
        tgt = t[:, :1].contiguous()
        rk = timed(eng, lambda: eng.item_rank_of(q, gal, items, tgt), args.warmup, args.reps)
        rec = {"shape": name, "B": b, "N": n, "D": d, "K": k, "G": g_items, "sim_topk_items": it_, "sim_topk_deep": deep, "item_rank_of_m1": rk,
               "ratio_vs_deep": round(it_["stage_us"] / deep["stage_us"], 2)}
        say(f"{b:5d}x{n:8d}x{d:4d} {k:5d} {g_items:7d}   {it_['stage_us']:14.1f} ({it_['sweep_us']:8.1f})   {deep['stage_us']:14.1f} ({deep['sweep_us']:8.1f})"
            f"   {rec['ratio_vs_deep']:5.2f}   {rk['stage_us']:14.1f}")
        say("json " + json.dumps(rec))
        del gal, q
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if bad:
        raise SystemExit(f"rank_items mismatches: {bad}")


if __name__ == "__main__":
    main()

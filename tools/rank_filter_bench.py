#!/usr/bin/env python
"""Filtered-ranking micro-benchmark: fern_sim_topk_filtered beside the UNFILTERED entry point of the same gallery form and K, timed in
the same process with the calls alternating (unfiltered, unfiltered again, filtered -- per repetition), so that the yardstick is the
unchanged code path and its own run-to-run spread is on the same line.

  shapes   64 x 46 000 x 512, 64 x 200 000 x 640, 64 x 1 000 000 x 512, 1 024 x 21 552 x 512
  K        50 (prepared: the masked dense form; bf16: the deep stage) and 1 000 (the deep stage)
  forms    prepared (fp32 + bf16 copy + meta) and bf16
  filters  all-pass (mask 0), one category of three (n % 3), one group of six rows

Stage time = libfern's own instrumentation (fern_prof_enable / fern_prof_collect: the stage interval and, inside it, the sweep kernel by
its dispatch timestamps), 5 warm-up and 20 timed calls.  Every filtered result is checked: all-pass against the unfiltered call bit for
bit, the others for eligibility of every listed row and for the number of filled places.

    python tools/rank_filter_bench.py [--reps 20] [--warmup 5] [--only c2,200k] [--out profiles/rank_filter_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fashionern_aaai2024_amd.engine import FernEngine, RowFilter  # noqa: E402

SHAPES = [("c2", 64, 46_000, 512), ("200k", 64, 200_000, 640), ("1M", 64, 1_000_000, 512), ("b1024", 1024, 21_552, 512)]


def one(eng, fn):
    fn()
    st = eng.prof_collect()
    return (st["sweep_ms"] + st["topk_ms"]) * 1e3, st["sweep_ms"] * 1e3


def alternating(eng, fns, warmup, reps):
    """[{stage_us, sweep_us}] per function, the functions called in turn inside every repetition."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    eng.prof_enable(True)
    tot = [[0.0, 0.0] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(tot, fns):
            stage, sweep = one(eng, fn)
            t[0] += stage
            t[1] += sweep
    eng.prof_enable(False)
    return [{"stage_us": round(t[0] / reps, 1), "sweep_us": round(t[1] / reps, 1)} for t in tot]


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

    say(f"# rank_filter_bench: {torch.cuda.get_device_name(0)}, {args.warmup} warm-up + {args.reps} timed calls, alternating; stage (sweep kernel) time in us")
    say("# shape              form      K     filter      unfiltered stage (sweep)   again (spread)   filtered stage (sweep)   ratio")
    for name, b, n, d in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        g = torch.Generator(device=dev).manual_seed(n + d)
        gal = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device=dev), dim=-1)
        q = torch.nn.functional.normalize(torch.randn(b, d, generator=g, device=dev), dim=-1)
        pg = eng.prepare_gallery(gal)
        rows = torch.arange(n, device=dev)
        tags = ((rows % 3) | ((rows // 6) << 2)).to(torch.int32)
        qs = torch.arange(b, device=dev)
        filters = {"all-pass": RowFilter(tags, 0, 0), "category": RowFilter(tags, 3, (qs % 3).to(torch.int32)),
                   "group-of-6": RowFilter(tags, ~3, (((qs * 7919) % (n // 6)) << 2).to(torch.int32))}
        for form, gform in (("prepared", pg), ("bf16", pg.bf16)):
            for k in (50, 1000):
                if k > 64:
                    plain = lambda: eng.sim_topk_deep(q, gform, k)                                  # noqa: E731
                elif form == "bf16":
                    plain = lambda: eng.sim_topk_bf16(q, gform, k)                                  # noqa: E731
                else:
                    plain = lambda: eng.sim_topk(q, gform, k)                                       # noqa: E731
                ref = plain()
                for fname, flt in filters.items():
                    filt = lambda: eng.sim_topk(q, gform, k, row_filter=flt)                        # noqa: E731
                    s, i = filt()
                    _, fm, fv = flt.resolve(b, n, dev)
                    listed = i >= 0
                    ok = ((tags[i.clamp(min=0).long()] & fm[:, None]) == fv[:, None]) | ~listed
                    if not bool(ok.all()):
                        bad.append((name, form, k, fname, "an ineligible row is listed"))
                    if fname == "all-pass" and not (torch.equal(i, ref[1]) and torch.equal(s, ref[0])):
                        bad.append((name, form, k, fname, "differs from the unfiltered call"))
                    if fname == "group-of-6" and not bool((listed.sum(dim=1) == min(k, 6)).all()):
                        bad.append((name, form, k, fname, "a group of six must fill exactly six places"))
                    a, a2, f = alternating(eng, [plain, plain, filt], args.warmup, args.reps)
                    rec = {"shape": name, "B": b, "N": n, "D": d, "form": form, "K": k, "filter": fname, "unfiltered": a, "unfiltered_again": a2,
                           "filtered": f, "spread": round(a2["stage_us"] / a["stage_us"], 3), "ratio": round(f["stage_us"] / a["stage_us"], 3)}
                    say(f"{b:5d}x{n:8d}x{d:4d}  {form:9s} {k:5d}  {fname:11s} {a['stage_us']:10.1f} ({a['sweep_us']:8.1f})   {a2['stage_us']:9.1f} ({rec['spread']:5.3f})"
                        f"   {f['stage_us']:10.1f} ({f['sweep_us']:8.1f})   {rec['ratio']:6.3f}")
                    say("json " + json.dumps(rec))
        del gal, q, pg
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if bad:
        raise SystemExit(f"filtered ranking mismatches: {bad}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Candidate-ranking micro-benchmark: fern_sim_topk_candidates beside the routes to the same answer that exist without it, timed in the
same process with the calls alternating inside every repetition.

  shapes   1 024 x 6 x 640 (CIRR's member sets), 64 x 1 024 x 512 (search within a deep list), 64 x 4 096 x 512; N = 46 000 throughout
  forms    fp32 and bf16-only galleries
  other    B <= 32: sim_topk(row_filter = one tag bit per query); otherwise rank_keys + read-back + a host-side sort of the keys

The candidate call is timed by device events (and by the host clock around a synchronisation, for the same scale as the other route, whose
host part no event sees); a warm-up on every shape, at least 200 timed calls per shape.  Every result is checked against the other route.
The bytes a call must move are B * M * D * s_g (every named row once per query) + B * D * 4 (the queries).  Needs a GPU.

    python tools/rank_candidates_bench.py [--reps 200] [--warmup 10] [--out profiles/rank_candidates_bench.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fashionern_aaai2024_amd.engine import FernEngine, RowFilter  # noqa: E402

N = 46_000
SHAPES = [("cirr", 1024, 6, 640), ("deep-list", 64, 1024, 512), ("longest", 64, 4096, 512)]


def host_sorted(keys, k):
    """The first k distinct keys of every row, descending, as (key bits uint64 [B,k]); 0 = unfilled."""
    a = keys.cpu().numpy().view(np.uint64)
    out = np.zeros((a.shape[0], k), dtype=np.uint64)
    for r in range(a.shape[0]):
        u = np.unique(a[r])[::-1]
        u = u[u != 0][:k]
        out[r, :len(u)] = u
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.reps < 200:
        raise SystemExit("at least 200 timed calls per shape")
    if not torch.cuda.is_available():
        raise SystemExit("rank_candidates_bench needs a GPU")
    from fashionern_aaai2024_amd.engine import ranking_keys
    eng = FernEngine("cuda:0")
    dev = eng.device
    lines, bad = [], []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# rank_candidates_bench: {torch.cuda.get_device_name(0)}, N = {N}, {args.warmup} warm-up + {args.reps} timed calls per shape, alternating")
    say("# shape        B      M     D   form   K     candidates: events us   host-clock us   GB/s (events)     other route: host-clock us   (which)")
    for name, b, m, d in SHAPES:
        g = torch.Generator(device=dev).manual_seed(m + d)
        gal = torch.nn.functional.normalize(torch.randn(N, d, generator=g, device=dev), dim=-1)
        q = torch.nn.functional.normalize(torch.randn(b, d, generator=g, device=dev), dim=-1)
        cand = torch.randint(0, N, (b, m), generator=g, device=dev, dtype=torch.int32)
        k = min(m, 1024)
        for form, gform, sg in (("fp32", gal, 4), ("bf16", eng.gallery_to_bf16(gal), 2)):
            ours = lambda: eng.sim_topk_candidates(q, gform, cand, k)                                   # noqa: E731
            if b <= 32:
                which = "sim_topk(row_filter)"
                tags = torch.zeros(N, dtype=torch.int32, device=dev)
                for r in range(b):
                    tags[cand[r].long()] |= (1 << r) if r < 31 else -(1 << 31)
                bit = torch.tensor([1 << r for r in range(b)], dtype=torch.int64)
                flt = RowFilter(tags, bit, bit)
                other = lambda: ranking_keys(*eng.sim_topk(q, gform, k, row_filter=flt)).cpu().numpy().view(np.uint64)      # noqa: E731
            else:
                which = "rank_keys + host sort"
                other = lambda: host_sorted(eng.rank_keys(q, gform, cand), k)                           # noqa: E731
            got = ranking_keys(*ours()).cpu().numpy().view(np.uint64)
            if not np.array_equal(got, other()):
                bad.append((name, form))
            for _ in range(args.warmup):
                ours()
                other()
            torch.cuda.synchronize()
            ev_us = wall_us = other_us = 0.0
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                ours()
                e1.record()
                torch.cuda.synchronize()
                wall_us += (time.perf_counter() - t0) * 1e6
                ev_us += e0.elapsed_time(e1) * 1e3
                t0 = time.perf_counter()
                other()
                torch.cuda.synchronize()
                other_us += (time.perf_counter() - t0) * 1e6
            ev_us, wall_us, other_us = ev_us / args.reps, wall_us / args.reps, other_us / args.reps
            nbytes = b * m * d * sg + b * d * 4
            rec = {"shape": name, "B": b, "M": m, "D": d, "N": N, "form": form, "K": k, "bytes": nbytes, "candidates_event_us": round(ev_us, 1),
                   "candidates_host_us": round(wall_us, 1), "gbps": round(nbytes / ev_us / 1e3, 1), "other": which, "other_host_us": round(other_us, 1)}
            say(f"{name:10s} {b:5d}  {m:5d}  {d:4d}   {form:5s} {k:5d}   {ev_us:12.1f}   {wall_us:12.1f}   {rec['gbps']:10.1f}   {other_us:18.1f}   ({which})")
            say("json " + json.dumps(rec))
        del gal, q
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if bad:
        raise SystemExit(f"candidate ranking differs from the other route: {bad}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Live-gallery micro-benchmark: what changing m rows of a prepared 1M x 512 store costs in place (fern_gallery_upsert, fern_gallery_move)
beside what the same change cost before -- fern_gallery_prepare over the whole store -- in the same process on the same box.

Call time = device events around `reps` back-to-back calls on one stream, divided by reps, after `warmup` calls of the same shape; every
call of a measurement gets its own random slots (and source rows), so no call finds its rows in a cache the previous one filled.  Bytes are
the algorithm's: an upsert reads m * D * 4 and writes m * D * 6, a move reads and writes m * D * 6, prepare reads N * D * 4 and writes
N * D * 2; the fraction is of the 8 TB/s HBM peak.  A time that does not move with m is the launch, not the bytes.  The store's bf16 copy
is checked against a fresh prepare of its fp32 rows after all updates.

    python tools/live_gallery_bench.py [--rows 1000000] [--dim 512] [--reps 50] [--warmup 5] [--out profiles/live_gallery_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fashionern_aaai2024_amd.engine import FernEngine  # noqa: E402

HBM_PEAK = 8.0e12
MS = (64, 1024, 8192)


def timed(fns, warmup):
    """us per call: `warmup` untimed calls, then every fn of `fns` once between two events."""
    for fn in fns[:warmup]:
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for fn in fns[warmup:]:
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (len(fns) - warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    eng = FernEngine("cuda:0")
    dev = eng.device
    n, d = args.rows, args.dim
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    gen = torch.Generator(device=dev).manual_seed(n + d)
    store = torch.nn.functional.normalize(torch.randn(n, d, generator=gen, device=dev), dim=-1)
    pg = eng.prepare_gallery(store)
    f32, b16, meta = pg.f32, pg.bf16, pg.meta
    say(f"# live_gallery_bench: {torch.cuda.get_device_name(0)}, prepared store {n} x {d}, {args.warmup} warm-up + {args.reps} timed calls, "
        f"device events, us per call")
    say("# entry                       m        us     bytes   GB/s   of 8 TB/s")
    calls = args.warmup + args.reps

    def report(name, m, us, nbytes):
        rate = nbytes / (us * 1e-6)
        rec = {"entry": name, "m": m, "us": round(us, 1), "bytes": nbytes, "GBps": round(rate / 1e9, 1), "of_hbm_peak": round(rate / HBM_PEAK, 4)}
        say(f"{name:24s} {m:8d} {us:9.1f} {nbytes:9.2e} {rate / 1e9:6.0f}   {rate / HBM_PEAK:8.4f}")
        say("json " + json.dumps(rec))
        return rec

    recs = []
    for m in MS:
        rows = torch.nn.functional.normalize(torch.randn(calls, m, d, generator=gen, device=dev), dim=-1)
        slots = torch.stack([torch.randperm(n, generator=gen, device=dev)[:m] for _ in range(calls)]).to(torch.int32)
        us = timed([lambda i=i: eng.gallery_upsert(rows[i], slots[i], f32, b16, meta) for i in range(calls)], args.warmup)
        recs.append(report("fern_gallery_upsert", m, us, m * d * 10))
    for m in MS:
        half = n // 2
        src = torch.stack([half + torch.randperm(n - half, generator=gen, device=dev)[:m] for _ in range(calls)]).to(torch.int32)
        dst = torch.stack([torch.randperm(half, generator=gen, device=dev)[:m] for _ in range(calls)]).to(torch.int32)
        us = timed([lambda i=i: eng.gallery_move(src[i], dst[i], f32, b16) for i in range(calls)], args.warmup)
        recs.append(report("fern_gallery_move", m, us, m * d * 12))
    fresh_b16 = torch.empty_like(b16)
    fresh_meta = torch.zeros(4, device=dev)
    from fashionern_aaai2024_amd.engine import PreparedGallery
    out = PreparedGallery(f32, fresh_b16, fresh_meta)
    reps = max(3, args.reps // 10)
    us = timed([lambda: eng.prepare_gallery(f32, out=out)] * (2 + reps), 2)
    whole = report("fern_gallery_prepare", n, us, n * d * 6)
    eng.sync()
    ok = torch.equal(b16.view(torch.int16), fresh_b16.view(torch.int16)) and bool((fresh_meta <= meta).all())
    say(f"# store check (bf16 copy == prepare of the fp32 rows, meta an upper bound of prepare's): {'ok' if ok else 'MISMATCH'}")
    for r in recs:
        if r["entry"] == "fern_gallery_upsert":
            say(f"# upsert m = {r['m']}: {whole['us'] / r['us']:.0f}x less time than the whole-store prepare it replaces")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("live_gallery_bench: the store's bf16 copy or meta is not what prepare gives")


if __name__ == "__main__":
    main()

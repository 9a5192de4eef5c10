#!/usr/bin/env python
"""Headline benchmark: composed queries/sec of the encode -> fuse -> rank path (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2|c3|c4|c5] [--dump-outputs DIR] [--full]

One STEP on one GPU = one batch of composed queries, inputs already resident in HBM:
    encode_image(B x 3xSxS) -> encode_text(B x 77 tokens, one tower pass)
    -> ERN mode="test" fusion (2-layer BERT over 91 tokens, cross-attention, SR pooling, 3 Combiners)
    -> cosine top-K against the fused gallery (fused sweep + selection: the [B, N] score matrix is never stored).
Workloads (BASELINE.json configs; synthetic data, random-init weights of the real architecture):
    c2  (default, the headline)  FashionIQ ViT-B/16, fp32, 64 queries per GPU vs a 46k-row gallery            configs[1]
    c3  Fashion200k RN50x4 (D = 640, 288 px), fp32, 64 queries per GPU vs a 200k-row gallery                  configs[2]
    c4  CIRR ViT-B/16, fp32, 128 queries per GPU (1024 on 8), K = 51 with the reference removed + subset      configs[3]
    c5  FashionIQ ViT-B/16, fp8 encoder GEMMs + bf16 similarity, 64 queries per GPU vs a 1M-row bf16 gallery  configs[4]

N GPUs = N ranks, one process per GPU (torch.distributed, backend nccl = RCCL over xGMI).  `python bench.py --gpus N` launches
them itself -- N fresh children through torch.distributed.run, BEFORE this process touches the GPU -- and also runs as a
rank when started under torchrun (RANK / WORLD_SIZE present).  The gallery is built sharded: every rank synthesises and
fuses ONLY its own rows (seed + rank), then one all_gather replicates the fused rows; queries are data parallel (weak scaling:
value = N x B x K / max-over-ranks time), with no data-path collective.  c5 also reports the gallery-sharded variant
(all-gather queries, local top-K with idx_offset, all-gather candidates, merge).

A plain run sets up, warms up, times the K steps and prints the headline line (`--dump-outputs DIR`: and writes what the last
timed step returned).  With `--full`, after the timed region the same step runs with libfern's HIP-event instrumentation (events
on the launch stream around every GEMM / attention / sweep launch) to fill `roofline`; on rank 0 at N = 1 the CPU oracle is timed
on bounded samples for `cpu_baseline` and used as the checker of the GPU result; the secondary legs and the c3 / c4 / c5 child
runs follow.
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# One hardware queue per lane (round 6): the ROCm runtime maps a process's HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4)
# and two streams that share one run back to back.  With 8 queues FOUR batches in flight beat three -- c2 3 030 -> 3 080 queries/s, c3
# +1.7 %, c4 +0.7 %, c5 18.5 -> 19.0 k -- where with the default 4 queues a fourth lane LOSES (c5 16.8 k: it shares a queue; `profiles/
# r06_lanes_hwq.txt`).  Must be in the environment before the first HIP call (torch is imported later, in main()); a value the user
# exported wins.  Child processes (other configs, --gpus N ranks) inherit it.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
_T0 = time.perf_counter()
_STAMPS = {}


def stamp(name):
    """Wall-clock seconds since the process started, per phase of the run (`timing_s` of the record: where a default run's minute goes)."""
    _STAMPS[name] = round(time.perf_counter() - _T0, 1)


def csrc_sha16() -> str:
    """sha256 over the kernel sources: the PMC traffic file is stamped with it (tools/pmc_traffic.py) and `roofline.traffic` is reported
    only when the stamp equals THIS tree's -- a counter figure measured on other kernels is omitted, not labelled stale (VERDICT r5 item 8;
    there is no .git on the GPU box to compare heads with)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "fashionern_aaai2024_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            with open(os.path.join(d, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]

def mixed_peak(st) -> float:
    """Peak of the block-scaled GEMM family's launches when some of their flops are bf16 flops (FERN_PREC_MX8_IMG under fern_encode_pair:
    the text tower's bf16 GEMM of a layer rides in the image tower's block-scaled launch -- fern_prof_stats.gemm_mx8_bf16_flops): each
    part priced against its own dense peak, i.e. total flops / (fp8 flops / 5 PFLOP/s + bf16 flops / 2.5 PFLOP/s).  Equals the fp8 peak
    when no launch is paired."""
    total, b16 = st["gemm_mx8_flops"], st.get("gemm_mx8_bf16_flops", 0.0)
    if total <= 0:
        return MX8_MFMA_PEAK_TFLOPS
    return total / ((total - b16) / MX8_MFMA_PEAK_TFLOPS + b16 / BF16_MFMA_PEAK_TFLOPS)


F32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
F32X3_BOUND_TFLOPS = 157.3 * 128.0 / 48.0      # f32x3: six 32-cycle bf16 MFMAs (192 cycles) do the work of two 64-cycle fp32 MFMAs -> 419.5 fp32-equivalent TFLOP/s
MX8_MFMA_PEAK_TFLOPS = 5000.0     # MI355X_MICROARCH.md: dense fp8 on the block-scaled MFMA (v_mfma_scale_f32_32x32x64_f8f6f4), 2x the bf16 rate
BF16_MFMA_PEAK_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 MFMA (the non-scaled fp8 32x32x16 MFMA issues at this rate too)
HBM_PEAK_GBS = 8000.0             # MI355X_MICROARCH.md: HBM3E spec (6.29 TB/s measured copy)
XGMI_PEAK_GBS = 7 * 153.0         # 7 point-to-point links x ~153 GB/s per GPU

WORKLOADS = {
    "c2": dict(clip="ViT-B-16", d=512, batch=64, gallery=46_000, k=50, precision="fp32", cirr=False, bf16_gallery=False,
               text="FashionIQ ViT-B/16 composed queries: 64-query batch per GPU vs 46k-image fused gallery (BASELINE.json configs[1])"),
    "c3": dict(clip="RN50x4", d=640, batch=64, gallery=200_000, k=50, precision="fp32", cirr=False, bf16_gallery=False,
               text="Fashion200k RN50x4 (D=640, 288 px) composed queries: 64-query batch per GPU vs ~200k-image gallery built sharded "
                    "+ RCCL all-gather (BASELINE.json configs[2])"),
    "c4": dict(clip="ViT-B-16", d=512, batch=128, gallery=21_552, k=51, precision="fp32", cirr=True, bf16_gallery=False,
               text="CIRR ViT-B/16 composed queries: 128-query batch per GPU (1024 on 8 GPUs), global top-51 with the reference removed "
                    "+ subset scores of 6 members (BASELINE.json configs[3])"),
    # c5's encoder mode (round 6): the FASTEST mode whose Recall@50 stays within 1 pp of the fp32 encoder's and whose
    # top-50 overlap is >= 0.94 on the 2 048-query `reduced_modes` table -- "mx8img" (FERN_PREC_MX8_IMG: 0.0 pp, 0.942); rounds 2-5 timed
    # "mx8" (-2.7 pp, 0.893: still reported beside it, `--precision mx8`)
    "c5": dict(clip="ViT-B-16", d=512, batch=64, gallery=1_000_000, k=50, precision="mx8img", cirr=False, bf16_gallery=True,
               text="FashionIQ ViT-B/16 fp8 MFMA encoder GEMMs + bf16 similarity: 64-query batch per GPU vs 1M-row bf16 gallery "
                    "(BASELINE.json configs[4])"),
}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)       # warm-up 10, >= 50 timed steps
    ap.add_argument("--config", choices=sorted(WORKLOADS), default="c2")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample", type=int, default=16)
    ap.add_argument("--gallery", type=int, default=None, help="override the workload's gallery rows")
    ap.add_argument("--lanes", type=int, default=4, help="query batches kept in flight on separate HIP streams (one hardware queue each: GPU_MAX_HW_QUEUES, "
                                                         "set to 8 above unless exported)")
    ap.add_argument("--graphs", action="store_true", help="replay each lane's step from a hipGraph (captured after two eager calls)")
    ap.add_argument("--precision", choices=["fp32", "f32x3", "bf16", "fp8", "mx8", "mx8mlp", "mx8img"], default=None,
                    help="override the encoder operand precision of the TIMED path (fp32 = parity mode, the c2 headline)")
    ap.add_argument("--headline-only", action="store_true",
                    help="--full: skip the secondary legs (reduced-precision modes, lookup variant, 1M-row bf16 sweep, encode rate): the GEMM "
                         "dispatches of the run are then the headline step's, for comparing rocprofv3 averages with `roofline`")
    ap.add_argument("--pmc-mode", action="store_true",
                    help="for `rocprofv3 --pmc`: warm up, emit a marker dispatch, run exactly --steps steps on one stream, exit (no JSON)")
    ap.add_argument("--save-tiles", type=str, default=None, help="write the GEMM tuner's choices to this file (FERN_GEMM_TILES format)")
    ap.add_argument("--rank-plain", action="store_true",
                    help="rank the fp32 gallery with the fp32-MFMA sweep (fern_sim_topk) instead of its prepared form (certified bf16 pre-filter + "
                         "exact fp32 rescoring, fern_sim_topk_prefiltered): same results, the round-4 stage")
    ap.add_argument("--cpu-all-cores", action="store_true",
                    help="cpu_baseline: also time ONE query with torch's pool on every schedulable core (256 threads on the GPU box: ~70 s, a "
                         "documented pathology of the pool -- not part of the default run since round 6)")
    ap.add_argument("--full-record", type=str, default=os.path.join(ROOT, "bench_full.json"),
                    help="--full: where rank 0 writes the FULL record (every leg, notes, tile table); stdout carries the compact line (< 4 KB)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="--full c2 run at N = 1: do not also run the c3 / c4 / c5 workloads (short child runs of this script, reported "
                         "under `other_configs`)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run everything else the benchmark measures and checks: roofline passes, the "
                         "gallery-build and all-gather figures, the reduced-precision and quality legs, the CPU baseline with its parity "
                         "check, the c3 / c4 / c5 child runs, the full record.  Without it a run sets up, warms up, times the steps and "
                         "prints the headline line")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="rank 0 writes what the timed path returned in its last step to DIR/<name>.npy (float32 / float64): the "
                         "top-K scores and indices, the fused query features and, for c4, the member scores")
    return ap.parse_args()


def spawn_ranks(args) -> None:
    """`python bench.py --gpus N` outside torchrun: start N rank processes and mirror rank 0's JSON line.  Nothing in THIS process
    has touched the GPU (torch is not even imported yet), so starting children is safe; the children are fresh interpreters."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: required for RCCL across processes on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def other_config_lines(steps: int) -> dict:
    """The BASELINE.json workloads other than the headline, measured on the same box by short child runs of this script (a child
    process, started after this one is done with its timed region; never an exec): one compact record per config so that the
    driver's single default run carries a c3 / c4 / c5 number too.  `value` of the main line is untouched."""
    import tempfile
    out = {}
    keep = ("value", "unit", "ms_per_step", "dtype", "encoder_precision", "accuracy_vs_fp32_encoder", "reduced_modes")
    for name in ("c3", "c4", "c5"):
        t0 = time.perf_counter()
        fd_, full_path = tempfile.mkstemp(prefix=f"fern_bench_{name}_", suffix=".json")
        os.close(fd_)
        cmd = [sys.executable, os.path.abspath(__file__), "--config", name, "--steps", str(steps), "--warmup", "4", "--full", "--no-cpu-baseline",
               "--no-other-configs", "--full-record", full_path]
        if name != "c5":
            cmd.append("--headline-only")      # c5 keeps its secondary leg: the ranking agreement of the fp8 encoder with the fp32 one
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
            if r.returncode != 0:
                raise RuntimeError(f"rc {r.returncode}: {r.stderr[-200:]}")
            with open(full_path) as f:
                j = json.load(f)
            rec = {k: j.get(k) for k in keep}
            rec["workload"] = j["config"]["workload"]
            rec["roofline"] = {k: j["roofline"].get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "kernel", "gemm_ms_per_step", "step_level")}
            rec["roofline"]["regime"] = "serial_passes (instrumented one-stream passes; `step_level` = same flops / the timed multi-lane ms_per_step)"
            rec["latency_ms_per_batch"] = j.get("latency_ms_per_batch")
            if j.get("roofline_sim_sweep"):
                rec["rank_stage_us"] = j["roofline_sim_sweep"].get("stage_us")
                rec["rank_stage_frac_of_hbm"] = j["roofline_sim_sweep"].get("frac")
            rec["wall_s"] = time.perf_counter() - t0
            out[name] = rec
        except Exception as e:      # a failed side run must not take the headline line down with it
            out[name] = {"error": f"{type(e).__name__}: {e}"[:300]}
        finally:
            try:
                os.unlink(full_path)
            except OSError:
                pass
    return out


def multi_gpu_preflight(torch, dist, fd, rank, world, local, device, backend, measure=True):
    """`--gpus N`, N > 1: before any model work, every rank reports where it runs and the job times the path's one collective
    shape on the wire -- so that the first run on a real multi-GPU node is self-diagnosing: RCCL world size,
    per-rank device (index, name, PCI bus id), two ranks on one device (refused unless the FERN_BENCH_SHARE_GPU debug layout), and
    (`measure`, i.e. --full) the all-gather rate of 64 MiB-per-rank bf16 blocks (the C5 shard is 128 MB) against 7 x 153 GB/s of xGMI.
    Printed to stderr by rank 0 and carried in the full record under `preflight`."""
    props = torch.cuda.get_device_properties(device)
    me = {"rank": rank, "local_rank": local, "device": device.index, "name": props.name, "host": socket.gethostname(),
          "pci_bus_id": getattr(props, "pci_bus_id", None), "hsa_ipc_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}
    everyone = [None] * world
    dist.all_gather_object(everyone, me)
    seen = {}
    for e in everyone:
        key = (e["host"], e["device"])
        if key in seen and not os.environ.get("FERN_BENCH_SHARE_GPU"):
            raise SystemExit(f"bench preflight: ranks {seen[key]} and {e['rank']} both run on {key}: one process per GPU is the layout "
                             "(LOCAL_RANK -> cuda:LOCAL_RANK); set FERN_BENCH_SHARE_GPU=1 only for the one-GPU debug rehearsal")
        seen[key] = e["rank"]
    if not measure:      # a run without --full: the layout check only
        return {"rccl_world": world if backend == "nccl" else f"{world} (debug backend {backend})", "backend": backend, "ranks": everyone}
    per = 64 << 20
    block = torch.full((per // 2,), float(rank), dtype=torch.bfloat16, device=device)
    out = torch.empty((world * (per // 2),), dtype=torch.bfloat16, device=device)
    fd._all_gather_into(out, block)                      # connection set-up, workspaces
    torch.cuda.synchronize()
    dist.barrier()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 3
    ev0.record()
    for _ in range(reps):
        fd._all_gather_into(out, block)
    ev1.record()
    torch.cuda.synchronize()
    ms = ev0.elapsed_time(ev1) / reps
    ok_here = bool((out.view(world, -1)[:, 0].float().cpu() == torch.arange(world, dtype=torch.float32)).all())
    t = torch.tensor([ms], dtype=torch.float64, device=device)
    if backend == "gloo":
        th = t.cpu()
        dist.all_reduce(th, op=dist.ReduceOp.MAX)
        ms = th.item()
    else:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ms = t.item()
    # every rank learns of a bad payload on ANY rank and they all leave together -- a rank that exits alone leaves the others
    # hanging in the gallery build's collectives until the process-group timeout
    oks = [None] * world
    dist.all_gather_object(oks, ok_here)
    ok = all(oks)
    recv = (world - 1) * per
    info = {"rccl_world": world if backend == "nccl" else f"{world} (debug backend {backend})", "backend": backend, "ranks": everyone,
            "all_gather_64MiB_per_rank": {"ms": ms, "bytes_received_per_rank": recv, "GBs_per_rank": recv / (ms * 1e-3) / 1e9,
                                          "frac_of_xgmi": recv / (ms * 1e-3) / 1e9 / XGMI_PEAK_GBS, "payload_ok": ok}}
    if rank == 0:
        print("[bench preflight] " + json.dumps(info), file=sys.stderr, flush=True)
    if not ok:
        raise SystemExit("bench preflight: the all-gather returned the wrong blocks on rank(s) " + str([r for r, o in enumerate(oks) if not o]))
    return info


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def _host_cpu():
    """(model name, logical cores) of the host this rank runs on -- north_star: "core count stated"."""
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return model, os.cpu_count()


def _cpu_threads():
    # threads actually used: the host cores this process may run on, capped at 32 (torch's intra-op pool stops scaling on these
    # small per-query matrices well before that; an uncapped 256-thread pool is ~100x slower)
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    return max(1, min(avail, 32))


def order_parity(o_scores_full, g_idx, o_idx):
    """How the GPU ranking relates to the oracle's: identical rows / positions, and -- at every position where they differ -- the
    gap between the ORACLE's own scores of the two rows (a near-tie of the oracle if tiny)."""
    import torch
    same_rows = int((g_idx == o_idx).all(dim=1).sum().item())
    gap = 0.0
    for r, p in (g_idx != o_idx).nonzero().tolist():
        gap = max(gap, abs(o_scores_full[r, g_idx[r, p]].item() - o_scores_full[r, o_idx[r, p]].item()))
    return {"rows_with_identical_order": same_rows, "positions_equal_frac": float((g_idx == o_idx).float().mean().item()),
            "max_oracle_score_gap_at_mismatching_positions": gap}


def cpu_baseline(clip_sd, fusion_sd, cfg, w, images, tokens, loc, gallery, sample, gpu_topk, repeats=3, extra_topk=None, all_cores_leg=False):
    """The CPU oracle (kind "port": this repo's restatement, pinned against the imported reference by tests/golden) timed on the
    host cores, on bounded samples of the same workload; it is also the checker of the HIP result (parity_vs_hip).
      * end to end: `sample` composed queries -- encode image + text, fuse, rank against the same fused gallery;
      * C2 fuse + rank at full size (B = 64, N = gallery rows), C1 plumbing sizes (D = 640, N = 1000, B = 32): BASELINE.md 3."""
    import torch
    from fashionern_aaai2024_amd import synth
    from oracle import clip as oclip, fusion as ofusion, rank as orank
    threads = _cpu_threads()
    torch.set_num_threads(threads)
    k, d = w["k"], w["d"]
    csd, fsd = ofusion.as_torch(clip_sd), ofusion.as_torch(fusion_sd)
    im, tk, lc, gal = images[:sample].cpu(), tokens[:sample].cpu(), loc[:sample].cpu(), gallery.float().cpu()

    def one():
        with torch.no_grad():
            rf = oclip.encode_image(csd, cfg, im)
            tg, ts = oclip.encode_text(csd, cfg, tk)
            q = ofusion.dvr_fuse(fsd, lc, ts, rf, tg)
            return q, orank.cosine_topk(q, gal, k)

    warm = _timed(one)
    best = min([warm] + [_timed(one) for _ in range(repeats)]) if warm < 20 else warm      # keep the run bounded
    oq, (o_s, o_i) = one()
    g_s, g_i = gpu_topk[0][:sample].cpu(), gpu_topk[1][:sample].cpu()
    parity = order_parity(oq @ gal.T, g_i.long(), o_i.long())
    parity.update({"queries": sample, "max_abs_cosine_diff": float((g_s - o_s).abs().max().item())})
    # the same check for other arithmetic modes of the HIP path on the same queries (f32x3: fp32 data, bf16x3 GEMM arithmetic) --
    # north_star's bar is identical ordering and cosine scores within 1e-3 of the CPU path
    parity_modes = {}
    for name, (x_s, x_i) in (extra_topk or {}).items():
        pm = order_parity(oq @ gal.T, x_i[:sample].cpu().long(), o_i.long())
        pm.update({"queries": sample, "max_abs_cosine_diff": float((x_s[:sample].cpu() - o_s).abs().max().item())})
        parity_modes[name] = pm

    def stage_rates(dd, n, b, tag):
        """fuse + rank plumbing on CPU at (D, N, B): mode="index" over the gallery, mode="test" on B queries, cosine top-K."""
        sd = fsd if dd == d else ofusion.as_torch(synth.fusion_state_dict(dd, seed=0))
        raw, lcl = torch.from_numpy(synth.global_feats(n, dd, 7, tag)), torch.from_numpy(synth.local_feats(n, dd, 7, tag + "-l"))
        rg, rl = torch.from_numpy(synth.global_feats(b, dd, 8, tag + "q")), torch.from_numpy(synth.local_feats(b, dd, 8, tag + "ql"))
        tg, ts = torch.from_numpy(synth.global_feats(b, dd, 9, tag + "t")), torch.from_numpy(synth._normal(9, tag + "ts", (b, 77, dd)))
        with torch.no_grad():
            t_index = _timed(lambda: ofusion.index_fuse(sd, torch.nn.functional.normalize(raw, dim=-1), lcl))
            fused = ofusion.index_fuse(sd, torch.nn.functional.normalize(raw, dim=-1), lcl)
            ofusion.dvr_fuse(sd, rl, ts, rg, tg)
            t_test = min(_timed(lambda: ofusion.dvr_fuse(sd, rl, ts, rg, tg)) for _ in range(2))
            qq = ofusion.dvr_fuse(sd, rl, ts, rg, tg)
            t_rank = min(_timed(lambda: orank.cosine_topk(qq, fused, k)) for _ in range(2))
        return {"feature_dim": dd, "gallery_rows": n, "query_batch": b, "index_fuse_rows_per_s": n / t_index, "dvr_fuse_queries_per_s": b / t_test,
                "rank_ms": t_rank * 1e3, "fuse_plus_rank_queries_per_s": b / (t_test + t_rank)}

    cpu_model, host_cores = _host_cpu()
    # --cpu-all-cores only: the same path with torch's intra-op pool on EVERY schedulable core (BASELINE.md 3 planned os.cpu_count()): on
    # a 256-logical-core host the pool's fork / join per small op dominates and the rate collapses (0.015 queries/s measured in round 5,
    # 67 s of the default run), which is why `value` is quoted at 32 threads and why this leg is no longer part of the default command
    all_cores = None
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    if all_cores_leg and avail > threads:
        torch.set_num_threads(avail)
        ns = 1                                                # ~20 s at the 0.05 queries/s this pool size reaches: one query, one run
        im4, tk4, lc4 = im[:ns], tk[:ns], lc[:ns]

        def small():
            with torch.no_grad():
                rf = oclip.encode_image(csd, cfg, im4)
                tg, ts = oclip.encode_text(csd, cfg, tk4)
                return orank.cosine_topk(ofusion.dvr_fuse(fsd, lc4, ts, rf, tg), gal, k)

        t_run = _timed(small)
        if t_run < 5:                                         # a host where the big pool is not pathological: time a second, warm run
            t_run = _timed(small)
        all_cores = {"value": ns / t_run, "unit": "composed queries/sec", "threads": avail, "sample": f"{ns} composed query, one timed run"}
        torch.set_num_threads(threads)
    return {"value": sample / best, "unit": "composed queries/sec", "cores": threads, "threads": threads, "host_cores": host_cores,
            "all_schedulable_cores": all_cores,
            "cpu_model": cpu_model, "kind": "port",
            "cores_note": "`cores` = torch intra-op threads actually used = min(schedulable cores, 32); `host_cores` = os.cpu_count() of the box",
            "sample": f"{sample} composed queries ({cfg.name} image + text encode, fusion, top-{k} of {gal.shape[0]} rows), "
                      f"torch CPU fp32, best of {repeats + 1}",
            "parity_vs_hip": parity,
            "parity_vs_hip_modes": parity_modes,
            "c2_fuse_rank_full_size": stage_rates(d, min(gal.shape[0], 46_000), 64, "cpu-c2") if d == 512 else None,
            "c1_plumbing": stage_rates(640, 1000, 32, "cpu-c1")}


class _BenchIndexDataset:
    """Index dataset in the reference's tuple format (dataloader/fashioniq.py:82-100, mode="classic": name, image, 13 local features);
    images come from a small pool (a 46k-image fp32 pool would be 27 GB of host memory)."""

    def __init__(self, n, images, local):
        self.n, self.images, self.local = n, images, local

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return f"img{i:06d}", self.images[i % len(self.images)], self.local[i % len(self.local)]


class _BenchRelativeDataset:
    """Relative (query) dataset in the reference's tuple format (fashioniq.py:69-81, mode="relative", split="val"): reference
    name, target name, the two relative captions, the reference image's 13 local features."""

    def __init__(self, q, n_gallery, local, seed=5):
        import numpy as np
        r = np.random.default_rng(seed)
        self.ref = r.integers(0, n_gallery, size=q)
        self.tgt = r.integers(0, n_gallery, size=q)
        words = ("red", "blue", "longer", "shorter", "sleeves", "striped", "floral", "darker", "brighter", "collar", "with", "is",
                 "more", "less", "formal", "casual", "pattern", "plain", "v-neck", "buttons")
        self.caps = [[" ".join(r.choice(words, size=int(r.integers(3, 8)))) + ".", " ".join(r.choice(words, size=int(r.integers(3, 8))))]
                     for _ in range(q)]
        self.local = local

    def __len__(self):
        return len(self.ref)

    def __getitem__(self, i):
        return f"img{int(self.ref[i]):06d}", f"img{int(self.tgt[i]):06d}", self.caps[i], self.local[i % len(self.local)]


def retrieval_quality_leg(torch, eng, cfg, D, device, modes, n_gallery=8192, queries=2048, k=64):
    """what a reduced-precision encoder costs in the metric BASELINE names -- Recall@10 / Recall@50 -- on a synthetic
    FashionIQ-shaped split: `n_gallery` images ENCODED under each mode (the raw index features a query's reference is looked up in,
    run/test/test_fiq.py:104-107, and the mode="index" gallery both come from that mode's image tower), `queries` composed queries
    (reference = a gallery row, 77-token caption) through that mode's text tower and fusion, exact ranking.  A query's TARGET is the row
    its fp32 ranking holds at a position drawn uniformly from 0..63 (so the fp32 recalls are ~15.6 % / ~78 %: targets sit at the ranks
    where Recall@10 / @50 are decided, not at rank 0).  Random-init weights on random inputs are the hard case for rank agreement --
    the top scores of a query lie ~1e-3 apart -- real checkpoints separate their neighbours better."""
    import numpy as np
    g = torch.Generator(device=device).manual_seed(2024)
    local = torch.randn((n_gallery, 13, D), generator=g, device=device)
    ref = torch.randint(0, n_gallery, (queries,), generator=g, device=device)
    toks = torch.randint(1, cfg.vocab_size - 2, (queries, cfg.context_length), generator=g, device=device)
    toks[:, 0] = cfg.vocab_size - 2
    toks[:, -1] = cfg.vocab_size - 1
    pos = torch.randint(0, k, (queries,), generator=g, device=device)
    prev = eng.precision
    out, ranked = {}, {}
    for mode in modes:
        eng.set_precision(mode)
        gi = torch.Generator(device=device).manual_seed(99)          # the SAME images for every mode
        raw = torch.empty((n_gallery, D), device=device)
        for o in range(0, n_gallery, 64):
            raw[o:o + 64] = eng.encode_image(torch.randn((64, 3, cfg.image_size, cfg.image_size), generator=gi, device=device))
        gallery = eng.index_fuse(raw, local, normalize_input=True)
        idx = torch.empty((queries, k), dtype=torch.int32, device=device)
        for o in range(0, queries, 64):
            tg, ts = eng.encode_text(toks[o:o + 64])
            r = ref[o:o + 64]
            q = eng.dvr_fuse(raw[r], local[r], tg, ts)
            idx[o:o + 64] = eng.sim_topk(q, gallery, k)[1]
        ranked[mode] = idx.cpu()
    eng.set_precision(prev)
    base = ranked[modes[0]]
    target = base[torch.arange(queries), pos.cpu()]

    def recalls(idx):
        hit = idx == target[:, None]
        return float(hit[:, :10].any(1).float().mean() * 100), float(hit[:, :50].any(1).float().mean() * 100)

    r10_0, r50_0 = recalls(base)
    hit50_0 = (base == target[:, None])[:, :50].any(1)
    for mode in modes:
        idx = ranked[mode]
        r10, r50 = recalls(idx)
        ov = np.mean([len(set(a.tolist()) & set(b.tolist())) / 50.0 for a, b in zip(base[:, :50], idx[:, :50])])
        hit50 = (idx == target[:, None])[:, :50].any(1)
        n_in, n_out = int((hit50 & ~hit50_0).sum()), int((~hit50 & hit50_0).sum())      # queries whose target entered / left the top-50
        out[mode] = {"recall_at_10": r10, "recall_at_50": r50, "delta_recall_at_10_pp": r10 - r10_0, "delta_recall_at_50_pp": r50 - r50_0,
                     "recall_at_50_flips_in_out": [n_in, n_out], "delta_recall_at_50_se_pp": float(np.sqrt(n_in + n_out) / queries * 100),
                     "top1_same": float((idx[:, 0] == base[:, 0]).float().mean()), "top50_overlap": float(ov)}
    return {"queries": queries, "gallery_rows": n_gallery, "reference_mode": modes[0], "modes": out,
            "note": "targets = the fp32 ranking's row at a uniform position 0..63 per query; deltas in percentage points of queries "
                    "(1 pp = 1 query in 100).  delta_recall_at_50 = (targets that entered the top-50 - targets that left it) / queries: a "
                    "difference of two counts of boundary flips, with a standard error of sqrt(in + out) / queries (~0.5 pp here) -- two "
                    "modes whose deltas differ by less than that are not distinguishable on this table; top50_overlap is the stable figure"}


def harness_leg(torch, eng, clip, model, cfg, D, device, n_gal, lookup_qps, enc_ips, queries=2048, images=2048):
    """what a caller of the REFERENCE API gets.  The drop-in harness itself -- `compute_fiq_val_metrics` /
    `generate_fiq_val_predictions` (run/test/test_fiq.py:18-122) and `extract_index_features` (utils/utils.py:44-69), called exactly as
    the reference's driver calls them -- on a synthetic FashionIQ-shaped split at the C2 size: DataLoader batches on the HOST, captions
    tokenised on the host by the CLIP BPE algorithm (synthetic merge table: the released vocabulary is not available offline),
    host -> device copies per batch, the reference-feature lookup, mode="test", the gallery's mode="index" fusion and the ranking."""
    import numpy as np
    from fashionern_aaai2024_amd import synth
    from fashionern_aaai2024_amd.run.test_fiq import compute_fiq_val_metrics, generate_fiq_val_predictions
    from fashionern_aaai2024_amd.tokenizer import ClipBpeTokenizer, register_tokenizer
    from fashionern_aaai2024_amd.utils import extract_index_features
    letters = "abcdefghijklmnopqrstuvwxyz-"
    merges = [(a, b) for a in "sleroncdbtfpmv" for b in "aeioulrt"][:96] + [(a, b + "</w>") for a in letters[:20] for b in "esdrnty"][:96]
    register_tokenizer("bench-clip-bpe", ClipBpeTokenizer(merges))
    g = torch.Generator(device=device).manual_seed(77)
    index_features = torch.randn((n_gal, D), generator=g, device=device)
    index_local = torch.randn((n_gal, 13, D), generator=g, device=device)
    index_names = [f"img{i:06d}" for i in range(n_gal)]
    host_local = torch.from_numpy(synth.local_feats(256, D, 31, "bench-ql"))
    rel = _BenchRelativeDataset(queries, n_gal, host_local)
    out = {"queries": queries, "gallery_rows": n_gal, "batch_size": 64, "tokenizer": "ClipBpeTokenizer (CLIP BPE algorithm, synthetic merge table), host",
           "lanes": int(os.environ.get("FERN_HARNESS_LANES", "4"))}

    def timed(fn, reps=2):
        fn()                                          # first call: forks, workspaces, tile tuning
        best, val = None, None
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        return best, val

    nw = 4                                            # the reference driver's default (run/test/test_fiq.py:131)
    out["num_workers"] = nw
    t_pred, _ = timed(lambda: generate_fiq_val_predictions(clip, rel, model, index_names, index_features, device, D, 64, nw, "bench-clip-bpe"))
    t_full, rec = timed(lambda: compute_fiq_val_metrics(rel, clip, index_features, index_local, index_names, model, device, D, 64, nw, "bench-clip-bpe"))
    out["generate_fiq_val_predictions"] = {"wall_s": t_pred, "queries_per_s": queries / t_pred,
                                           "note": "the query loop alone (host batches -> tokenise -> upload -> lookup -> text tower -> mode=test): "
                                                   "the figure comparable with the engine's `lookup_variant`"}
    out["compute_fiq_val_metrics"] = {"wall_s": t_full, "queries_per_s": queries / t_full, "recall_at_10_50": list(rec),
                                      "note": "query loop + mode=index fusion of the whole gallery + ranking + recall arithmetic, per call as the reference does"}
    out["engine_lookup_variant_queries_per_s"] = lookup_qps
    out["predictions_vs_engine_lookup"] = (queries / t_pred) / lookup_qps if lookup_qps else None
    prev_lanes = os.environ.get("FERN_HARNESS_LANES")      # a value the user exported survives the toggle
    os.environ["FERN_HARNESS_LANES"] = "0"
    try:
        t_serial, _ = timed(lambda: generate_fiq_val_predictions(clip, rel, model, index_names, index_features, device, D, 64, nw, "bench-clip-bpe"), reps=1)
    finally:
        if prev_lanes is None:
            os.environ.pop("FERN_HARNESS_LANES", None)
        else:
            os.environ["FERN_HARNESS_LANES"] = prev_lanes
    out["generate_fiq_val_predictions_call_by_call"] = {"wall_s": t_serial, "queries_per_s": queries / t_serial,
                                                        "note": "FERN_HARNESS_LANES=0: the round-4 loop (one stream, two encode_text calls served by one pass)"}
    pool_im = torch.from_numpy(synth.images(32, cfg, 9))
    pool_lc = torch.from_numpy(synth.local_feats(32, D, 9, "bench-il"))
    ds = _BenchIndexDataset(images, pool_im, pool_lc)
    t_ext, res = timed(lambda: extract_index_features(ds, clip, 13, device, D), reps=1)
    out["extract_index_features"] = {"images": images, "wall_s": t_ext, "images_per_s": images / t_ext, "batch_size": 32, "num_workers": 4,
                                     "engine_encode_images_per_s": enc_ips,
                                     "note": "the reference's loop (utils/utils.py:44-69): batches of 32 from a 4-worker DataLoader, pinned host "
                                             "memory, one host -> device copy of 19 MB per batch, encode_image"}
    del index_features, index_local
    torch.cuda.empty_cache()
    return out


def dump_outputs(out_dir: str, res) -> None:
    """--dump-outputs: what the timed path returned for its last batch (a pipeline QueryResult) as DIR/<name>.npy -- top-K scores
    and gallery indices, the fused query features, c4's member scores; float32, indices as float64 (exact).  A few hundred KB."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    scores, idx = res.wait()
    for name, t in (("topk_scores", scores), ("topk_idx", idx), ("fused_queries", res.fused), ("member_scores", res.member_scores)):
        if t is not None:
            np.save(os.path.join(out_dir, name + ".npy"), (t.float() if t.is_floating_point() else t.double()).cpu().numpy())


COMPACT_CAP_BYTES = 4000      # the driver reads ONE stdout line; round 5's 24.6 KB line came back unparsed


def _r(x, sig=5):
    """Round a float to `sig` significant digits (the compact line is a summary; bench_full.json keeps every digit)."""
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x != x or x in (float("inf"), float("-inf")):
        return None
    return float(f"{x:.{sig}g}")


def _pick(d, *keys, sig=5):
    return {k: _r(d[k], sig) for k in keys if isinstance(d, dict) and d.get(k) is not None}


def compact_record(full: dict, cap: int = COMPACT_CAP_BYTES) -> dict:
    """The ONE stdout line the driver parses: the contract keys, `roofline` and `cpu_baseline` without their prose, and one number per
    extra leg (other configs, harness, PCIe-inclusive rate, reduced modes).  Everything else stays in the full record (bench_full.json +
    stderr).  Extras are dropped from the back until the line fits `cap` bytes; the contract keys, `roofline` and `cpu_baseline` never are."""
    out = {k: _r(full.get(k), 6) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                           "vs_baseline", "dtype", "data")}
    cfg = full.get("config") or {}
    out["config"] = {k: cfg[k] for k in ("workload", "name", "clip", "query_batch_per_gpu", "gallery_rows", "gallery_dtype", "feature_dim", "top_k",
                                         "batches_in_flight", "hw_queues") if k in cfg}
    out["config"]["parallelism"] = str(cfg.get("parallelism", "")).split(";")[0]
    out["encoder_precision"] = full.get("encoder_precision")
    roof = full.get("roofline")
    if roof:                                                # --full
        r = _pick(roof, "bound", "achieved", "peak", "unit", "frac")
        r["traffic"] = roof.get("traffic")                  # HBM counter bytes per launch; None unless measured at this HEAD
        r["kernel"] = str(roof.get("kernel", "")).split(" (")[0][:60]
        r.update(_pick(roof, "algorithmic_bytes_per_launch", "gemm_ms_per_step", "gemm_gflop_per_step"))
        if isinstance(roof.get("step_level"), dict):
            r["step_level"] = _pick(roof["step_level"], "achieved", "frac")
        out["roofline"] = r
    cb = full.get("cpu_baseline")
    if cb:
        c = _pick(cb, "value", "unit", "cores", "host_cores", "cpu_model", "kind")
        c["sample"] = str(cb.get("sample", ""))[:120]
        if isinstance(cb.get("parity_vs_hip"), dict):
            c["parity_vs_hip"] = _pick(cb["parity_vs_hip"], "queries", "rows_with_identical_order", "max_abs_cosine_diff",
                                       "max_oracle_score_gap_at_mismatching_positions", sig=3)
        out["cpu_baseline"] = c
    extras = []                                             # (key, value) in the order they are dropped LAST -> FIRST
    lat = full.get("latency_ms_per_batch")
    if lat:
        extras.append(("latency_ms_per_batch", _pick(lat, "p50", "p99", sig=4)))
    rs = full.get("roofline_sim_sweep")
    if rs:
        extras.append(("rank_stage", _pick(rs, "stage_us", "frac", "sweep_only_us", "sweep_only_GBs", sig=4)))
    oc = full.get("other_configs")
    if oc:
        o = {}
        for name, rec in oc.items():
            if "error" in rec:
                o[name] = {"error": rec["error"][:80]}
                continue
            e = {"value": _r(rec.get("value"), 5), "precision": rec.get("encoder_precision"),
                 "roofline_frac": _r((rec.get("roofline") or {}).get("frac"), 4), "rank_stage_us": _r(rec.get("rank_stage_us"), 4),
                 "rank_frac": _r(rec.get("rank_stage_frac_of_hbm"), 3)}
            rcl = (rec.get("accuracy_vs_fp32_encoder") or {}).get("recall") or {}
            if rcl:
                e["dR50_pp"] = _r(rcl.get("delta_recall_at_50_pp"), 3)
                e["dR50_se_pp"] = _r(rcl.get("delta_recall_at_50_se_pp"), 2)
                e["top50_overlap"] = _r(rcl.get("top50_overlap"), 3)
            o[name] = e
        extras.append(("other_configs", o))
    h = full.get("harness")
    if h:
        extras.append(("harness", {"generate_fiq_val_predictions_qps": _r(h["generate_fiq_val_predictions"]["queries_per_s"]),
                                   "compute_fiq_val_metrics_qps": _r(h["compute_fiq_val_metrics"]["queries_per_s"]),
                                   "extract_index_features_ips": _r(h["extract_index_features"]["images_per_s"])}))
    if full.get("pcie_inclusive"):
        extras.append(("pcie_inclusive", _pick(full["pcie_inclusive"], "value", "vs_resident_inputs")))
    if full.get("lookup_variant"):
        extras.append(("lookup_variant", _pick(full["lookup_variant"], "value")))
    modes = {}
    q = (full.get("reduced_modes") or {}).get("modes") or {}
    for m in ("f32x3", "bf16", "mx8mlp", "mx8img", "fp8", "mx8"):
        info = full.get("encoder_" + m)
        if info or m in q:
            e = {}
            if info:
                e.update({"qps": _r(info.get("value")), "gemm_frac": _r(info.get("gemm_frac"), 3)})
            if m in q:
                e.update({"dR50_pp": _r(q[m].get("delta_recall_at_50_pp"), 3), "dR50_se_pp": _r(q[m].get("delta_recall_at_50_se_pp"), 2),
                          "top50_overlap": _r(q[m].get("top50_overlap"), 3)})
            modes[m] = e
    if modes:
        extras.append(("modes", modes))
    if full.get("roofline_sim_sweep_bf16_1M"):
        extras.append(("rank_stage_bf16_1M", _pick(full["roofline_sim_sweep_bf16_1M"], "stage_us", "frac", sig=4)))
    if full.get("sharded_merge"):
        extras.append(("sharded_merge", _pick(full["sharded_merge"], "value", "identical_to_replicated")))
    ag = full.get("all_gather")
    if ag and full.get("n_gpus", 1) > 1:
        extras.append(("all_gather", _pick(ag, "ms", "GBs_per_rank", "frac_of_xgmi", sig=4)))
    if full.get("timing_s"):
        extras.append(("timing_s", full["timing_s"]))
    if full.get("full_record"):
        out["full_record"] = full["full_record"]
    for k, v in extras:
        out[k] = v
    while len(json.dumps(out)) > cap and extras:
        k, _ = extras.pop()
        out.pop(k, None)
    return out


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ:
        spawn_ranks(args)

    import torch
    import torch.distributed as dist
    from fashionern_aaai2024_amd import distributed as fd
    from fashionern_aaai2024_amd import synth
    from fashionern_aaai2024_amd.clip_model import create_model
    from fashionern_aaai2024_amd.model import ERN
    from fashionern_aaai2024_amd.pipeline import ComposedQueryPipeline

    rank, world, local = fd.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if os.environ.get("FERN_BENCH_SHARE_GPU"):      # debug only: several ranks on one GPU (with FERN_DIST_BACKEND=gloo)
        local = local % torch.cuda.device_count()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    w = dict(WORKLOADS[args.config])
    if args.gallery:
        w["gallery"] = args.gallery
    precision = args.precision or w["precision"]
    cfg = synth.CLIP_CONFIGS[w["clip"]]
    D, B, K, n_gal = w["d"], w["batch"], w["k"], w["gallery"]
    backend = dist.get_backend() if world > 1 else None
    gloo = backend == "gloo"
    preflight = multi_gpu_preflight(torch, dist, fd, rank, world, local, device, backend, measure=args.full) if world > 1 else None

    def dev_randn(shape, seed):
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        return torch.randn(shape, generator=g, device=device)

    gal_bf16_early = None      # filled right after the engine exists (see below)

    def collective(fn, *tensors):
        """torch.distributed collective on device tensors; the gloo debug backend (ranks sharing one GPU) goes through the host."""
        if not gloo:
            return fn(*tensors)
        host = [t.cpu() for t in tensors]
        fn(*host)
        tensors[0].copy_(host[0])

    # ---- weights (random init, real architecture) and synthetic inputs, resident in HBM --------------------
    stamp("imports_done")
    clip_sd = synth.clip_state_dict(cfg, seed=0)
    fusion_sd = synth.fusion_state_dict(D, seed=0)
    clip = create_model(cfg, device=device)
    clip.load_state_dict(clip_sd)
    model = ERN(clip, D, device, engine=clip.engine).load_state_dict(fusion_sd)
    eng = model.engine
    # The gallery store is allocated NOW, like a serving process allocates its gallery at start-up (the all-gather below writes
    # straight into it): a 1 GB buffer allocated after a minute of other work (workspaces of three lanes, tuner scratch, freed
    # sources) sits in small physical fragments and the same sweep kernel streams it ~20 % slower (209 vs 171 us on one box).
    _s0, _s1, _per = fd.shard_rows(n_gal, rank, world)
    gallery_store = torch.empty((world * _per, D), dtype=torch.bfloat16 if w["bf16_gallery"] else torch.float32, device=device)
    if args.full and not args.headline_only and args.config == "c2" and precision == "fp32":
        # the 1M-row bf16 gallery of the HBM-bound ranking leg is allocated NOW, like a serving process allocates its gallery at start-up:
        # allocated after a minute of other work (workspaces of three lanes, four precision modes, a freed 2 GB fp32 source) the same
        # kernel streams it 20 % slower (209 vs 171 us on one box) -- the buffer then sits in small physical fragments
        _src = torch.nn.functional.normalize(dev_randn((1_000_000, D), 3), dim=-1)
        gal_bf16_early = eng.gallery_to_bf16(_src)
        del _src
    n_batches = 3      # distinct input batches, rotated step by step
    batches = []
    for j in range(n_batches):
        seed = 42 + rank + 1000 * j
        batches.append((torch.from_numpy(synth.images(B, cfg, seed)).to(device), torch.from_numpy(synth.captions(B, cfg, seed)).to(device),
                        torch.from_numpy(synth.local_feats(B, D, seed)).to(device)))

    # ---- gallery build (not in the step): every rank synthesises + fuses ONLY its shard, one RCCL all_gather --------------
    start, stop, per = fd.shard_rows(n_gal, rank, world)
    gal_dtype = torch.bfloat16 if w["bf16_gallery"] else torch.float32

    def build_shard():
        block = torch.zeros((per, D), dtype=gal_dtype, device=device)
        ch = 32_768
        for o in range(start, stop, ch):
            m = min(ch, stop - o)
            raw = dev_randn((m, D), (7 + rank) * 1_000_003 + o)
            lcl = dev_randn((m, 13, D), (11 + rank) * 1_000_003 + o)
            fused = eng.index_fuse(raw, lcl, normalize_input=True)
            block[o - start:o - start + m] = eng.gallery_to_bf16(fused) if w["bf16_gallery"] else fused
        return block

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # fp32 galleries are ranked through their PREPARED form (engine.prepare_gallery: bf16 pre-filter copy + the norms that certify it;
    # built once, like the index itself): the same exact fp32 scores and ordering, one HBM-bound bf16 pass + rescoring of the few rows
    # that can still be in the top-K instead of an fp32-MFMA-bound sweep.  Round 6: every rank prepares ONLY ITS SHARD; the fp32 and the
    # bf16 blocks are all-gathered and the norms MAX-reduced (distributed.all_gather_prepared) -- round 5 prepared the whole gathered
    # gallery on every rank.  --rank-plain keeps the round-4 stage (plain fp32 gallery) for comparison.
    use_prepared = not w["bf16_gallery"] and not args.rank_plain
    prep_store = None
    if use_prepared:
        from fashionern_aaai2024_amd.engine import PreparedGallery
        prep_store = PreparedGallery(gallery_store, torch.empty((world * _per, D), dtype=torch.bfloat16, device=device),
                                     torch.zeros(4, dtype=torch.float32, device=device))

    def gather(block):
        if use_prepared:
            return fd.all_gather_prepared(eng, block, n_gal, out=prep_store)
        return fd.all_gather_shards(block, n_gal, out=gallery_store)      # bytes on the wire; the gloo debug backend is staged through the host in there

    stamp("weights_and_inputs_resident")
    shard = build_shard()
    gallery = gather(shard)                    # warm (RCCL connection setup, workspaces)
    barrier()
    fuse_s = prepare_ms = ag_ms = None
    if args.full:                              # the gallery build's own figures: the same build again, timed
        t0 = time.perf_counter()
        shard = build_shard()
        torch.cuda.synchronize()
        fuse_s = time.perf_counter() - t0
        if use_prepared:                       # this rank's share of the preparation (its shard), timed on its own
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.prepare_gallery(shard)
            torch.cuda.synchronize()
            prepare_ms = (time.perf_counter() - t0) * 1e3
        barrier()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        gallery = gather(shard)
        ev1.record()
        torch.cuda.synchronize()
        ag_ms = ev0.elapsed_time(ev1)
    ag_bytes = (world - 1) * per * D * (shard.element_size() + (2 if use_prepared else 0))      # bytes this rank receives (fp32 rows + their bf16 copy)
    shard_start = start
    gallery_raw = gallery.f32 if use_prepared else gallery

    # CIRR extras (c4): one excluded gallery index (the reference image) and 6 img_set members per query
    ex_idx = members = None
    if w["cirr"]:
        g = torch.Generator().manual_seed(4 + rank)
        ex_idx = torch.randint(0, n_gal, (B,), generator=g, dtype=torch.int32).to(device)
        members = torch.randint(0, n_gal, (B, 6), generator=g, dtype=torch.int32).to(device)
        members[:, 0] = ex_idx

    pipe = ComposedQueryPipeline(eng, lanes=args.lanes, timing=True, graphs=args.graphs)
    pipe.set_precision(precision)
    step_no = [0]

    def step():          # one batch of composed queries; consecutive steps go to consecutive lanes (streams) and rotate the input batch
        im, tk, lc = batches[step_no[0] % n_batches]
        step_no[0] += 1
        return pipe.submit(im, tk, lc, gallery, K, exclude_idx=ex_idx, members=members)

    def step_serial(j=0):   # the same work on the current stream (instrumented / PMC passes)
        im, tk, lc = batches[j % n_batches]
        rf, tg, ts = eng.encode_pair(im, tk)        # what the pipeline's lanes call (pipeline.py: _step)
        q = eng.dvr_fuse(rf, lc, tg, ts)
        out = eng.sim_topk_bf16(q, gallery, K, exclude_idx=ex_idx) if w["bf16_gallery"] else eng.sim_topk(q, gallery, K, exclude_idx=ex_idx)
        if members is not None:
            eng.gather_scores(q, gallery, members)
        return out

    last_latency = [None]

    def timed_loop(fn, steps):
        """`steps` calls of fn bracketed by barrier + synchronize; max over ranks.  Also the median gap between consecutive
        batches' completion events (hipEvents on the lanes' streams): a per-step figure that one slow step does not move."""
        barrier()
        t0 = time.perf_counter()
        outs = [fn() for _ in range(steps)]
        barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device=device)
            collective(lambda x: dist.all_reduce(x, op=dist.ReduceOp.MAX), t)
            el = t.item()
        # consecutive batches of ONE lane complete in order on that lane's stream: the gap between batch i and batch i + lanes,
        # divided by the lanes that interleave with them, is a per-step service time
        gaps = []
        evs = [o.done_event for o in outs if hasattr(o, "done_event")]
        nl = args.lanes
        for a, b in zip(evs[:-nl], evs[nl:]):
            gaps.append(a.elapsed_time(b) / nl)
        # per-batch service latency: the batch's first kernel reaches the head of its lane -> its top-K is complete, with the
        # other lanes' batches in flight beside it (throughput is quoted with `lanes` batches in flight; this is what one batch pays)
        lat = sorted(o.start_event.elapsed_time(o.done_event) for o in outs if getattr(o, "start_event", None) is not None)
        last_latency[0] = None if not lat else {"p50": lat[len(lat) // 2], "p99": lat[min(len(lat) - 1, int(0.99 * len(lat)))],
                                                "max": lat[-1], "batches": len(lat), "batches_in_flight": nl,
                                                "note": "hipEvent on the batch's lane in front of its first kernel -> event behind its last, "
                                                        "other lanes busy; queueing behind earlier batches of the same lane is not included"}
        return el, outs[-1], (statistics.median(gaps) if gaps else None)

    for _ in range(max(args.warmup, args.lanes, n_batches)):      # every lane's workspace / every tuned shape exists before the timed region
        step()
    barrier()
    if world > 1:      # all ranks run rank 0's tile choices: a max-over-ranks step time must not carry rank-to-rank tuner noise
        fd.share_gemm_tiles(eng)
        for _ in range(max(args.lanes, n_batches)):
            step()
        barrier()
    if args.pmc_mode:      # tools/pmc_traffic.py keys on this single-workgroup l2norm dispatch to find the measured steps
        pipe.set_precision(precision)
        for j in range(n_batches):
            step_serial(j)
        torch.cuda.synchronize()
        eng.l2_normalize(torch.zeros(3, 64, device=device))
        for j in range(args.steps):
            step_serial(j)
        barrier()
        return
    stamp("gallery_built_and_warm")
    elapsed, last, gap_median = timed_loop(step, args.steps)
    stamp("timed_region_done")
    value = world * B * args.steps / elapsed
    headline_latency = last_latency[0]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last)
    head = {
        "metric": "composed queries/sec", "value": value, "unit": "queries/sec", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": {"fp32": "f32", "f32x3": "bf16x3", "bf16": "bf16", "fp8": "fp8", "mx8": "fp8", "mx8mlp": "fp8", "mx8img": "fp8"}[precision], "data": "synthetic",
        "config": {"workload": w["text"], "name": args.config, "clip": cfg.name, "query_batch_per_gpu": B, "gallery_rows": n_gal,
                   "gallery_dtype": "bf16" if w["bf16_gallery"] else "f32", "feature_dim": D, "top_k": K,
                   "image": f"3x{cfg.image_size}x{cfg.image_size}", "tokens": 77, "patch_feats": 13, "batches_in_flight": args.lanes,
                   "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
                   "input_batches_rotated": n_batches,
                   "parallelism": f"dp{world} queries; gallery built sharded ({per} rows per rank, seed + rank), fused blocks all-gathered once"},
        "ms_per_step_event_median": gap_median,
        "latency_ms_per_batch": headline_latency,
        "encoder_precision": precision,
    }
    if not args.full:      # the headline line only; everything below is --full
        if rank == 0:
            print(json.dumps(compact_record(head)), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- c5 only: gallery-SHARDED ranking (SURVEY 8e alternative): all-gather the fused queries, sweep the local shard for all of
    # them, all-gather the candidates, merge -- every rank reads N/W gallery rows per batch instead of N
    sharded_info = None
    if args.config == "c5":
        my = shard[: stop - start]

        def step_sharded():
            im, tk, lc = batches[step_no[0] % n_batches]
            step_no[0] += 1
            rf = eng.encode_image(im)
            tg, ts = eng.encode_text(tk)
            q = eng.dvr_fuse(rf, lc, tg, ts)
            if world == 1:
                return eng.sim_topk_bf16(q, my, K, idx_offset=shard_start)
            allq = torch.empty((world * B, D), dtype=torch.float32, device=device)
            collective(lambda o, i: dist.all_gather_into_tensor(o, i), allq, q)
            s, i = eng.sim_topk_bf16(allq, my, K, idx_offset=shard_start)
            all_s = torch.empty((world, world * B, K), dtype=torch.float32, device=device)
            all_i = torch.empty((world, world * B, K), dtype=torch.int32, device=device)
            collective(lambda o, x: dist.all_gather_into_tensor(o.view(-1, K), x), all_s, s)
            collective(lambda o, x: dist.all_gather_into_tensor(o.view(-1, K), x), all_i, i)
            return eng.topk_merge(all_s[:, rank * B:(rank + 1) * B].contiguous(), all_i[:, rank * B:(rank + 1) * B].contiguous())

        for _ in range(3):
            step_sharded()
        el, out_sh, _ = timed_loop(step_sharded, args.steps)
        step_no[0] -= 1
        ref_s, ref_i = step_serial(step_no[0])          # the replicated path on the same input batch
        torch.cuda.synchronize()
        sharded_info = {"value": world * B * args.steps / el, "unit": "queries/sec", "ms_per_step": el / args.steps * 1e3,
                        "gallery_rows_per_gpu": stop - start, "collectives_per_step": 0 if world == 1 else 3,
                        "identical_to_replicated": bool(torch.equal(out_sh[1], ref_i) and torch.equal(out_sh[0], ref_s)),
                        "note": "one stream (collectives between the stages); the replicated variant keeps batches in flight on 3 streams"}

    # ---- reduced-precision encoder modes on the c2 workload: reported beside the fp32 headline, never as its `value`
    # (north_star's parity bar -- scores within 1e-3, identical ordering -- is an fp32 statement)
    def reduced_precision_leg(prec, ref_scores, ref_idx):
        pipe.set_precision(prec)
        for _ in range(max(args.warmup, args.lanes, n_batches)):
            step()
        step_no[0] = 0
        el, out_b, _ = timed_loop(step, args.steps)
        step_no[0] = 0
        b_scores, b_idx = step().wait()
        eng.prof_enable(True)
        for j in range(2):
            step_serial(j)
        sp = eng.prof_collect()
        eng.prof_enable(False)
        key = {"fp8": "gemm_fp8", "mx8": "gemm_mx8", "mx8mlp": "gemm_mx8", "mx8img": "gemm_mx8", "bf16": "gemm_bf16", "f32x3": "gemm"}[prec]
        # f32x3: the GEMMs stay fp32 GEMMs algorithmically (2MNK flop each, accounted under the fp32 family) but run six 32-cycle bf16
        # MFMAs per pair of 64-cycle fp32 MFMAs, so the bound of their arithmetic is 157.3 x 128 / 48 = 419.5 fp32-equivalent TFLOP/s:
        # THAT is the peak `gemm_frac` is quoted against (quoted against the fp32 peak it read 0.987 and was no roofline fraction)
        peak = mixed_peak(sp) if prec in ("mx8", "mx8mlp", "mx8img") else F32X3_BOUND_TFLOPS if prec == "f32x3" else BF16_MFMA_PEAK_TFLOPS
        tfl = sp[key + "_flops"] / (sp[key + "_ms"] * 1e-3) / 1e12 if sp[key + "_ms"] > 0 else 0.0
        overlap = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(ref_idx.cpu(), b_idx.cpu())) / ref_idx.numel()
        info = {"value": world * B * args.steps / el, "unit": "queries/sec", "ms_per_step": el / args.steps * 1e3,
                "latency_ms_per_batch": last_latency[0],
                "dtype": ("f32 data; plain GEMMs of >= 256 rows as three bf16 planes per operand, six bf16 MFMAs per fp32 pair, f32 accumulate "
                          "(fp32-accurate, not the bit-exact fma chain; attention, statistics and the ranking stage unchanged)") if prec == "f32x3" else
                         {"bf16": "bf16", "fp8": "fp8 e4m3fn (per-token / per-channel scales)",
                          "mx8": "fp8 e4m3fn, one E8M0 scale per 32-element block (block-scaled MFMA)",
                          "mx8mlp": "image tower's MLP pair (c_fc, c_proj): fp8 e4m3fn block-scaled; QKV / out-proj and the text tower: bf16 --",
                          "mx8img": "image tower's four token-level GEMMs: fp8 e4m3fn block-scaled over the fp32 residual stream; text tower: bf16 --"}[prec] +
                         " operands, f32 accumulate (encoder block GEMMs; attention and the fusion BERT blocks in bf16 operand form)",
                "gemm_tflops": tfl, "gemm_peak_tflops": peak, "gemm_frac": tfl / peak,
                "gemm_speedup_vs_fp32_mfma_peak": (tfl / F32_MFMA_PEAK_TFLOPS) if prec == "f32x3" else None,
                "gemm_ms_per_step": sp[key + "_ms"] / 2, "gemm_f32_ms_per_step": sp["gemm_ms"] / 2, "attention_ms_per_step": sp["attn_ms"] / 2,
                "vs_fp32_top1_same": float((ref_idx[:, 0] == b_idx[:, 0]).float().mean().item()),
                "vs_fp32_top50_overlap": overlap,
                "vs_fp32_max_abs_top1_score_diff": float((ref_scores[:, 0] - b_scores[:, 0]).abs().max().item())}
        pipe.set_precision(precision)
        return info

    secondary = not args.headline_only and args.config == "c2" and precision == "fp32"
    bf16_info = fp8_info = mx8_info = f32x3_info = mx8mlp_info = mx8img_info = accuracy = quality = None
    if secondary:
        step_no[0] = 0
        ref_scores, ref_idx = step().wait()
        f32x3_info = reduced_precision_leg("f32x3", ref_scores, ref_idx)
        bf16_info = reduced_precision_leg("bf16", ref_scores, ref_idx)
        fp8_info = reduced_precision_leg("fp8", ref_scores, ref_idx)
        mx8_info = reduced_precision_leg("mx8", ref_scores, ref_idx)
        mx8mlp_info = reduced_precision_leg("mx8mlp", ref_scores, ref_idx)
        mx8img_info = reduced_precision_leg("mx8img", ref_scores, ref_idx)
        if rank == 0:
            pipe.synchronize()
            quality = retrieval_quality_leg(torch, eng, cfg, D, device, ["fp32", "f32x3", "bf16", "mx8mlp", "mx8img", "fp8", "mx8"])
            for name, info in (("f32x3", f32x3_info), ("bf16", bf16_info), ("mx8mlp", mx8mlp_info), ("mx8img", mx8img_info), ("fp8", fp8_info), ("mx8", mx8_info)):
                quality["modes"][name]["queries_per_s"] = info["value"]
            quality["modes"]["fp32"]["queries_per_s"] = value
    elif not args.headline_only and precision in ("fp8", "mx8", "mx8mlp", "mx8img"):
        # c5: what the timed fp8 form costs in ranking agreement with the fp32 encoder on the same gallery, and the other fp8 form
        pipe.set_precision("fp32")
        step_no[0] = 0
        ref_scores, ref_idx = step().wait()
        pipe.set_precision(precision)
        step_no[0] = 0
        t_scores, t_idx = step().wait()
        accuracy = {"vs_fp32_top1_same": float((ref_idx[:, 0] == t_idx[:, 0]).float().mean().item()),
                    "vs_fp32_top50_overlap": sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(ref_idx.cpu(), t_idx.cpu())) / ref_idx.numel(),
                    "vs_fp32_max_abs_top1_score_diff": float((ref_scores[:, 0] - t_scores[:, 0]).abs().max().item())}
        others = [m for m in ("mx8img", "mx8", "mx8mlp", "fp8") if m != precision]
        infos = {m: reduced_precision_leg(m, ref_scores, ref_idx) for m in others}
        fp8_info, mx8_info, mx8mlp_info, mx8img_info = infos.get("fp8"), infos.get("mx8"), infos.get("mx8mlp"), infos.get("mx8img")
        if rank == 0:
            pipe.synchronize()
            quality = retrieval_quality_leg(torch, eng, cfg, D, device, ["fp32", precision] + others)
            for m in others:
                quality["modes"][m]["queries_per_s"] = infos[m]["value"]
            quality["modes"][precision]["queries_per_s"] = value
            accuracy["recall"] = quality["modes"][precision]

    stamp("mode_and_quality_legs_done")
    # ---- roofline: instrumented passes (events around every kernel class), outside the timed region ----------
    for j in range(n_batches):
        step_serial(j)
    torch.cuda.synchronize()
    eng.prof_enable(True)
    prof_steps = max(3, min(6, args.steps))
    for j in range(prof_steps):
        step_serial(j)
    st = eng.prof_collect()
    eng.prof_enable(False)
    gkey = {"fp32": "gemm", "f32x3": "gemm", "bf16": "gemm_bf16", "fp8": "gemm_fp8", "mx8": "gemm_mx8", "mx8mlp": "gemm_mx8", "mx8img": "gemm_mx8"}[precision]      # the dominant GEMM family of this run
    gemm_tflops = st[gkey + "_flops"] / (st[gkey + "_ms"] * 1e-3) / 1e12 if st[gkey + "_ms"] > 0 else 0.0
    gemm_peak = {"fp32": F32_MFMA_PEAK_TFLOPS, "f32x3": F32X3_BOUND_TFLOPS, "mx8": MX8_MFMA_PEAK_TFLOPS, "mx8mlp": MX8_MFMA_PEAK_TFLOPS, "mx8img": MX8_MFMA_PEAK_TFLOPS}.get(precision, BF16_MFMA_PEAK_TFLOPS)
    if gkey == "gemm_mx8":
        gemm_peak = mixed_peak(st)
    attn_tflops = st["attn_flops"] / (st["attn_ms"] * 1e-3) / 1e12 if st["attn_ms"] > 0 else 0.0

    def sweep_block(stats, calls, kernel, alg_bytes_per_call=None):
        """The ranking stage against SURVEY 8d's bytes (N*D*s_g + B*D*4 + B*K*8 per call, s_g = the bytes per element of the gallery the
        CALLER holds: 4 for an fp32 gallery even when the stage streams its bf16 pre-filter copy): `achieved` counts the WHOLE stage
        (every launch of it and the boundaries between them), `sweep_only_*` the sweep kernel alone against the bytes IT moves."""
        if calls <= 0 or stats["sweep_ms"] <= 0:
            return None
        total_ms = stats["sweep_ms"] + stats["topk_ms"]
        kb = stats["sweep_bytes"]
        by = alg_bytes_per_call * calls if alg_bytes_per_call else kb
        return {"bound": "hbm", "achieved": by / (total_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": by / (total_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None, "kernel": kernel,
                "algorithmic_bytes_per_call": by / calls, "stage_us": total_ms / calls * 1e3,
                "sweep_only_us": stats["sweep_ms"] / calls * 1e3, "sweep_kernel_bytes_per_call": kb / calls,
                "sweep_only_GBs": kb / (stats["sweep_ms"] * 1e-3) / 1e9,
                "selection_us": stats["topk_ms"] / calls * 1e3}

    if w["bf16_gallery"]:
        sweep_kernel = "sweep_bf16_kernel<FILTER> (bf16 gallery) + topk_sample_bound_kernel / topk_candidates_kernel; the [B, N] score matrix is never stored"
    elif args.rank_plain:
        sweep_kernel = ("gemm_f32 kernels with the EPI_TOPK_FILTER epilogue (fp32 gallery) + topk_sample_bound_kernel / topk_candidates_kernel; "
                        "the [B, N] score matrix is never stored")
    else:
        sweep_kernel = ("certified bf16 pre-filter + exact fp32 rescoring of an fp32 gallery (fern_sim_topk_prefiltered): sweep_bf16_kernel over the "
                        "prepared bf16 copy, then one select-and-rescore kernel (dense form: the sweep stores its [B, N] approximate scores and, per "
                        "32 gallery rows, their maximum -- topk_tiles_rescore_kernel selects on those maxima from 16 384 rows up, "
                        "topk_dense_rescore_kernel walks the rows below) or sample bound - margin + candidate lists + topk_rescore_kernel (galleries "
                        "whose score matrix would be real traffic); scores and order are the fp32 fma chain's.  stage_us = first dispatch begin -> "
                        "last dispatch end of the stage (dispatch timestamps)")
    alg_rank_bytes = float(n_gal) * D * (2 if w["bf16_gallery"] else 4) + B * D * 4 + B * K * 8
    rank_roof = sweep_block(st, prof_steps, sweep_kernel, alg_rank_bytes)
    rank_plain_roof = None
    if rank == 0 and not w["bf16_gallery"] and not args.rank_plain and not args.pmc_mode:
        # the same stage on the un-prepared gallery (round 4's fp32-MFMA sweep), and that the two agree bit for bit
        im, tk, lc = batches[0]
        qf = eng.dvr_fuse(eng.encode_image(im), lc, *eng.encode_text(tk))
        for _ in range(3):
            eng.sim_topk(qf, gallery_raw, K, exclude_idx=ex_idx)
        eng.prof_enable(True)
        for _ in range(10):
            ps, pi = eng.sim_topk(qf, gallery_raw, K, exclude_idx=ex_idx)
        sp = eng.prof_collect()
        eng.prof_enable(False)
        fs, fi = eng.sim_topk(qf, gallery, K, exclude_idx=ex_idx)
        rank_plain_roof = sweep_block(sp, 10, "fern_sim_topk: gemm_f32 EPI_TOPK_FILTER sweep on the fp32 gallery (round 4's stage)", alg_rank_bytes)
        rank_plain_roof["identical_to_prefiltered"] = bool(torch.equal(ps, fs) and torch.equal(pi, fi))
        if not rank_plain_roof["identical_to_prefiltered"]:
            raise SystemExit("bench: the pre-filtered ranking differs from the fp32 sweep's")

    enc_ips = lookup_qps = None
    big_roof = None
    harness_info = None
    pcie_info = None
    if secondary:
        im, tk, lc = batches[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            eng.encode_image(im)
        torch.cuda.synchronize()
        enc_ips = 3 * B / (time.perf_counter() - t0)

        # reference-faithful query variant (run/test/test_fiq.py:104-107): the reference image feature is LOOKED UP in the raw
        # gallery index instead of being encoded per query -> text tower + fusion + rank only
        ref_feats = dev_randn((B, D), 99)

        def step_lookup():      # the same lanes (streams) as the headline step
            return pipe.submit(None, tk, lc, gallery, K, ref_feats=ref_feats)

        for _ in range(2 * args.lanes):
            step_lookup()
        pipe.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step_lookup()
        pipe.synchronize()
        torch.cuda.synchronize()
        lookup_qps = B * args.steps / (time.perf_counter() - t0)

        # PCIe-inclusive rate (measured, not the 3 % estimate): the step's inputs start in PINNED HOST memory --
        # 38.5 MB of images, tokens, 1.7 MB of patch features per batch -- and are copied by a dedicated stream into rotating device
        # staging buffers while earlier batches compute; `value` of the main line keeps its inputs resident in HBM
        host_batches = [tuple(t.cpu().pin_memory() for t in bt) for bt in batches]
        n_sets = 2 * args.lanes
        staging = [tuple(torch.empty_like(t) for t in batches[0]) for _ in range(n_sets)]
        set_done = [None] * n_sets
        copy_stream = torch.cuda.Stream(device=device)
        pc = [0]

        def step_pcie():
            j = pc[0] % n_sets
            src = host_batches[pc[0] % n_batches]
            pc[0] += 1
            with torch.cuda.stream(copy_stream):
                if set_done[j] is not None:
                    copy_stream.wait_event(set_done[j])          # the batch that last used this staging set has been consumed
                for dst, hs in zip(staging[j], src):
                    dst.copy_(hs, non_blocking=True)
                up = torch.cuda.Event()
                up.record(copy_stream)
            torch.cuda.current_stream().wait_event(up)
            r = pipe.submit(*staging[j], gallery, K)
            set_done[j] = r.done_event
            return r

        for _ in range(2 * n_sets):
            step_pcie()
        pipe.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step_pcie()
        pipe.synchronize()
        torch.cuda.synchronize()
        pcie_s = time.perf_counter() - t0
        in_bytes = sum(t.numel() * t.element_size() for t in host_batches[0])
        pcie_info = {"value": B * args.steps / pcie_s, "unit": "queries/sec", "ms_per_step": pcie_s / args.steps * 1e3,
                     "host_to_device_bytes_per_step": in_bytes, "host_to_device_GBs": in_bytes * args.steps / pcie_s / 1e9,
                     "vs_resident_inputs": (B * args.steps / pcie_s) / value,
                     "note": "inputs in pinned host memory, uploaded per step by a dedicated copy stream into rotating staging buffers "
                             f"({n_sets} sets), {args.lanes} batches in flight; one GPU's share"}
        del staging, host_batches

        # HBM-bound form of the ranking stage (BASELINE config 5 "bf16 similarity"): 1M-row bf16 gallery, 64 queries
        big_n = 1_000_000
        gal_bf16 = gal_bf16_early
        q_unit = torch.nn.functional.normalize(dev_randn((B, D), 5), dim=-1)
        for _ in range(3):
            eng.sim_topk_bf16(q_unit, gal_bf16, K)
        eng.prof_enable(True)
        for _ in range(10):
            eng.sim_topk_bf16(q_unit, gal_bf16, K)
        sb = eng.prof_collect()
        eng.prof_enable(False)
        big_roof = sweep_block(sb, 10, "sweep_bf16_kernel<FILTER>: 64 queries x 1M-row bf16 gallery + sample bound / candidate select")
        del gal_bf16
        gal_bf16_early = None
        torch.cuda.empty_cache()
        harness_info = harness_leg(torch, eng, clip, model, cfg, D, device, n_gal, lookup_qps, enc_ips) if rank == 0 else None

    stamp("roofline_lookup_pcie_1M_harness_legs_done")
    result = None
    if rank == 0:
        traffic = traffic_src = alg_bytes = sweep_traffic = None
        traffic_file = os.path.join(ROOT, "profiles", "pmc_traffic_c5.json" if args.config == "c5" else "pmc_traffic.json")
        if os.path.exists(traffic_file) and args.config in ("c2", "c5") and precision == w["precision"]:
            tr = json.load(open(traffic_file))
            fam = "gemm_mx8" if args.config == "c5" and "gemm_mx8" in tr else "gemm"
            if (tr.get("measured") or {}).get("csrc_sha16") == csrc_sha16():
                traffic = tr.get(fam, {}).get("hbm_bytes_per_launch")
                alg_bytes = tr.get(fam, {}).get("algorithmic_bytes_per_launch")
                sweep_traffic = tr.get("sweep", {}).get("hbm_bytes_per_launch")
                traffic_src = ("profiles/" + os.path.basename(traffic_file) + ": separate `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes of "
                               "`bench.py --pmc-mode` on THESE kernel sources (csrc_sha16 " + csrc_sha16() + "; " + str(tr.get("source")) + ")")
            else:
                traffic_src = ("omitted: " + os.path.basename(traffic_file) + " was measured on other kernel sources (" +
                               json.dumps(tr.get("measured")) + "), this tree is csrc_sha16 " + csrc_sha16())
        result = {
            **head,
            "rccl_world": world if backend == "nccl" else (1 if world == 1 else f"{world} (debug backend {backend})"),
            "preflight": preflight,
            "all_gather": {"ms": ag_ms if world > 1 else 0.0, "bytes_received_per_rank": ag_bytes,
                           "GBs_per_rank": (ag_bytes / (ag_ms * 1e-3) / 1e9) if world > 1 and ag_ms > 0 else None,
                           "xgmi_peak_GBs_per_gpu": XGMI_PEAK_GBS,
                           "frac_of_xgmi": (ag_bytes / (ag_ms * 1e-3) / 1e9 / XGMI_PEAK_GBS) if world > 1 and ag_ms > 0 else None,
                           "shard_rows": per, "collective": "all_gather_into_tensor of the fused [rows/rank, D] fp32 blocks" + (" + of their bf16 pre-filter copies (each rank prepares only its shard), all_reduce(MAX) of the 4 norms" if use_prepared else "")},
            "roofline": {"bound": "mfma", "achieved": gemm_tflops, "peak": gemm_peak, "unit": "TFLOP/s",
                         "frac": gemm_tflops / gemm_peak, "traffic": traffic, "traffic_source": traffic_src,
                         "algorithmic_bytes_per_launch": st["gemm_alg_bytes"] / max(1, st["gemm_launches"]) if precision == "fp32" else alg_bytes,
                         "kernel": {"fp32": "gemm_f32_glds_kernel / gemm_f32_kernel (fp32 MFMA GEMM, all tile variants)",
                                    "f32x3": "gemm_f32_glds_kernel<SPLIT=3> (fp32 operands as three bf16 planes; peak = the six-product bf16 bound, 419.5 fp32-equivalent TFLOP/s)",
                                    "bf16": "gemm_bf16_glds_kernel (bf16 MFMA GEMM of the encoder blocks)",
                                    "fp8": "gemm_bf16_glds_kernel<FP8> (fp8 MFMA GEMM of the encoder blocks)",
                                    "mx8": "gemm_mx8_kernel (block-scaled fp8 GEMM of the encoder blocks, v_mfma_scale_f32_32x32x64_f8f6f4)",
                                    "mx8mlp": "gemm_mx8_kernel (block-scaled fp8 GEMMs of the MLP pair; QKV / out-proj run on gemm_bf16_glds_kernel)",
                                    "mx8img": "gemm_mxbf_pair_kernel / gemm_mx8_kernel (block-scaled fp8 GEMMs of the image tower, v_mfma_scale_f32_32x32x64_f8f6f4, "
                                              "each carrying the text tower's bf16 GEMM of the same layer in its launch: the flops of both over the launch's "
                                              "time; `peak` prices the fp8 part at 5 and the bf16 part at 2.5 PFLOP/s -- bench.mixed_peak; fusion BERT on "
                                              "the bf16 kernels)"}[precision],
                         "peak_basis": "nominal (MI355X_MICROARCH.md, 2.4 GHz).  Measured on this pool with operands in registers and random data "
                                       "(tools/probe/mfma_issue_probe.hip, bf16_issue_probe.hip, mx_issue_probe.hip; profiles/r04_*_issue_probe.txt): the "
                                       "MFMA stream itself delivers 140-156 TFLOP/s fp32 (~2.04 GHz held inside the GEMM), 1.9-2.0 PFLOP/s bf16 and "
                                       "4.05 PFLOP/s block-scaled fp8 (~1.93 GHz) -- the nominal peaks are not reachable under load",
                         "regime": "serial_passes: `achieved` = sum of 2MNK / sum of the dispatches' own begin-end timestamps (hipExtLaunchKernelGGL "
                                   "event pairs) over every launch of the family "
                                   "in INSTRUMENTED ONE-STREAM passes of the step (run after the timed region); the timed region itself keeps "
                                   f"{args.lanes} batches in flight, so `gemm_ms_per_step` may exceed `ms_per_step` -- `step_level` is the same "
                                   "flop count over the timed wall clock",
                         "step_level": {"achieved": st[gkey + "_flops"] / prof_steps / 1e12 / (elapsed / args.steps),
                                        "frac": st[gkey + "_flops"] / prof_steps / 1e12 / (elapsed / args.steps) / gemm_peak,
                                        "note": "family flops per step / timed ms_per_step (multi-lane regime): a LOWER bound of the family's "
                                                "rate -- the wall clock also holds every other kernel of the step"},
                         "gemm_ms_per_step": st[gkey + "_ms"] / prof_steps, "gemm_gflop_per_step": st[gkey + "_flops"] / prof_steps / 1e9,
                         "gemm_launches_per_step": st[gkey + "_launches"] / prof_steps,
                         "gemm_dispatches_per_step": (st["gemm_dispatches"] / prof_steps) if precision == "fp32" else None,
                         "gemm_us_per_dispatch": (st["gemm_ms"] * 1e3 / max(1, st["gemm_dispatches"])) if precision == "fp32" else None,
                         "f32_gemm_ms_per_step": st["gemm_ms"] / prof_steps},
            "roofline_sim_sweep": rank_roof,
            "roofline_sim_sweep_fp32_mfma_form": rank_plain_roof,
            "gallery_prepare_ms": prepare_ms,
            "roofline_sim_sweep_bf16_1M": big_roof,
            "encoder_f32x3": f32x3_info,
            "encoder_bf16": bf16_info,
            "encoder_fp8": fp8_info,
            "encoder_mx8": mx8_info,
            "encoder_mx8mlp": mx8mlp_info,
            "encoder_mx8img": mx8img_info,
            "reduced_modes": quality,
            "accuracy_vs_fp32_encoder": accuracy,
            "sharded_merge": sharded_info,
            "attention": {"achieved_tflops": attn_tflops, "ms_per_step": st["attn_ms"] / prof_steps},
            "harness": harness_info,
            "pcie_inclusive": pcie_info,
            "lookup_variant": None if lookup_qps is None else {"value": lookup_qps * world, "unit": "queries/sec",
                               "note": "reference-faithful query path (test_fiq.py:104-107): reference features looked up in the index, "
                                       f"no per-query image encode; {args.lanes} batches in flight like the headline"},
            "gallery_build": {"shard_fuse_s": fuse_s, "rows_per_s_per_gpu": (stop - start) / fuse_s if fuse_s > 0 else None,
                              "rows_per_s_all_gpus": n_gal / fuse_s if fuse_s > 0 else None,
                              "encode_images_per_s_per_gpu": enc_ips},
            "gemm_tiles": eng.tuner_export().strip().split("\n"),
            "gemm_tiles_pinned_from": os.environ.get("FERN_GEMM_TILES"),
        }
        if rank_roof is not None:
            rank_roof["traffic"] = sweep_traffic
        if args.save_tiles:
            with open(args.save_tiles, "w") as f:
                f.write(eng.tuner_export())
        children = None

        def start_children():
            """The other BASELINE configs as child runs of this script, one after the other on a background thread, started when THIS process
            has made its last GPU call: after the CPU-baseline leg, or beside it under FERN_BENCH_OVERLAP_CHILDREN=1 (see there)."""
            if not (world == 1 and args.config == "c2" and not args.headline_only and not args.no_other_configs and not args.pmc_mode):
                return None
            import threading
            pipe.close()
            torch.cuda.synchronize()
            stamp("other_configs_started")
            box = {}
            th = threading.Thread(target=lambda: box.update(r=other_config_lines(min(args.steps, 20))), daemon=True)
            th.start()
            return th, box

        if world == 1 and not args.no_cpu_baseline:
            pipe.set_precision("fp32")      # the oracle is an fp32 statement: compare it with the fp32 path, whatever was timed
            im, tk, lc = batches[0]
            rf = eng.encode_image(im)
            tg, ts = eng.encode_text(tk)
            qf = eng.dvr_fuse(rf, lc, tg, ts)
            gpu_topk = eng.sim_topk(qf, gallery.float(), K) if w["bf16_gallery"] else eng.sim_topk(qf, gallery, K)
            torch.cuda.synchronize()
            gallery = gallery_raw                                                       # plain tensor from here on (slicing, .cpu())
            n_cpu = gallery.shape[0] if gallery.shape[0] <= 200_000 else 200_000      # bound the CPU matmul on the 1M-row config
            if n_cpu != gallery.shape[0]:
                gpu_topk = eng.sim_topk(qf, gallery[:n_cpu].float(), K)
            extra_topk = {}
            if not w["bf16_gallery"]:
                pipe.set_precision("f32x3")
                rf3 = eng.encode_image(im)
                tg3, ts3 = eng.encode_text(tk)
                extra_topk["f32x3"] = eng.sim_topk(eng.dvr_fuse(rf3, lc, tg3, ts3), gallery[:n_cpu], K)
                torch.cuda.synchronize()
                pipe.set_precision("fp32")
            gal_cpu = gallery[:n_cpu].cpu()
            # FERN_BENCH_OVERLAP_CHILDREN=1: start the c3 / c4 / c5 child runs here, beside the CPU-oracle leg (this process is done with the GPU):
            # 59 -> 47 s for the default command.  Off by default: on one box, alternating, the overlapped c4 child read 2 928 / 3 117 queries/s
            # against 3 111 / 3 111 after the leg, and the CPU figure itself 16.3 / 19.1 against 22.7 / 19.9 -- the legs disturb each other.
            if os.environ.get("FERN_BENCH_OVERLAP_CHILDREN"):
                children = start_children()
            result["cpu_baseline"] = cpu_baseline(clip_sd, fusion_sd, cfg, w, im, tk, lc, gal_cpu, args.cpu_sample, gpu_topk, extra_topk=extra_topk,
                                                  all_cores_leg=args.cpu_all_cores)
            if children is not None:
                result["cpu_baseline"]["host_shared_with"] = ("the c3 / c4 / c5 child runs of this script (GPU-bound, one busy host thread each + their start-up) ran "
                                                              "on the GPU while the host timed this leg on " + str(result["cpu_baseline"].get("cores")) + " cores")
            gap = result["cpu_baseline"]["parity_vs_hip"]["max_oracle_score_gap_at_mismatching_positions"]
            if gap > 2e-6 and not w["bf16_gallery"]:
                raise SystemExit(f"bench: the HIP top-{K} differs from the CPU oracle's beyond near-ties (oracle score gap {gap:.3e} > 2e-6)")
        stamp("cpu_baseline_done")
        if children is None:
            children = start_children()
        if children is not None:
            children[0].join()
            result["other_configs"] = children[1]["r"]
        stamp("end")
        result["timing_s"] = dict(_STAMPS)
        result["full_record"] = os.path.basename(args.full_record) + " (+ stderr)"
        # The FULL record (every leg with its notes, the tile table, per-config child records) goes to a side file and to stderr; the
        # LAST stdout line -- the one the driver parses -- is its compact form (< 4 KB: contract keys, roofline, cpu_baseline, one number
        # per extra leg).  Round 5's single 24.6 KB line came back unparsed.
        try:
            with open(args.full_record, "w") as f:
                json.dump(result, f)
        except OSError as e:
            print(f"[bench] could not write {args.full_record}: {e}", file=sys.stderr)
        print("[bench full record] " + json.dumps(result), file=sys.stderr, flush=True)
        print(json.dumps(compact_record(result)), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

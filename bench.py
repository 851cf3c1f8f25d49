#!/usr/bin/env python
"""Headline benchmark: Mpixels/s of the fused grain -> 33^3 LUT -> colour match -> unsharp chain at 4K.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]     # N=1: plain python; N>1: launched by torchrun

A plain run sets up, warms up, times the K steps of the headline leg, writes its outputs when --dump-outputs is given, and prints
the line.  Everything else described below -- the output check, the fast colour-match policy, the timing of the reference-frame
statistics alone, the live PMC passes, the `configs` legs, the device-resident graph leg, the host-fed rates, the CPU baseline, the
fp64 statistics leg at N > 1 and the shader-clock sampling -- runs only with --full (the --no-* options still switch parts of it off).

`--dump-outputs DIR` writes what the timed steps left in rank 0's output batch after the last step, as float32 .npy files (~22 MB in
all): `output_sample` = the elements at a fixed, seeded set of 2^22 flat indices of the whole batch, `output_first_rows` /
`output_last_rows` = the first / last 64 rows of the first / last frame.  Inputs are seeded, so equal arguments give equal inputs.

Workload (BASELINE.json metric / configs[4] per-GPU shard): every rank holds `--frames` (default 256) synthetic
4K fp32 RGB frames resident in HBM (generated on device, never touched by the host), chain = Fast Film Grain
(I=0.04, s=0.5, one torch.randn draw per 4 frames) -> 3D LUT 33^3 (strength 10) -> Color Match to a 4K
reference frame (k=1) -> Fast Unsharp (0.5, edge-replicate).  A step = one pass of that chain over the rank's
batch: reference-frame statistics, the statistics pass over the batch, and the fused apply pass.  Weak scaling:
per-GPU work is fixed, value = all ranks' pixels / max time.

Prints ONE JSON line on rank 0.  `roofline` is for the dominant kernel of the step, timed with HIP events on the stream
it is launched on: the contract's HBM figures plus the unit that actually binds it (`bound`, `valu_busy_frac`;
`issue` has the terms).  `configs` (N = 1) holds the other single-GPU BASELINE configs as legs of the same run, each timed
the way the headline is, on both synthetic pixel distributions: chain3_4k x256 (configs[2]), grain_lut_1080p x128
(configs[1]), colormatch_4k x512 (configs[3]), and the headline on video-like pixels -- with ms_per_step, Mpixels/s, the
dominant kernel, its HBM and VALU-busy fractions and `verified` (first / last RNG chunk against the oracle after the timed
steps).  `cpu_baseline` times the reference's own node classes on the host cores where the reference checkout exists (the
build container: kind "reference"), otherwise the oracle port of them (kind "port"), on a bounded sample, on rank 0 at any N.

`--gpus N` with N > 1 and no torchrun environment re-executes itself under `python -m torch.distributed.run` (one rank
per GPU, RCCL); it fails loudly when fewer than N GPUs are visible.  At N > 1 the line carries a second timed leg,
`fp64_stats_leg`: the same chain with the fp64 statistics policy, whose reference-frame statistics are reduced over rows
split across the ranks and merged by the RCCL all-reduce inside every timed step (the collective configs[4] names; the default
device policy evaluates torch's own reduction over the whole reference frame on every rank and needs none).  Colour-match
arithmetic: the default "device" policy (bit-equal to torch-ROCm's element-wise ops); the "fast" policy is
timed next to it and reported under `fast_variant`, never as `value`.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CM_BATCH = 1                    # ColorMatchToReference's batch_size widget default: frames per statistics call of the reference
HBM_PEAK_GBS = 8000.0           # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s achievable by a copy kernel
WORKLOADS = {
    # name: (H, W, stages)
    "chain4_4k": (2160, 3840, ("grain", "lut", "colormatch", "sharpen")),      # headline (configs[4] per-GPU shard)
    "chain3_4k": (2160, 3840, ("grain", "lut", "sharpen")),                    # configs[2]
    "grain_lut_1080p": (1080, 1920, ("grain", "lut")),                         # configs[1]
    "colormatch_4k": (2160, 3840, ("colormatch",)),                            # configs[3]
}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=None, help="frames per GPU (default: BASELINE's 256; 128 for the 1080p workload, 512 for colour match alone)")
    ap.add_argument("--workload", default="chain4_4k", choices=sorted(WORKLOADS))
    ap.add_argument("--dist", default="uniform", choices=["uniform", "video"], help="synthetic pixel distribution")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=2, help="4K frames of the bounded CPU-baseline sample (x4 at 1080p)")
    ap.add_argument("--no-fast-variant", action="store_true", help="skip the extra timing of the fast colour-match policy")
    ap.add_argument("--sync-ref", action="store_true", help="reference-frame statistics on the main stream in front of pass 1 (A/B of the side-stream form)")
    ap.add_argument("--no-live-traffic", action="store_true", help="do not run the two rocprofv3 --pmc passes for roofline.traffic (use profiles/)")
    ap.add_argument("--no-verify", action="store_true", help="skip the output check after the timed region (first and last RNG chunk of rank 0 against "
                                                             "the stand-alone operators and the device oracle)")
    ap.add_argument("--digest", action="store_true", help="add the SHA-256 of every rank's output (per RNG chunk) to the line: equal frame ranges of "
                                                          "runs with different GPU counts must give equal digests")
    ap.add_argument("--no-host-fed", action="store_true", help="skip the host-fed (CPU tensors in and out, PCIe inclusive) node rates of the line's `host_fed` key")
    ap.add_argument("--same-data", action="store_true", help="frames are a function of their ABSOLUTE index in the job (rank r holds frames "
                                                             "[r*frames, (r+1)*frames) of one job-wide batch), so that runs with different GPU counts process "
                                                             "the same data; default: an independent batch per rank")
    ap.add_argument("--cm-stats", default=None, choices=["device", "fp64"], help="colour statistics of the headline leg (default: device)")
    ap.add_argument("--no-configs", action="store_true", help="skip the `configs` legs (the other single-GPU BASELINE configs, both pixel distributions; N = 1, headline "
                                                              "workload only)")
    ap.add_argument("--no-fp64-leg", action="store_true", help="N > 1: skip the second headline leg with the fp64 statistics policy (the one whose reference-frame "
                                                               "statistics cross the RCCL all-reduce inside the timed steps)")
    ap.add_argument("--full", action="store_true", help="also run every check and measurement beyond the headline figure (see the module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write rank 0's output of the last timed step to DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def self_launch(args):
    """`python bench.py --gpus N` outside torchrun: run `torch.distributed.run --nproc-per-node N bench.py ...` as a child process and exit
    with its status (a child, not exec: this process has already opened the GPU to count the devices)."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    n_vis = torch.cuda.device_count()
    if n_vis < args.gpus and os.environ.get("VRGDG_DIST_BACKEND", "nccl") == "nccl":
        sys.stderr.write(f"bench.py: --gpus {args.gpus} requested but only {n_vis} GPU(s) are visible to PyTorch-ROCm; "
                         "refusing to print a line for fewer GPUs than asked for\n")
        raise SystemExit(2)
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    import subprocess
    rc = subprocess.run(cmd, env=env).returncode
    raise SystemExit(128 - rc if rc < 0 else rc)        # killed by signal s: the shell's status 128 + s (SIGABRT 134, SIGSEGV 139)


def make_frames(n, H, W, dev, seed, dist, first_frame=None):
    """Synthetic frames generated on the device.  uniform: iid U[0,1) (worst case for LUT gathers);
    video: smooth low-frequency field + N(0, 0.02) texture, clamped (LUT-coherent like real footage).
    `first_frame` (--same-data): frame i is drawn from a generator seeded by its absolute index first_frame + i."""
    g = torch.Generator(device=dev).manual_seed(seed)
    if first_frame is not None:
        x = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev)
        for i in range(n):
            x[i] = make_frames(1, H, W, dev, seed * 1000003 + first_frame + i, dist)[0]
        return x
    if dist == "uniform":
        x = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev)
        for i in range(0, n, 16):
            x[i:i + 16].copy_(torch.rand((min(16, n - i), H, W, 3), generator=g, device=dev))
        return x
    yy = torch.linspace(0, 1, H, device=dev).view(1, H, 1, 1)
    xx = torch.linspace(0, 1, W, device=dev).view(1, 1, W, 1)
    x = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev)
    for i in range(n):
        ph = torch.rand((1, 1, 1, 3), generator=g, device=dev) * 6.28
        fr = 0.5 + 0.25 * torch.sin(6.0 * xx + ph) * torch.cos(4.0 * yy + 0.5 * ph) + 0.15 * torch.sin(9.0 * yy - ph)
        fr = fr + 0.02 * torch.randn((1, H, W, 3), generator=g, device=dev)
        x[i] = fr.clamp_(0, 1)[0]
    return x


def _profile_json(*names):
    """first of the committed PMC summaries that exists (newest round first)"""
    for n in names:
        path = os.path.join(ROOT, "profiles", n)
        if os.path.exists(path):
            with open(path) as fh:
                return json.load(fh), n
    raise FileNotFoundError(names[0])


#: pass of a workload -> substrings that name its kernel in a rocprofv3 trace (first match wins per kernel name)
PASS_KERNELS = {
    ("chain4_4k", "stats"): ("k_produce_lab<3",),
    ("chain4_4k", "apply"): ("k_apply_march<",),
    ("chain4_4k", "tstats"): ("k_tstats_frame<false, 1>",),
    ("chain3_4k", "apply"): ("k_chain_march<3, true",),
    ("grain_lut_1080p", "apply"): ("k_chain_march<3, false", "k_chain_pointwise<3"),      # (the march from ~10,000 strip jobs on: csrc/vrg_chain.hip)
    ("colormatch_4k", "stats"): ("k_lab_partials<0, true>",),
    ("colormatch_4k", "apply"): ("k_chain_pointwise4<20",),
    ("colormatch_4k", "tstats"): ("k_tstats_frame<false, 1>",),
}
SIMD_CYCLES_PER_S = 256 * 4 * 2.4e9          # 1,024 SIMDs at the 2.4 GHz the PMC runs report (GRBM_GUI_ACTIVE / time)


def live_traffic(timeout_s=150):
    """HBM bytes, VALU lane-instructions and VALU-busy cycles per pixel of every kernel of the bench's workloads from the PMC counters
    ON THIS BOX: three extra `rocprofv3 --kernel-trace --pmc` runs (FETCH_SIZE; WRITE_SIZE; the SQ set -- separate passes, as
    MI355X_MICROARCH.md prescribes) of tools/prof_driver.py, which executes the same kernels on 16 x 4K frames in its own process
    (rocprofv3 wraps a process, so it cannot observe this one).  FETCH_SIZE is doubled (the gfx950 under-count for wide coalesced
    reads; calibrated on k_lut3d's known 12 B/px in the same run), both counters are in KB; the SQ_* counters count wave64
    instructions / quad-cycles summed over the chip.  Returns {(workload, pass): {...}, "calibration_k_lut3d": {...}} or raises."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if not exe:
        raise RuntimeError("rocprofv3 not on PATH")
    tmp = tempfile.mkdtemp(prefix="vrg_traffic_")
    per_px = {}
    px = 16 * 2160 * 3840
    sq = ("SQ_INSTS_VALU", "SQ_INSTS_VALU_TRANS_F32", "SQ_INSTS_VALU_INT64", "SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES", "SQ_WAIT_INST_ANY", "SQ_WAIT_ANY")
    try:
        for counters in (("FETCH_SIZE",), ("WRITE_SIZE",), sq):
            out = os.path.join(tmp, counters[0])
            env = dict(os.environ, TMPDIR="/tmp", VRGDG_SELFCHECK="0")      # (the first-use self-check would launch the same kernels on tiny frames)
            for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
                env.pop(k, None)
            subprocess.run([exe, "--kernel-trace", "--pmc", *counters, "--output-format", "csv", "-d", out, "-o", "p", "--",
                            sys.executable, os.path.join(ROOT, "tools", "prof_driver.py"), "traffic"],
                           cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, check=True)
            for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                with open(f) as fh:
                    for r in csv.DictReader(fh):
                        if "vrg" in r["Kernel_Name"] and r["Counter_Name"] in counters:
                            # FETCH_SIZE / WRITE_SIZE count KB; SQ_INSTS_* wave64 instructions (x64 lanes); the others quad-cycles (x4)
                            c = r["Counter_Name"]
                            scale = 1024.0 if not c.startswith("SQ_") else (64.0 if c.startswith("SQ_INSTS") else 4.0)
                            per_px.setdefault(r["Kernel_Name"], {}).setdefault(c, []).append(float(r["Counter_Value"]) * scale / px)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    def summary(substrings, runs=1):
        # tools/prof_driver.py runs every workload ONCE: a kernel's figure per pixel is the SUM over its launches (pass 1 of the colour match
        # alone is launched per group of frames), divided by the number of driver workloads that launch it (`runs`: the whole-frame
        # reductions serve both the headline chain and the colour match alone)
        names = [k for k in per_px if any(s in k for s in substrings)]
        def avg(c, mult=1.0):
            return sum(sum(per_px[k][c]) * mult for k in names if c in per_px[k]) / runs
        rd, wr = avg("FETCH_SIZE", 2.0), avg("WRITE_SIZE")
        busy, wave = avg("SQ_ACTIVE_INST_VALU"), avg("SQ_WAVE_CYCLES")
        return {"kernels": sorted(n.split("(")[0][:80] for n in names), "read": round(rd, 2), "written": round(wr, 2), "total": round(rd + wr, 2),
                "valu_lane_instr": round(avg("SQ_INSTS_VALU"), 1), "valu_trans": round(avg("SQ_INSTS_VALU_TRANS_F32"), 1),
                "valu_int64": round(avg("SQ_INSTS_VALU_INT64"), 1),
                "valu_busy_simd_cycles": round(busy, 3),                    # SIMD-cycles per pixel with a VALU instruction executing
                "wave_cycles": round(wave, 3), "wait_issue_share": round(avg("SQ_WAIT_INST_ANY") / wave, 3) if wave else None,
                "wait_memory_share": round(avg("SQ_WAIT_ANY") / wave, 3) if wave else None}
    shared = {("chain4_4k", "tstats"), ("colormatch_4k", "tstats")}
    res = {key: summary(subs, 2 if key in shared else 1) for key, subs in PASS_KERNELS.items()}
    res["calibration_k_lut3d"] = summary(("k_lut3d",))
    if not res["calibration_k_lut3d"]["total"]:
        raise RuntimeError("no counters collected")
    return res


def committed_pmc():
    """{(workload, pass): {...}} from the newest committed profiles/rNN_pmc_bench_kernels.json (written by tools/collect_bench_pmc.py from a
    live_traffic() run on a GPU box), or {} -- what the legs fall back to when the live passes are switched off or fail."""
    for n in ("r06_pmc_bench_kernels.json", "r05_pmc_bench_kernels.json"):
        path = os.path.join(ROOT, "profiles", n)
        if os.path.exists(path):
            with open(path) as fh:
                raw = json.load(fh)
            return {(tuple(k.split("|")) if "|" in k else k): v for k, v in raw.get("passes", {}).items()}, n
    return {}, None


def _median_time(fn, warmup=1, reps=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def cpu_baseline(stages, cpu_frames, H, W, lut_cpu, per_node=False):
    """The chain on the host cores over a bounded sample: warm-up 1, median of 3.  kind "reference": the reference's own
    node classes (FastFilmGrain / VRGDG_LUTS / ColorMatchToReference / FastUnsharpSharpen, stub-loaded by
    oracle/reference_loader.py; kornia's Lab transforms are the restated ones) -- only where the reference checkout exists,
    i.e. not on the GPU box; kind "port": oracle/restated.py, the op-for-op port of them."""
    from oracle import reference_loader as RL
    g = torch.Generator().manual_seed(7)
    x = torch.rand((cpu_frames, H, W, 3), generator=g)
    ref = torch.rand((1, H, W, 3), generator=g)
    mpix = cpu_frames * H * W / 1e6
    if RL.reference_available():
        nodes, iv = RL.load_nodes(), RL.load_iv_adjustments()
        lut_name = "Vintage Color.cube"                      # the reference's own 33^3 asset
        fns = {"grain": lambda y: nodes.FastFilmGrain().apply_grain(y, 0.04, 0.5, 4)[0],
               "lut": lambda y: iv.VRGDG_LUTS().apply_lut(y, lut_name, "cpu", 10.0)[0],
               "colormatch": lambda y: nodes.ColorMatchToReference().match_color(y, ref, 1.0, 1)[0],
               "sharpen": lambda y: nodes.FastUnsharpSharpen().apply_unsharp(y, 0.5, False)[0]}
        kind, what = "reference", "the reference's node classes (oracle/reference_loader.py; kornia Lab transforms restated)"
    else:
        from oracle import restated as R
        fns = {"grain": lambda y: R.fast_film_grain(y, 0.04, 0.5, 4),
               "lut": lambda y: R.apply_lut_with_strength(y, lut_cpu, 10.0),
               "colormatch": lambda y: R.color_match(y, ref, 1.0, 1),
               "sharpen": lambda y: R.unsharp(y, 0.5, False)}
        kind, what = "port", ("oracle/restated.py (op-for-op port of the reference's eager torch / numpy ops; BIT-EQUAL to the reference's own node classes "
                              "wherever those can run -- tests/test_oracle_golden.py::test_restatement_against_live_reference_random_shapes and the fixtures "
                              "under tests/golden/ produced by them; the reference itself cannot travel to this box -- it was timed on the 8-vCPU build box: "
                              "profiles/r04_cpu_baseline_buildbox.json)")

    def chain():
        y = x
        for st in ("grain", "lut", "colormatch", "sharpen"):
            if st in stages:
                y = fns[st](y)
        return y

    # torch's default on a 256-thread host is 128 intra-op threads: on 2 frames that mostly measures its threading overhead, so a
    # one-run probe picks the better of the default and 32 threads before the timed runs (`cores` = the count actually used)
    default_threads = torch.get_num_threads()
    probe = {}
    for nt in sorted({default_threads, min(32, default_threads)}):
        torch.set_num_threads(nt)
        probe[nt] = _median_time(chain, warmup=1 if not probe else 0, reps=1)
    best = min(probe, key=probe.get)
    torch.set_num_threads(best)
    dt = _median_time(chain, warmup=0)
    out = {"value": round(mpix / dt, 2), "unit": "Mpixels/s", "cores": torch.get_num_threads(), "kind": kind,
           "thread_probe_s": {str(k): round(v, 2) for k, v in probe.items()},
           "sample": f"{cpu_frames} frames {W}x{H}, chain {'+'.join(stages)} via {what}; warm-up 1, median of 3 = {dt:.2f} s; "
                     f"os.cpu_count()={os.cpu_count()}, torch.get_num_threads()={torch.get_num_threads()} (numpy unsharp is single-threaded)"}
    if per_node:
        # each node on its own over the same sample (one warm-up, median of 3): what BASELINE.md section 3 asks to see beside the chain
        out["per_node"] = {st: {"value": round(mpix / _median_time(lambda st=st: fns[st](x)), 2), "unit": "Mpixels/s"} for st in stages}
    return out


def verify_output(ops, x, out, ref, lut, lut_cpu, stages, geom_stream, rank, frames, chunk, dev, cm_stats):
    """Outside the timed region, on rank 0's own output: the first and the last RNG chunk of the rank's batch (at 4K with chunk 4 the
    Philox quarters of a chunk span 11.4 rows and their sibling runs cross frame boundaries inside every chunk) are re-derived
      (a) with the stand-alone operators of this library, one after the other (film_grain -> lut3d -> color_match -> stencil3x3), and
      (b) with the oracle composition (oracle/chain_oracle.py: torch.randn on the device, the CPU restatements pinned to the reference's
          fixtures for grain / LUT / unsharp, the restated colour match evaluated by torch on the device) -- the checker, never timed,
    and compared bit for bit with what the timed steps left in `out`.  (b) holds with the device statistics; with fp64 statistics the
    oracle differs by the statistics band and only (a) is asserted."""
    from oracle import chain_oracle as CO          # checker only (like the cpu_baseline leg)
    res = {"frames_checked": [], "vs_standalone_operators": True, "vs_device_oracle": None, "max_abs_vs_oracle": 0.0}
    chunks = sorted({0, frames // chunk - 1}) if "grain" in stages else [0, max(frames // chunk - 1, 0)]
    ref_ms = ops.reference_stats(ref, cm_stats=cm_stats) if "colormatch" in stages else None
    for c in sorted(set(chunks)):
        f0, f1 = c * chunk, min(frames, (c + 1) * chunk)
        xs = x[f0:f1]
        y = xs
        if "grain" in stages:
            plan = ops.NoisePlan(chunk, geom_stream, chunk0=rank * (frames // chunk) + c)
            y = ops.film_grain(y, 0.04, 0.5, chunk_frames=chunk, plans=(plan, None, 1))
        if "lut" in stages:
            y = ops.lut3d(y, lut, 10.0)
        if "colormatch" in stages:
            y = ops.color_match(y, None, 1.0, ref_ms=ref_ms, cm_chunk=CM_BATCH, cm_stats=cm_stats)
        if "sharpen" in stages:
            y = ops.stencil3x3(y, "unsharp", 0.5, False)
        got = out[f0:f1]
        res["vs_standalone_operators"] = bool(res["vs_standalone_operators"] and torch.equal(got, y))
        want = CO.headline_chain(xs.cpu(), dev, stages=stages, stream=geom_stream, chunk0=rank * (frames // chunk) + c, chunk_frames=chunk,
                                 lut_cpu=lut_cpu, reference_dev=ref, cm_batch=CM_BATCH)
        same = torch.equal(got.cpu(), want)
        res["max_abs_vs_oracle"] = max(res["max_abs_vs_oracle"], float((got.cpu() - want).abs().max()))
        res["vs_device_oracle"] = same if res["vs_device_oracle"] is None else (res["vs_device_oracle"] and same)
        res["frames_checked"].append([f0, f1])
        del y, want
    oracle_must_hold = "colormatch" not in stages or (cm_stats or "device") == "device"
    res["verified"] = bool(res["vs_standalone_operators"] and (res["vs_device_oracle"] or not oracle_must_hold))
    return res


def output_digests(out, chunk):
    """SHA-256 per RNG chunk of a rank's output (bytes of the fp32 frames): independent of how many ranks share the job."""
    import hashlib
    return [hashlib.sha256(out[f:f + chunk].cpu().numpy().tobytes()).hexdigest() for f in range(0, out.shape[0], chunk)]


DUMP_SAMPLE = 1 << 22           # elements of the seeded sample (16 MB in fp32): a 4K batch is far over the 64 MB a dump may hold
DUMP_ROWS = 64


def dump_outputs(out, dump_dir):
    """--dump-outputs: a fixed, seeded sample of the elements of the whole batch `out` (the indices depend on its size only) and the first /
    last DUMP_ROWS rows of its first / last frame, as float32 .npy files."""
    import numpy as np
    os.makedirs(dump_dir, exist_ok=True)
    flat = out.view(-1)
    if flat.numel() > DUMP_SAMPLE:
        idx = torch.randint(0, flat.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(20261016)).sort().values
        flat = flat[idx.to(out.device)]
    arrays = {"output_sample": flat, "output_first_rows": out[0, :DUMP_ROWS], "output_last_rows": out[-1, -DUMP_ROWS:]}
    for name, a in arrays.items():
        np.save(os.path.join(dump_dir, name + ".npy"), a.to(torch.float32).cpu().numpy())


class Ctx:
    """What every leg needs: the package modules, the rank geometry, the LUT."""
    pass


class ClockSampler:
    """Shader clock and socket power DURING a timed region, from the amdgpu hwmon files (freq1_input = sclk in Hz, power1_input /
    power1_average in microwatts), polled every 50 ms by a thread.  The box exposes the hwmon directories of every GPU of its node; the
    one this process drives is the one whose power rises, so the summary is taken from the card with the highest mean power.  Round 6
    (VERDICT round 5, weak 6): the chip does NOT run these kernels at the 2.4 GHz the guide's peaks assume -- it is power-limited (~1.3-1.4 kW)
    to 1.85-2.3 GHz depending on the kernel (profiles/r06_sclk_power_per_kernel_sysfs.json, r06_clock_per_kernel_grbm.txt) -- so every
    cycle-based fraction of this line is stated against the MEASURED v_fma_f32 rate, and the clock of each leg is reported beside it."""

    def __init__(self):
        import glob
        self.cards = {}
        for hw in glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*"):
            f = os.path.join(hw, "freq1_input")
            pw = next((os.path.join(hw, n) for n in ("power1_input", "power1_average") if os.path.exists(os.path.join(hw, n))), None)
            if os.path.exists(f) and pw:
                self.cards[hw] = (f, pw)
        self.rows, self._stop, self._th = [], None, None

    def __enter__(self):
        import threading
        self.rows = []
        if not self.cards:
            return self
        self._stop = threading.Event()

        def poll():
            while not self._stop.is_set():
                r = {}
                for hw, (f, pw) in self.cards.items():
                    try:
                        r[hw] = (int(open(f).read()), int(open(pw).read()))
                    except (OSError, ValueError):
                        pass
                self.rows.append(r)
                self._stop.wait(0.05)
        self._th = threading.Thread(target=poll, daemon=True)
        self._th.start()
        return self

    def __exit__(self, *exc):
        if self._th is not None:
            self._stop.set()
            self._th.join()
        return False

    def summary(self):
        if not self.rows or not self.cards:
            return None
        mean_p = {hw: sum(r[hw][1] for r in self.rows if hw in r) / max(sum(1 for r in self.rows if hw in r), 1) for hw in self.cards}
        hw = max(mean_p, key=mean_p.get)
        clk = sorted(r[hw][0] for r in self.rows if hw in r)
        if not clk:
            return None
        return {"sclk_mhz_median": round(clk[len(clk) // 2] / 1e6), "sclk_mhz_min": round(clk[0] / 1e6), "sclk_mhz_max": round(clk[-1] / 1e6),
                "socket_power_w_mean": round(mean_p[hw] / 1e6), "samples": len(clk), "source": "amdgpu hwmon freq1_input / power1_input, 50 ms poll"}


def _kernel_name(stages, which):
    if which == "stats":
        return ("k_produce_lab, Lab-only form (grain->LUT->Lab pass 1: shared Philox, stores the Lab image; the statistics are reduced from it by "
                "k_tstats_frame)" if "grain" in stages else
                "k_lab_partials, Lab-only form (rgb->Lab pass 1, stores the Lab image; the statistics are reduced from it by k_tstats_frame)")
    if which == "tstats":
        return "k_tstats_frame (torch's mean / Welford reductions replayed over the stored Lab image)"
    if "colormatch" in stages:
        return "k_apply_march<COLORMATCH|FROM_LAB> (match -> Lab->RGB -> 3x3 sharpen, register-resident wave march)"
    if "sharpen" in stages and "grain" in stages:
        return "k_chain_march (fused grain -> LUT -> sharpen, register-resident wave march)"
    if "grain" in stages and "lut" in stages:
        return "k_chain_march without a stencil (large launches) / k_chain_pointwise (fused grain -> LUT)"
    return "k_chain_tile / k_chain_pointwise (fused apply pass)"


def kernel_path(ops, dev, stages):
    """Which kernels the automatic choice really launched in this process: the wave-march kernels with their
    hand-counted LDS-DMA waits, or -- where ops.toolchain_selfcheck found them disagreeing with the tile kernels on this toolchain -- the
    LDS-tile / point-wise kernels (same bits, 10-25 % slower)."""
    st = ops.toolchain_status(dev)
    march = bool(st.get("march_equals_tile_kernels"))
    if "colormatch" in stages:
        ks = ["k_produce_lab" if "grain" in stages else "k_lab_partials (Lab-only form)", "k_tstats_frame", "k_apply_march" if march else "k_chain_tile<COLORMATCH|FROM_LAB>"]
    elif "sharpen" in stages or ("grain" in stages and "lut" in stages):
        ks = ["k_chain_march" if march else "k_chain_tile / k_chain_pointwise"]
    else:
        ks = ["k_chain_pointwise"]
    return {"kernels": ks, "fallback_to_tile_kernels": not march, "toolchain_selfcheck": st}


ALGO_BPP = {"stats": 12, "apply": 24, "tstats": 12}         # SURVEY.md section 8d; tstats re-reads the Lab image (12 B/px)


def run_workload(C, args, workload, pixel_dist, frames, steps, warmup, *, cm_stats=None, verify=True, digest=False, fast_variant=False,
                 time_reference_stats=False, cube_name=None, dump_dir=None):
    """One leg: `frames` synthetic frames of `workload` resident in HBM on every rank, `warmup` untimed + `steps` timed steps bracketed
    by barrier + synchronize, MAX over ranks; the shader clock is sampled during them with --full.  Returns the measurements and frees
    its buffers."""
    ops, sharding, dist = C.ops, C.sharding, C.dist
    rank, world, dev = C.rank, C.world, C.dev
    H, W, stages = WORKLOADS[workload]
    chunk = 4
    lut, lut_cpu = C.lut, C.lut_cpu
    if cube_name is not None:             # a leg with another cube size (25^3: 8 of the reference's 12 cubes; 17^3: the table lives in LDS)
        lut_cpu = C.cube.parse_cube_file(os.path.join(C.luts_dir, cube_name))
        lut = ops.upload_lut(lut_cpu, dev)
    x = make_frames(frames, H, W, dev, 1234 + (0 if args.same_data else rank), pixel_dist, first_frame=rank * frames if args.same_data else None)
    out = torch.empty_like(x)
    lab_ws = torch.empty_like(x) if "colormatch" in stages else None      # Lab image between the two colour-match passes
    ref = make_frames(1, H, W, dev, 4321, pixel_dist)          # same reference frame on every rank
    fe = H * W * 3
    # one job-wide generator state: rank r takes chunks [r*frames/chunk, ...) of the same stream, so the result
    # does not depend on the number of GPUs
    geom_stream = None
    if "grain" in stages:
        gen = torch.Generator(device=dev).manual_seed(42)
        geom_stream = ops.rng.reserve(chunk * fe, world * frames // chunk, dev, gen)
    ref_events = []

    def step(kernel_events=None, cm_math=None, cm_stats=cm_stats):
        ref_ms = ref_ev = None
        if "colormatch" in stages:
            if ops._cm_stats(cm_stats, cm_math, dev) == "device":
                # device statistics = torch's own reduction over the WHOLE reference frame: every rank evaluates it (no exchange), on
                # the side stream -- only the apply pass needs it, pass 1 of the batch runs meanwhile
                if args.sync_ref:
                    ref_ms = ops.reference_stats(ref, cm_math, step_frames=frames)
                else:
                    ref_ms, ref_ev = ops.reference_stats_async(ref, cm_math, step_frames=frames)
            else:
                # fp64 (n, mean, M2): rows split across the ranks + all-reduce over RCCL (BASELINE configs[4])
                if kernel_events is not None:
                    r0, r1 = ops.HipEvent(), ops.HipEvent()
                    r0.record()
                ref_ms = sharding.reference_stats_sharded(ref, rank, world, cm_math=cm_math)      # fp64 triples, RCCL all-reduce
                if kernel_events is not None:
                    r1.record()
                    ref_events.append((r0, r1))
        plans = None
        if geom_stream is not None:
            plans = (ops.NoisePlan(chunk, geom_stream, chunk0=rank * (frames // chunk)), None, frames // chunk)
        spec = ops.ChainSpec(grain=(0.04, 0.5, chunk) if "grain" in stages else None,
                             lut=(lut, 10.0) if "lut" in stages else None,
                             colormatch=(ref_ms, 1.0) if "colormatch" in stages else None,
                             sharpen=("unsharp", 0.5, False) if "sharpen" in stages else None, cm_math=cm_math, cm_chunk=CM_BATCH,
                             cm_ref_event=ref_ev, cm_stats=(cm_stats if cm_math is None else None))
        ops.fused_chain(x, spec, plans=plans, out=out, kernel_events=kernel_events, lab_workspace=lab_ws)

    def barrier():
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()

    clocks = {}

    def timed(**kw):
        for _ in range(warmup):
            step(**kw)
        barrier()
        ev = []
        cs = ClockSampler() if args.full else None
        with cs or contextlib.nullcontext():
            t0 = time.perf_counter()
            for _ in range(steps):
                step(ev, **kw)
            barrier()
            el = time.perf_counter() - t0
        clocks["last"] = cs.summary() if cs is not None and rank == 0 else None
        per_rank = [el / steps * 1e3]
        if dist.is_initialized():
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            every = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(every, t)
            per_rank = [round(float(v.item()) / steps * 1e3, 3) for v in every]
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, per_rank, ev

    elapsed, per_rank_ms, events = timed()
    R = {"clock": clocks.get("last"), "workload": workload, "dist": pixel_dist, "cube": cube_name, "frames": frames, "H": H, "W": W, "stages": stages, "chunk": chunk, "steps": steps, "warmup": warmup,
         "elapsed": elapsed, "per_rank_ms": per_rank_ms, "px_rank": frames * H * W, "cm_stats": cm_stats}
    # the timed steps' own output, written, checked and fingerprinted BEFORE anything else overwrites it (never inside the timed region)
    if dump_dir is not None and rank == 0:
        dump_outputs(out, dump_dir)
    R["verify"] = None
    if rank == 0 and verify:
        try:
            R["verify"] = verify_output(ops, x, out, ref, lut, lut_cpu, stages, geom_stream, rank, frames, chunk, dev, cm_stats)
        except Exception as exc:              # a checker problem must not lose the measurement; it is reported as unverified
            R["verify"] = {"verified": False, "error": f"{type(exc).__name__}: {exc}"}
    R["digests"] = None
    if digest:
        mine = output_digests(out, chunk)
        R["digests"] = [mine]
        if dist.is_initialized():
            R["digests"] = [None] * world
            dist.all_gather_object(R["digests"], mine)
    # the fast colour-match policy, same data, timed the same way (reported beside the headline, never as `value`)
    R["fast_variant"] = None
    if fast_variant and "colormatch" in stages:
        fel, _pr, _ev = timed(cm_math="fast", cm_stats=None)
        R["fast_variant"] = {"cm_math": "fast", "value": round(world * frames * H * W * steps / fel / 1e6, 1), "unit": "Mpixels/s",
                             "ms_per_step": round(fel / steps * 1e3, 3),
                             "cm_stats": "fp64 (reference-frame rows split across the ranks, merged by the RCCL all-reduce when N > 1)",
                             "note": "table-driven powers (<= 0.534 ulp) instead of ocml powf and fp64-accumulated statistics instead of torch's "
                                     "fp32 reductions: a few ulp from the reference, not bit-equal to it (DESIGN.md section 4)"}
    # per-pass device time from HIP events on the launch stream
    passes = {}
    for name, a, b, nf in events:
        passes.setdefault(name, []).append(a.elapsed_ms(b))
    R["pass_ms"] = {k: sum(v) / steps for k, v in passes.items()}          # per step (pieces of a step added up)
    R["launches_per_step"] = {k: len(v) // max(steps, 1) for k, v in passes.items()}
    # reference-frame statistics: the device form is overlapped with pass 1 in the step, so it is timed on its own here (3 runs, median);
    # the fp64 / all-reduce form was bracketed by events inside its steps
    R["ref_ms_per_step"] = R["ref_allreduce_ms"] = None
    if "colormatch" in stages and time_reference_stats:
        ts = []
        for _ in range(4):
            a, b = ops.HipEvent(), ops.HipEvent()
            a.record(); ops.reference_stats(ref, step_frames=frames); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_ms(b))
        R["ref_ms_per_step"] = round(sorted(ts[1:])[1], 4)
    if ref_events:
        R["ref_allreduce_ms"] = round(sum(a.elapsed_ms(b) for a, b in ref_events[-steps:]) / max(steps, 1), 4)
    del x, out, lab_ws, ref
    torch.cuda.empty_cache()
    return R


def graph_leg(C, args, frames, steps, warmup):
    """The headline workload driven through NODE_CLASS_MAPPINGS: FastFilmGrain -> VRGDG_LUTS -> ColorMatchToReference -> FastUnsharpSharpen called one
    after the other on device-resident 4K frames, ComfyUI's intermediate device on the GPU (`--gpu-only`; a stub of comfy.model_management says so
    for the duration of the leg).  The nodes defer and fuse (_devices.defer): the four calls record a recipe, the first use of the last result runs
    ONE fused chain into that result's tensor.  Timed like every leg (barrier + synchronize around `steps` graph executions); verified bit for bit
    against ops.fused_chain on the same generator state."""
    import types
    pack = sys.modules["comfyui_vrgamedevgirl_amd"]
    from comfyui_vrgamedevgirl_amd import _devices
    ops, dev = C.ops, C.dev
    H, W, _st = WORKLOADS["chain4_4k"]
    mm = types.ModuleType("comfy.model_management")
    mm.get_torch_device = lambda: dev
    mm.intermediate_device = lambda: dev
    comfy = types.ModuleType("comfy")
    comfy.model_management = mm
    saved = {k: sys.modules.get(k) for k in ("comfy", "comfy.model_management")}
    sys.modules["comfy"], sys.modules["comfy.model_management"] = comfy, mm
    try:
        import gc
        gc.collect()
        torch.cuda.empty_cache()            # the legs before this one held up to 200 GB: start from an unfragmented pool
        x = make_frames(frames, H, W, dev, 1234, "uniform")
        ref = make_frames(1, H, W, dev, 4321, "uniform")
        N = pack.NODE_CLASS_MAPPINGS
        call = lambda key, *a: getattr(N[key](), N[key].FUNCTION)(*a)[0]

        def graph():
            t = call("FastFilmGrain", x, 0.04, 0.5, 4)
            t = call("VRGDG_LUTS", t, "AMD_TealOrange_33.cube", "auto", 10.0)
            t = call("ColorMatchToReference", t, ref, 1.0, CM_BATCH)
            t = call("FastUnsharpSharpen", t, 0.5, False)
            return _devices.materialise(t)             # the first use of the result (what the consumer of the graph's output does)

        fused0 = _devices._LAZY.fused
        for _ in range(warmup):
            graph()
        torch.cuda.synchronize()
        with ClockSampler() as cs:
            t0 = time.perf_counter()
            for _ in range(steps):
                out = graph()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
        fused = (_devices._LAZY.fused - fused0) // max(steps + warmup, 1)
        torch.manual_seed(20260930)
        got = graph()
        torch.manual_seed(20260930)
        ref_ms = ops.reference_stats(ref, step_frames=frames)
        want = ops.fused_chain(x, ops.ChainSpec(grain=(0.04, 0.5, 4), lut=(C.lut, 10.0), colormatch=(ref_ms, 1.0), sharpen=("unsharp", 0.5, False), cm_chunk=CM_BATCH))
        same = bool(torch.equal(got, want)) and bool(got.is_cuda)
        ms = el / steps * 1e3
        res = {"what": "FastFilmGrain -> VRGDG_LUTS -> ColorMatchToReference -> FastUnsharpSharpen through NODE_CLASS_MAPPINGS, device-resident frames, intermediate "
                       "device = the GPU; the four calls are deferred and run as one fused chain at the first use of the last result (_devices.defer)",
               "frames": frames, "height": H, "width": W, "steps": steps, "warmup": warmup, "ms_per_graph": round(ms, 3),
               "Mpix_s": round(frames * H * W / ms / 1e3, 1), "nodes_fused_per_graph": int(fused), "bit_identical_to_ops_fused_chain": same,
               "clock_during_timed_steps": cs.summary()}
        del x, ref, out, got, want
        torch.cuda.empty_cache()
        return res
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


VALU_PEAK_T = 66.47       # T lane-instr/s: v_fma_f32 at 8 waves/SIMD over >= 17 ms launches on this chip (profiles/r02_valu_issue_rate_long.json; 78.6 by the clock)


def valu_fractions(c, rate_px_s):
    """Two readings of "how busy is the VALU" for a kernel with PMC record `c` running at `rate_px_s` pixels per second:
      valu_busy_frac            = class-weighted lane-instructions per second / the measured v_fma_f32 peak.  Weights = measured issue cost
                                  relative to a plain fp32 / integer op: transcendental 3.45x, 64-bit integer multiply-add 1.8x
                                  (profiles/r02_valu_issue_rate_long.json; v_pk_* and compare+select pairs, 1.8x / 1.65x, have no counter: not
                                  included, so this is a lower bound of the issue time);
      sq_active_inst_valu_x4    = SQ_ACTIVE_INST_VALU x 4 per pixel x the rate / (1,024 SIMDs x 2.4 GHz) -- rocprof's "VALUBusy" formula.  On
                                  gfx950 the counter advances ~1.02 per VALU wave-instruction whatever the instruction (4.88 for 4.76
                                  instructions per pixel in the march, 10.94 for 10.74 in pass 1), i.e. it counts instructions in quad-cycle
                                  clothing while a SIMD-32 issues a wave64 instruction in 2 cycles: the formula reads 128 % for pass 1 and
                                  222 % for rgb->Lab.  Reported for transparency; not a roofline."""
    ipp = c.get("valu_lane_instr")
    if not ipp:
        return None, None
    w = ipp + 2.45 * (c.get("valu_trans") or 0.0) + 0.8 * (c.get("valu_int64") or 0.0)
    busy = c.get("valu_busy_simd_cycles")
    return round(w * rate_px_s / 1e12 / VALU_PEAK_T, 4), (round(busy * rate_px_s / SIMD_CYCLES_PER_S, 4) if busy else None)


#: (workload, pass) -> the committed ISA price of that kernel's hot loop (tools/isa_cost.py over profiles/r06_valu_instruction_costs.json)
ISA_COST_PROFILES = {("chain4_4k", "stats"): "r06_isa_cost_produce_lab.json", ("chain4_4k", "apply"): "r06_isa_cost_apply_march.json",
                     ("chain3_4k", "apply"): "r06_isa_cost_march_chain3.json"}


def issue_cost_roofline(workload, which, c, rate_px_s):
    """The VALU roofline of THIS kernel's instruction mix (round 6).  gfx950 issues only part of its VALU at the 2-cycle rate (fp32 add / sub /
    mul / fma, xor / and / or / mov, add_u32); every DPP form, min / max / med3, conversion, compare and select takes 4.4 cycles, packed fp32
    4.6-5.1, v_mad_u64_u32 4.8, transcendentals 8.4 (tools/probe_valu_classes.py -> profiles/r06_valu_instruction_costs.json, cycles at the
    2.4 GHz the probe launches ran at).  The kernel's hot loop, priced opcode by opcode (tools/isa_cost.py), gives its mean issue units per
    VALU instruction; x the lane-instructions per pixel the PMC pass counted = issue units per pixel-lane; 1,024 SIMDs x 64 lanes x 2.4e9 units
    per second / that = the pixel rate at which the VALU issue ports are full.  `frac` = measured rate / that rate (it can pass 1.0 by the
    model's error: the probe's clock against the kernel's, hot loop against whole kernel)."""
    name = ISA_COST_PROFILES.get((workload, which))
    ipp = c.get("valu_lane_instr") if c else None
    if not name or not ipp or not rate_px_s:
        return None
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None
    with open(path) as fh:
        isa = json.load(fh)
    units = isa["issue_cycles"] / max(isa["valu"], 1)
    bound = 1024 * 64 * 2.4e9 / (ipp * units)
    return {"units_per_valu_instruction": round(units, 3), "lane_instr_per_px": round(ipp, 1), "issue_bound_Mpix_s": round(bound / 1e6, 1),
            "achieved_Mpix_s": round(rate_px_s / 1e6, 1), "frac": round(rate_px_s / bound, 4), "isa_profile": f"profiles/{name}",
            "by_class_share": {k: round(v / isa["issue_cycles"], 3) for k, v in sorted(isa["by_class"].items(), key=lambda kv: -kv[1]) if v}}


def leg_summary(R, world, pmc, pmc_src):
    """The compact record of a leg for the line's `configs` object: whole-leg rate, the dominant pass and its two roofline fractions --
    algorithmic bytes against 8 TB/s (`hbm_frac`) and class-weighted VALU issue against the measured peak (`valu_busy_frac`, see
    valu_fractions; instruction counts per pixel of that kernel from the PMC pass named in `pmc_source` x the pixel rate the pass reached
    here)."""
    stages, px = R["stages"], R["px_rank"]
    ms = R["elapsed"] / R["steps"] * 1e3
    bpp_chain = 36 if "colormatch" in stages else 24
    dom = max(R["pass_ms"], key=R["pass_ms"].get)
    dms = R["pass_ms"][dom]
    rate = px / (dms * 1e-3) if dms > 0 else 0.0
    c = pmc.get((R["workload"], dom), {}) if pmc else {}
    vfrac, x4 = valu_fractions(c, rate)
    out = {"workload": R["workload"], "pixels": f"synthetic-{R['dist']}", "frames": R["frames"], "height": R["H"], "width": R["W"], "stages": "+".join(stages),
           "steps": R["steps"], "warmup": R["warmup"], "ms_per_step": round(ms, 3), "Mpix_s": round(world * px / ms / 1e3, 1),
           "algorithmic_bytes_per_pixel": bpp_chain, "hbm_frac": round(px / (ms * 1e-3) * bpp_chain / (HBM_PEAK_GBS * 1e9), 4),
           "passes_ms": {k: round(v, 3) for k, v in R["pass_ms"].items()},
           "dominant_kernel": _kernel_name(stages, dom), "dominant_kernel_ms": round(dms, 3),
           "dominant_kernel_hbm_frac": round(ALGO_BPP[dom] * rate / 1e9 / HBM_PEAK_GBS, 4),
           "valu_busy_frac": vfrac, "sq_active_inst_valu_x4_frac": x4, "valu_lane_instr_per_px": c.get("valu_lane_instr") or None,
           "issue_cost_roofline": issue_cost_roofline(R["workload"], dom, c, rate),
           "wait_issue_share_of_wave_cycles": c.get("wait_issue_share"), "wait_memory_share_of_wave_cycles": c.get("wait_memory_share"),
           "hbm_bytes_per_px_measured": c.get("total") or None, "pmc_source": pmc_src if c else None,
           "clock_during_timed_steps": R.get("clock"),
           "verified": None if R["verify"] is None else bool(R["verify"].get("verified"))}
    if R["verify"] is not None and not R["verify"].get("verified"):
        out["verify"] = R["verify"]
    return out


def main():
    args = parse_args()
    self_launch(args)
    # stdout carries exactly one line, the JSON: everything else that writes to fd 1 while we run (RCCL prints a
    # version banner to stdout when a communicator is created) is sent to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    from __graft_entry__ import load_package
    load_package()
    from comfyui_vrgamedevgirl_amd import ops, sharding
    from comfyui_vrgamedevgirl_amd import VRGDG_IV_Adjustments as iv
    from comfyui_vrgamedevgirl_amd import cube
    import torch.distributed as dist

    # rank 0 checks its output against the oracle and times the CPU baseline AFTER the timed region while the other ranks wait at the
    # final barrier: the process group's timeout must cover that (a 4K chunk through the CPU oracle takes tens of seconds)
    rank, local, world = sharding.init_from_env(timeout_s=3600)
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world} (launch with torchrun --nproc-per-node {args.gpus}, or let "
                         "bench.py launch itself)")
    if world > 1:
        want_backend = os.environ.get("VRGDG_DIST_BACKEND", "nccl")      # gloo only for functional tests on a 1-GPU box
        if not dist.is_initialized() or dist.get_world_size() != world or dist.get_backend() != want_backend:
            raise SystemExit("bench.py: RCCL process group did not come up with the requested world size")
    C = Ctx()
    C.ops, C.sharding, C.dist, C.rank, C.world = ops, sharding, dist, rank, world
    C.dev = dev = torch.device("cuda", torch.cuda.current_device())
    C.lut_cpu = lut_cpu = cube.parse_cube_file(os.path.join(iv.LUTS_DIR, "AMD_TealOrange_33.cube"))
    C.lut = ops.upload_lut(lut_cpu, dev)
    C.cube, C.luts_dir = cube, iv.LUTS_DIR
    H, W, stages = WORKLOADS[args.workload]
    default_frames = {"grain_lut_1080p": 128, "colormatch_4k": 512}
    frames = args.frames or default_frames.get(args.workload, 256)      # BASELINE.json configs[1..4]

    full = args.full
    M = run_workload(C, args, args.workload, args.dist, frames, args.steps, args.warmup, cm_stats=args.cm_stats, verify=full and not args.no_verify,
                     digest=args.digest, fast_variant=full and not args.no_fast_variant, time_reference_stats=full, dump_dir=args.dump_outputs)
    # N > 1: a second headline leg whose reference-frame statistics are the fp64 (n, mean, M2) form -- rows split across the ranks, merged
    # by the RCCL all-reduce INSIDE the timed steps (BASELINE configs[4] names that collective; the default device policy needs none)
    fp64_leg = None
    if full and world > 1 and "colormatch" in stages and not args.no_fp64_leg and (args.cm_stats or "device") == "device":
        F64 = run_workload(C, args, args.workload, args.dist, frames, args.steps, args.warmup, cm_stats="fp64", verify=not args.no_verify)
        fp64_leg = {"cm_stats": "fp64 (reference-frame rows split across the ranks, (n, mean, M2) merged by two SUM all-reduces over RCCL inside every step)",
                    "value": round(world * F64["px_rank"] * args.steps / F64["elapsed"] / 1e6, 1), "unit": "Mpixels/s",
                    "ms_per_step": round(F64["elapsed"] / args.steps * 1e3, 3), "per_rank_ms_per_step": F64["per_rank_ms"],
                    "reference_stats_allreduce_ms_per_step": F64["ref_allreduce_ms"],
                    "verified": None if F64["verify"] is None else bool(F64["verify"].get("verified")),
                    "note": "arithmetic device-exact, statistics fp64-accumulated: within the statistics band of the reference (tens of ulp(1.0)), "
                            "not bit-equal to it; checked against the stand-alone operators of this library"}

    elapsed, px_rank = M["elapsed"], M["px_rank"]
    value = world * px_rank * args.steps / elapsed / 1e6
    pass_ms = M["pass_ms"]
    dom = max(pass_ms, key=pass_ms.get)
    kern_avg_ms = pass_ms[dom]
    algo_bytes = ALGO_BPP[dom] * px_rank
    achieved = algo_bytes / (kern_avg_ms * 1e-3) / 1e9 if kern_avg_ms > 0 else 0.0
    bytes_per_px_chain = 36 if "colormatch" in stages else 24

    # PMC counters of every workload's kernels: live on this box (three rocprofv3 --pmc passes of tools/prof_driver.py in their own
    # process, right after the timed region; --full only), else the committed run of the same command
    pmc, pmc_src, pmc_err = {}, None, None
    if full and rank == 0 and world == 1 and not args.no_live_traffic:
        try:
            pmc = live_traffic()
            pmc_src = "rocprofv3 --kernel-trace --pmc on this box right after the timed region (separate passes, own process, the same kernels on 16x4K frames)"
        except Exception as exc:
            pmc_err = f"live PMC passes failed ({type(exc).__name__}: {exc}); "
    if not pmc:
        pmc, name = committed_pmc()
        pmc_src = f"NOT collected in this process (rocprofv3 wraps a process): profiles/{name}" if name else None
    c = pmc.get((args.workload, dom), {})
    traffic = traffic_note = None
    if c.get("total"):
        cal = pmc.get("calibration_k_lut3d", {})
        traffic = round(c["total"] * px_rank / 1e9, 2)
        traffic_note = ((pmc_err or "") + f"{pmc_src}: FETCH_SIZE / WRITE_SIZE {c['read']} B/px read + {c['written']} B/px written (FETCH_SIZE x2 per the gfx950 "
                        f"calibration; k_lut3d in the same run: {cal.get('read')} + {cal.get('written')} for its known 12 + 12) x this launch's pixels"
                        + ("; the written bytes are the Lab image kept for pass 2, not re-reads" if dom == "stats" and "colormatch" in stages else ""))
    elif pmc_err:
        traffic_note = pmc_err

    # The unit that binds the dominant kernel.  Every kernel of this path moves its algorithmic bytes once (traffic above), and none of the
    # chains reaches the HBM roofline: they are bound by VALU issue.  Two views of it: `valu_busy_frac` = SIMD-cycles with a VALU
    # instruction executing (SQ_ACTIVE_INST_VALU) per pixel x the pixel rate, against the chip's 1,024 SIMDs x 2.4 GHz; `issue` =
    # lane-instructions per pixel x the rate against the measured v_fma_f32 peak, weighted by the issue cost of the instruction classes
    # that have a counter.
    rate = px_rank / (kern_avg_ms * 1e-3) if kern_avg_ms > 0 else 0.0
    valu_busy, valu_x4 = valu_fractions(c, rate)
    issue = None
    try:
        rates, rname = _profile_json("r02_valu_issue_rate_long.json", "r01_valu_issue_rate.json")
        peak_t = max(r["tera_lane_instr_s"] for r in rates["rows"] if r["instr"] == "v_fma_f32")
        ipp = c.get("valu_lane_instr")
        if ipp:
            rate_t = ipp * rate / 1e12
            # issue cost of the measured classes relative to a plain fp32 / integer op (profiles/r02_valu_issue_rate_long.json):
            # transcendental 3.45x, 64-bit integer multiply-add 1.8x (compare + select pairs, 1.65x, have no counter: not included)
            w_ipp = ipp + 2.45 * (c.get("valu_trans") or 0.0) + 0.8 * (c.get("valu_int64") or 0.0)
            w_rate = w_ipp * rate / 1e12
            issue = {"lane_instr_per_px": round(ipp, 1), "achieved": round(rate_t, 2), "peak": peak_t, "unit": "T lane-instr/s",
                     "frac": round(rate_t / peak_t, 4),
                     "weighted": {"lane_instr_per_px": round(w_ipp, 1), "of_which_transcendental": c.get("valu_trans"), "of_which_int64": c.get("valu_int64"),
                                  "achieved": round(w_rate, 2), "frac_of_measured_peak_66p5": round(w_rate / peak_t, 4),
                                  "frac_of_guide_peak_78p6": round(w_rate / 78.6, 4)},
                     "note": f"lane-instructions per pixel from {pmc_src} x this run's pixel rate; peak = v_fma_f32 at 8 waves/SIMD over >= 17 ms "
                             f"launches (profiles/{rname}); v_pk_* / fp64 / v_mad_u64_u32 issue at 1.8x, compare+select pairs 1.65x, transcendentals "
                             "3.45x a plain op"}
    except Exception:
        pass
    bound = "hbm"
    if valu_busy is not None and valu_busy > achieved / HBM_PEAK_GBS:
        bound = "valu-issue"

    if rank == 0:
        line = {
            "metric": "Mpixels/s (grain+LUT+colormatch+sharpen) at 4K" if args.workload == "chain4_4k" else f"Mpixels/s ({'+'.join(stages)})",
            "value": round(value, 1), "unit": "Mpixels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": f"synthetic-{args.dist} (generated on device, resident in HBM)",
            "config": {"workload": f"{W}x{H} x{frames} frames/GPU, {'+'.join(stages)} fused chain, LUT 33^3 (AMD_TealOrange_33.cube, this "
                                   f"pack's own cube: same size as the reference's Vintage Color.cube), grain chunk {M['chunk']} "
                                   f"(BASELINE configs[4] per-GPU shard)" if args.workload == "chain4_4k"
                       else f"{W}x{H} x{frames} frames/GPU, {'+'.join(stages)}",
                       "frames_per_gpu": frames, "height": H, "width": W, "parallelism": f"frames sharded x{world}",
                       "algorithmic_bytes_per_pixel_chain": bytes_per_px_chain,
                       "cm_math": "device" if "colormatch" in stages else None,
                       "cm_stats": ((f"device (torch-ROCm's reductions bit for bit, batch_size {CM_BATCH})" if (args.cm_stats or "device") == "device"
                                     else "fp64 (reference-frame rows split across the ranks, RCCL all-reduce)") if "colormatch" in stages else None),
                       "lut_note": "the cost of the LUT stage depends on the cube's SIZE and on the pixel values that index it, never on the values the "
                                   "cube holds (the gathers' addresses are the cell indices of the grained pixels): this pack's AMD_TealOrange_33.cube is the "
                                   "same workload as the reference's 33^3 Vintage Color.cube (SURVEY config 2; third-party asset, not shipped: lut_sha256 "
                                   "827ea0f659c8d6eb... in tests/golden/shipped_lut_digests.json) for both pixel distributions"},
            "rccl_ranks": dist.get_world_size() if dist.is_initialized() else 1,
            "dist_backend": (dist.get_backend() if dist.is_initialized() else None),
            "per_rank_ms_per_step": M["per_rank_ms"],
            "reference_stats_ms_per_step": M["ref_ms_per_step"],
            "reference_stats_note": ("device statistics of the whole reference frame on every rank, on a side stream next to pass 1 (timed alone here); "
                                     "the fp64 form -- rows split across the ranks + RCCL all-reduce -- is timed inside the steps of `fp64_stats_leg` "
                                     "(N > 1)") if "colormatch" in stages else None,
            "chain_hbm_frac": round(value / world * bytes_per_px_chain * 1e6 / 1e9 / HBM_PEAK_GBS, 4),
            "roofline": {"bound": bound, "kernel": _kernel_name(stages, dom),
                         "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                         "valu_busy_frac": valu_busy, "sq_active_inst_valu_x4_frac": valu_x4,
                         "bound_note": ("`achieved` / `peak` / `frac` are the contract's HBM figures (algorithmic bytes of the dominant kernel / its HIP-event "
                                        "time / 8 TB/s).  `bound` names the unit that limits the kernel: its measured HBM traffic is the algorithmic "
                                        "bytes (`traffic`), so HBM does not bind it; `valu_busy_frac` = class-weighted VALU lane-instructions per second "
                                        "/ the measured v_fma_f32 peak (66.5 T/s; `issue` has the terms) is the fraction of the VALU roofline it reaches; "
                                        "`sq_active_inst_valu_x4_frac` is rocprof's VALUBusy formula, which exceeds 1 on gfx950 (the counter advances once "
                                        "per instruction, a SIMD-32 issues a wave64 instruction in 2 cycles): reported, not used (DESIGN.md section 5.1)"),
                         "traffic_note": traffic_note,
                         "algorithmic_bytes_per_launch": algo_bytes, "avg_launch_ms": round(kern_avg_ms, 4),
                         "passes_ms": {k: round(v, 4) for k, v in pass_ms.items()}, "launches_per_step": M["launches_per_step"],
                         "issue": issue,
                         "issue_cost_roofline": issue_cost_roofline(args.workload, dom, c, rate),
                         "clock_during_timed_steps": M.get("clock"),
                         "path": kernel_path(ops, dev, stages)},
        }
        line["verified"] = None if M["verify"] is None else bool(M["verify"].get("verified"))
        line["verify"] = M["verify"]
        if M["digests"] is not None:
            line["output_sha256_per_rank_per_chunk"] = M["digests"]
        if M["fast_variant"] is not None:
            line["fast_variant"] = M["fast_variant"]
        if fp64_leg is not None:
            line["fp64_stats_leg"] = fp64_leg
    # The other single-GPU BASELINE configs and the second pixel distribution ("report both"), each timed the way
    # the headline is -- every rank would have to take part, so N = 1 only
    if full and world == 1 and args.workload == "chain4_4k" and not args.no_configs:
        n1080 = 128 if args.frames is None else args.frames          # BASELINE's frame counts unless --frames shrinks the run
        legs = [("chain4_4k", "video", frames), ("chain3_4k", "uniform", frames), ("chain3_4k", "video", frames),
                ("grain_lut_1080p", "uniform", n1080), ("grain_lut_1080p", "video", n1080), ("colormatch_4k", "uniform", 2 * frames)]
        # chain 3 with the other cube sizes of the field: 25^3 (8 of the reference's 12 shipped cubes) and 17^3 (node table staged in LDS)
        legs += [("chain3_4k", "uniform", frames, "AMD_WarmFilm_25.cube"), ("chain3_4k", "video", frames, "AMD_WarmFilm_25.cube"),
                 ("chain3_4k", "uniform", frames, "AMD_Identity_17.cube")]
        # north_star's own size for its target pass: "fused grain+LUT+sharpen at 4K x 512 frames" (102 GB in + out resident)
        legs += [("chain3_4k", "uniform", 2 * frames), ("chain3_4k", "video", 2 * frames)]
        cfgs = {"headline": leg_summary(M, world, pmc, pmc_src)}
        for wl, pd, nf, *cb in legs:
            key = f"{wl}.{pd}" + (f".{cb[0].split('_')[-1].split('.')[0]}cube" if cb else "") + (f".{nf}frames" if wl == "chain3_4k" and nf != frames else "")
            try:
                # (a 1080p step is 3 ms: one host hiccup inside five of them shows -- those legs take four times the steps)
                L = run_workload(C, args, wl, pd, nf, max(args.steps // 2, 3) * (4 if WORKLOADS[wl][0] <= 1080 else 1), 3, verify=not args.no_verify,
                                 cube_name=cb[0] if cb else None)
                cfgs[key] = leg_summary(L, world, pmc if not cb else {}, pmc_src)        # (the PMC passes ran the 33^3 cube)
                if cb:
                    cfgs[key]["cube"] = cb[0]
            except Exception as exc:
                cfgs[key] = {"error": f"{type(exc).__name__}: {exc}"}
        cfgs["note"] = ("BASELINE.json configs[1] = grain_lut_1080p (128 frames), configs[2] = chain3_4k (256 frames; the pass north_star's >= 60 % target "
                        "names), configs[3] = colormatch_4k (512 frames), configs[4] per-GPU shard = headline; `pixels` uniform = iid U[0,1) (worst case "
                        "for the LUT gathers), video = smooth field + N(0, 0.02) texture (SURVEY.md section 8d, D2 / D1).  hbm_frac = Mpix_s x "
                        "algorithmic_bytes_per_pixel / 8 TB/s; valu_busy_frac of the dominant kernel as in `roofline`; `verified` = first and last RNG "
                        "chunk against the stand-alone operators and the oracle after the timed steps; the `...25cube` / `...17cube` legs run chain 3 with this pack's "
                        "25^3 and 17^3 cubes (the default legs: AMD_TealOrange_33.cube); `chain3_4k....512frames` = the same pass at north_star's own size, 4K x 512 "
                        "frames (102 GB of frames resident); `clock_during_timed_steps` = the shader clock and socket power sampled while the leg's timed steps ran")
        try:
            g = graph_leg(C, args, frames, max(args.steps // 2, 3), 2)
            g["vs_headline"] = round(g["Mpix_s"] / max(value, 1e-9), 3)
            cfgs["graph_four_nodes_device_resident"] = g
        except Exception as exc:
            cfgs["graph_four_nodes_device_resident"] = {"error": f"{type(exc).__name__}: {exc}"}
        line["configs"] = cfgs
    if rank == 0:
        if full and world == 1 and not args.no_host_fed and args.workload == "chain4_4k":
            # what a ComfyUI graph sees: CPU tensors in, CPU tensors out, every node call crossing PCIe both ways -- never `value`
            try:
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import host_fed
                torch.cuda.empty_cache()
                line["host_fed"] = host_fed.measure(frames=16, reps=5, warmup=4)       # (torch's host / device pools of this process settle after 3 calls per row)
            except Exception as exc:
                line["host_fed"] = {"error": f"{type(exc).__name__}: {exc}"}
        if full and not args.no_cpu_baseline:
            # rank 0 only, any N (the other ranks wait at the final barrier; the process group's timeout covers it)
            try:
                line["cpu_baseline"] = cpu_baseline(stages, args.cpu_frames if H > 1080 else 4 * args.cpu_frames, H, W, lut_cpu, per_node=True)
            except Exception as exc:      # never lose the GPU line to a host-side problem
                line["cpu_baseline"] = {"value": None, "unit": "Mpixels/s", "cores": torch.get_num_threads(), "kind": "port",
                                        "sample": f"failed: {type(exc).__name__}: {exc}"}
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(line) + "\n").encode())
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

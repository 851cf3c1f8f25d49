"""Measure the Video Compare Slider's byte hand-off on an MI355X and write profiles/compare_video.json.

    python tools/bench_compare.py [--rounds 8] [--warmup 2] [--reps 3] [--out profiles/compare_video.json]

Shapes: 257 frames of 1920 x 1080 and 64 of 3840 x 2160, three channels, a sink that discards the bytes.
  launch     vrg_rgb24_frames_u8 timed by HIP events (`reps` calls between two events) in the SAME run beside a non-temporal copy of the
             same 15 B/px (12 in, 3 out: vrg_debug_copy_f32, mode 1) and beside vrg_anchor_store_u8 at the same shape, order rotated;
  hand-off   ops.stream_rgb24 by the wall clock around the whole call, from a device-resident batch, from a pending LazyFrames and from a
             CPU batch, beside the reference's own sequence on this machine's CPU -- `.cpu().numpy()` of the fp32 batch, then
             np.clip(frame[..., :3] * 255.0, 0, 255).astype(np.uint8) and .tobytes() frame by frame -- in the same process, order rotated.
Medians of `rounds` rounds after `warmup` rounds.  No threshold is set: the figures are what was found, losing legs included."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--shapes", default="257x1080x1920,64x2160x3840")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_video.json"))
a = ap.parse_args()

load_package()
from comfyui_vrgamedevgirl_amd import _devices, _hip, ops  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_compare: no GPU visible; nothing is measured without one")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
SHAPES = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]


def rotated(candidates, timed):
    """every candidate once per round, the first one moving on by one each round; `timed(fn)` -> ms"""
    names = list(candidates)
    samples = {name: [] for name in names}
    for r in range(a.warmup + a.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            ms = timed(candidates[name])
            if r >= a.warmup:
                samples[name].append(ms)
        print("  round", r, {name: round(s[-1], 3) for name, s in samples.items() if s}, flush=True)
    return {name: {"ms": statistics.median(s), "samples_ms": s} for name, s in samples.items()}


def by_events(fn):
    e0, e1 = ops.HipEvent(), ops.HipEvent()
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_ms(e1) / a.reps


def by_wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def discard(view):
    pass


def reference_sequence(images):
    host = images.detach().cpu().numpy()
    for frame in host:
        discard(np.clip(frame[..., :3] * 255.0, 0, 255).astype(np.uint8).tobytes())


def pending_result(resident):
    """a LazyFrames over `resident`'s frames whose download has not been queued: what a node of the pack returns"""
    host = torch.empty(resident.shape, dtype=torch.float32)                 # never filled: the frames stay in HBM
    ran = torch.cuda.Event()
    ran.record()
    pend = _devices._Pending(host, dev, [(0, int(resident.shape[0]), resident, ran)], resident.numel() * 4)
    return _devices.LazyFrames(host, pend), pend


result = {"device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps, "shapes": {}}
for n, height, width in SHAPES:
    label = f"{n}x{width}x{height}x3"
    g = torch.Generator(device=dev).manual_seed(n)
    resident = torch.rand((n, height, width, 3), device=dev, generator=g) * 1.2 - 0.1
    data = torch.empty((n, height, width, 3), dtype=torch.uint8, device=dev)
    pixels = n * height * width
    moved = pixels * 15
    scratch = torch.empty(2 * (moved // 8 // 4 * 4) + 64, dtype=torch.float32, device=dev)
    floats = moved // 8 // 4 * 4

    def copy():
        _hip.check(_hip.lib().vrg_debug_copy_f32(_hip.ptr(scratch), _hip.ptr(scratch[floats:]), floats, 1, _hip.current_stream()), "vrg_debug_copy_f32")

    rec = {"pixels": pixels, "moved_bytes": moved, "copy_bytes": floats * 8}
    rec["launch"] = rotated({"rgb24_frames": lambda: ops.rgb24_frames(resident, out=data), "copy_15B_per_px": copy,
                             "anchor_store_bytes": lambda: ops.anchor_store_bytes(resident, out=data)}, by_events)
    rec["launch_bytes_per_s_over_copy"] = (moved / rec["launch"]["rgb24_frames"]["ms"]) / (floats * 8 / rec["launch"]["copy_15B_per_px"]["ms"])
    rec["launch_gpix_per_s"] = pixels / rec["launch"]["rgb24_frames"]["ms"] / 1e6
    del scratch
    cpu = resident.cpu()
    want = np.clip(cpu[0].numpy()[..., :3] * 255.0, 0, 255).astype(np.uint8)
    rec["first_frame_equals_numpy"] = bool(np.array_equal(ops.rgb24_frames(resident[:1]).cpu().numpy()[0], want))
    lazy, pend = pending_result(resident)
    skipped = _devices._LAZY.downloads_skipped
    rec["handoff"] = rotated({"device_resident": lambda: ops.stream_rgb24(resident, discard), "pending_lazyframes": lambda: ops.stream_rgb24(lazy, discard),
                              "cpu_batch": lambda: ops.stream_rgb24(cpu, discard), "reference_sequence_cpu_batch": lambda: reference_sequence(cpu),
                              "reference_sequence_device_batch": lambda: reference_sequence(resident)}, by_wall)
    rec["pending_still_pending"] = _devices.pending_of(lazy) is pend
    rec["downloads_skipped"] = _devices._LAZY.downloads_skipped - skipped
    ref_cpu, ref_dev = rec["handoff"]["reference_sequence_cpu_batch"]["ms"], rec["handoff"]["reference_sequence_device_batch"]["ms"]
    rec["reference_over_handoff"] = {"device_resident": ref_dev / rec["handoff"]["device_resident"]["ms"],
                                     "pending_lazyframes": ref_dev / rec["handoff"]["pending_lazyframes"]["ms"],
                                     "cpu_batch": ref_cpu / rec["handoff"]["cpu_batch"]["ms"]}
    result["shapes"][label] = rec
    print(label, json.dumps({k: ({n_: round(v_["ms"], 3) for n_, v_ in v.items()} if k in ("launch", "handoff") else v) for k, v in rec.items()}), flush=True)
    del resident, data, cpu, lazy, pend

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", a.out)

"""The LTX MSR reference frames, timed: five 4000 x 3000 byte stills -> 41 frames of 736 x 1280 and of 1920 x 1080.

    python tools/bench_msr.py [--rounds 7] [--reps 5] [--out profiles/msr_reference.json]

Device-resident (HIP events around `--reps` launches after a warm-up; the candidates alternate inside every round, median of `--rounds`):
  * vrg_msr_frames_f32 alone (descriptors and table already on the device);
  * a non-temporal float4 fill of the same output bytes (vrg_debug_copy_f32 mode 4): the write ceiling the launch is bounded by;
  * the two-step route without this kernel: vrg_lanczos4_u8 per source, then torch's convert, divide (by a 0-d tensor: torch's IEEE
    division; `/ 255.0` with a Python scalar is a reciprocal multiply on the device and is counted apart) and index_select on the
    device.  Its output bits are compared with the launch's.
  * ops.msr_reference_frames from resident pictures (the launch plus its host check and descriptor upload).
Host-fed (wall clock ending in a device synchronise): ops.msr_reference_frames from CPU byte pictures, alone and followed by the
download into a page-locked host tensor (what the builder node returns).
The host part of the reference's route that runs without cv2, on this machine's CPU: np.stack of the 41 byte frames, astype(float32),
/ 255.0 -- the five cv2 resizes come on top of it."""
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
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msr_reference.json"))
a = ap.parse_args()

load_package()
from comfyui_vrgamedevgirl_amd import _hip, ops  # noqa: E402
from comfyui_vrgamedevgirl_amd import vrgdg_ltx_msr_reference_builder as nodes  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_msr: no GPU visible; nothing is measured without one")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
SRC_W, SRC_H, FRAMES, PICTURES = 4000, 3000, 41, 5
rng = np.random.Generator(np.random.PCG64(2))
host_pics = [rng.integers(0, 256, (SRC_H, SRC_W, 3), dtype=np.uint8) for _ in range(PICTURES)]
dev_pics = [torch.from_numpy(p).to(dev) for p in host_pics]
counts = ops.expand_counts(PICTURES, FRAMES)
index = torch.tensor([i for i, n in enumerate(counts) for _ in range(n)], device=dev)
unit = torch.full((), 255.0, dtype=torch.float32, device=dev)          # a tensor divisor: torch's IEEE division


def interleaved(candidates):
    """{name: (median ms, samples)}: every round times each candidate once, `reps` calls between two events"""
    for fn in candidates.values():
        fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in candidates}
    for _ in range(a.rounds):
        for name, fn in candidates.items():
            e0, e1 = ops.HipEvent(), ops.HipEvent()
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            samples[name].append(e0.elapsed_ms(e1) / a.reps)
    return {name: (statistics.median(s), s) for name, s in samples.items()}


def wall(fn, rounds):
    fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3)
    return {"ms": statistics.median(samples), "samples_ms": samples}


sizes = {}
for width, height in ((736, 1280), (1920, 1080)):
    label = f"{width}x{height}x{FRAMES}"
    out_bytes = FRAMES * height * width * 12
    plan = ops.msr_plan([p.shape[:2] for p in host_pics], (width, height), FRAMES)
    desc = plan.desc.copy()
    for i, p in enumerate(dev_pics):
        desc["src"][i] = p.data_ptr()
    plan.check(desc)
    table = torch.from_numpy(plan.table()).to(dev)
    d = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(dev)
    out = torch.empty((FRAMES, height, width, 3), dtype=torch.float32, device=dev)
    fill = torch.empty(out.numel(), dtype=torch.float32, device=dev)

    def launch():
        _hip.check(_hip.lib().vrg_msr_frames_f32(_hip.ptr(d), len(desc), _hip.ptr(table), plan.n_taps, _hip.ptr(out), FRAMES, height, width,
                                                 _hip.current_stream()), "vrg_msr_frames_f32")

    def write_ceiling():
        _hip.check(_hip.lib().vrg_debug_copy_f32(_hip.ptr(fill), _hip.ptr(fill), fill.numel(), 4, _hip.current_stream()), "fill")

    def two_step(divisor=unit):
        small = torch.cat([ops.resize_frames_u8(p.unsqueeze(0), width, height) for p in dev_pics])
        return (small.to(torch.float32) / divisor).index_select(0, index)

    def whole_op():
        return ops.msr_reference_frames(dev_pics, (width, height), FRAMES)

    launch()
    same_bits = bool(torch.equal(out.view(torch.int32), two_step().view(torch.int32)))
    # torch divides a device tensor by a Python scalar as a multiplication by its reciprocal: not the reference's numpy division
    scalar = two_step(255.0)
    scalar_differs = int((out.view(torch.int32) != scalar.view(torch.int32)).sum())
    scalar_worst = float((out - scalar).abs().max())
    del scalar
    assert torch.equal(out, whole_op())
    res = interleaved({"vrg_msr_frames_f32": launch, "non-temporal float4 fill of the output bytes": write_ceiling,
                       "two-step route (vrg_lanczos4_u8 per source + torch convert, divide, index_select)": two_step,
                       "ops.msr_reference_frames, resident pictures": whole_op})
    ceiling = res["non-temporal float4 fill of the output bytes"][0]
    rows = {}
    for name, (ms, s) in res.items():
        rows[name] = {"ms": ms, "samples_ms": s, "output_TB_per_s": out_bytes / ms / 1e9, "fraction_of_write_ceiling": ceiling / ms}
        print(f"{label}: {name}: {ms:.3f} ms, {out_bytes / ms / 1e9:.2f} TB/s of output, {ceiling / ms:.3f} of the fill", flush=True)
    del fill
    host = {"ops.msr_reference_frames from CPU byte pictures": wall(lambda: ops.msr_reference_frames(host_pics, (width, height), FRAMES), a.host_rounds),
            "the same plus the download into a page-locked host tensor":
                wall(lambda: nodes._to_host(ops.msr_reference_frames(host_pics, (width, height), FRAMES)), a.host_rounds)}
    byte_frames = [rng.integers(0, 256, (height, width, 3), dtype=np.uint8) for _ in range(PICTURES)]
    frames = [byte_frames[i] for i, n in enumerate(counts) for _ in range(n)]
    cpu = []
    for _ in range(a.host_rounds):
        t0 = time.perf_counter()
        np.stack(frames).astype(np.float32) / 255.0
        cpu.append((time.perf_counter() - t0) * 1e3)
    host["reference on this CPU: np.stack, astype(float32), / 255.0 (without its five cv2 resizes)"] = {"ms": statistics.median(cpu), "samples_ms": cpu}
    for name, row in host.items():
        print(f"{label}: {name}: {row['ms']:.1f} ms", flush=True)
    sizes[label] = {"output_bytes": out_bytes, "two_step_output_bits_equal": same_bits,
                    "two_step_with_python_scalar_divisor": {"values_that_differ": scalar_differs, "largest_difference": scalar_worst}, "device_resident": rows, "host_fed": host}
    del out
    torch.cuda.empty_cache()

result = {"workload": f"{PICTURES} uniform-random {SRC_W}x{SRC_H} byte stills -> {FRAMES} fp32 frames, repeats {counts}",
          "device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "host_rounds": a.host_rounds, "sizes": sizes}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print("wrote", a.out)

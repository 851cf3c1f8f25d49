"""The detector input, timed: 4K fp32 frames in HBM, rotation modes off / light / strong.

    python tools/bench_detect_prep.py [--frames 256] [--host-frames 16] [--out profiles/detect_prep.json]

Device-resident (HIP events around `--reps` launches after a warm-up, median of `--rounds`), per mode: the fused launch of
vrg_detect_blobs_f32 (every frame x angle x region) as time per batch and per frame, and vrg_warp_linear_u8 over the rotated angles of the
mode as time and as TB/s of the bytes it writes; the float4 copy of the SAME frames (vrg_debug_copy_f32: reads and writes them) is timed in
the same run as the yardstick of what touching every pixel once costs.  Host-fed (wall clock, `--host-frames` CPU 4K frames, pageable and
page-locked): detector_blobs in the default mode against the plain upload of the same frames.  No threshold is attached to these
numbers."""
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
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--host-frames", type=int, default=16)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_prep.json"))
a = ap.parse_args()

load_package()
from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes as FF  # noqa: E402
from comfyui_vrgamedevgirl_amd import _hip, ops  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) / a.reps)
    return statistics.median(samples), samples


def wall(fn):
    fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(samples), samples


F, H, W = a.frames, 2160, 3840
x = torch.rand((F, H, W, 3), dtype=torch.float32, device=dev)
frame_bytes = H * W * 12
dst = torch.empty_like(x)
copy_ms, copy_samples = timed(lambda: _hip.check(_hip.lib().vrg_debug_copy_f32(_hip.ptr(x), _hip.ptr(dst), x.numel(), 1, _hip.current_stream()), "copy"))
del dst
torch.cuda.empty_cache()
copy_rate = 2 * F * frame_bytes / (copy_ms * 1e-3) / 1e12
print(f"float4 copy of {F} x 4K: {copy_ms:.3f} ms, {copy_rate:.3f} TB/s read + write", flush=True)

modes = {}
for label, mode in (("off", "Off (fastest)"), ("light", "Light: ±15°"), ("strong", "Strong: ±15° and ±30°")):
    plan = FF.detection_plan(W, H, mode)
    desc, _ = plan.descriptors(range(F))
    n_blobs = int(desc.size)
    rec = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(dev)
    tr = torch.from_numpy(plan.transforms.copy()).to(dev) if len(plan.transforms) else None
    out = torch.empty((n_blobs, 3, 300, 300), dtype=torch.float32, device=dev)

    def blobs():
        _hip.check(_hip.lib().vrg_detect_blobs_f32(_hip.ptr(x), F, H, W, 3, _hip.ptr(tr) if tr is not None else None, len(plan.transforms), _hip.ptr(rec),
                                                   n_blobs, _hip.ptr(out), _hip.current_stream()), "vrg_detect_blobs_f32")

    ms, samples = timed(blobs)
    entry = {"angles": plan.angles, "blobs": n_blobs, "blob_bytes": n_blobs * 3 * 300 * 300 * 4,
             "vrg_detect_blobs_f32": {"ms": ms, "samples_ms": samples, "ms_per_frame": ms / F, "time_as_fraction_of_the_copy_time": ms / copy_ms}}
    print(f"{label}: {n_blobs} blobs in one launch: {ms:.3f} ms = {ms / F * 1e3:.1f} us per frame, {ms / copy_ms:.3f} of the copy's time", flush=True)
    del out
    torch.cuda.empty_cache()
    rotated = [t for t in plan.transform_index if t >= 0]
    if rotated:
        fd = np.array([(f, t) for f in range(F) for t in rotated], dtype=ops.DETECT_FRAME_DESC)
        frec = torch.from_numpy(fd.view(np.uint8).reshape(-1).copy()).to(dev)
        wout = torch.empty((fd.size, H, W, 3), dtype=torch.uint8, device=dev)

        def warp():
            _hip.check(_hip.lib().vrg_warp_linear_u8(_hip.ptr(x), 3, F, H, W, _hip.ptr(tr), len(plan.transforms), _hip.ptr(frec), int(fd.size), _hip.ptr(wout),
                                                     _hip.current_stream()), "vrg_warp_linear_u8")

        wms, wsamples = timed(warp)
        written = int(fd.size) * H * W * 3
        entry["vrg_warp_linear_u8"] = {"frames_written": int(fd.size), "ms": wms, "samples_ms": wsamples, "written_bytes": written,
                                       "TB_per_s_written": written / (wms * 1e-3) / 1e12, "ms_per_rotated_frame": wms / fd.size}
        print(f"{label}: {fd.size} rotated frames: {wms:.3f} ms, {written / (wms * 1e-3) / 1e12:.3f} TB/s written", flush=True)
        del wout
        torch.cuda.empty_cache()
    modes[label] = entry
del x
torch.cuda.empty_cache()

n = a.host_frames
host = {}
plan = FF.detection_plan(W, H, "Light: ±15°")
pageable = torch.rand((n, H, W, 3), dtype=torch.float32)
for label, frames in (("pageable", pageable), ("page-locked", pageable.pin_memory())):
    blob_ms, blob_samples = wall(lambda: FF.detector_blobs(frames, plan))
    up_ms, up_samples = wall(lambda: frames.to(dev, non_blocking=True))
    host[label] = {"frames": n, "detector_blobs, light": {"ms": blob_ms, "samples_ms": blob_samples},
                   "plain upload of the same frames": {"ms": up_ms, "samples_ms": up_samples}}
    print(f"host-fed, {n} x 4K {label}: detector_blobs (light) {blob_ms:.2f} ms, plain upload {up_ms:.2f} ms", flush=True)

result = {"workload": "uniform-random fp32 RGB 4K frames", "device": torch.cuda.get_device_name(0), "frames": F, "height": H, "width": W,
          "reps": a.reps, "rounds": a.rounds,
          "float4 copy of the same frames (reads and writes them)": {"ms": copy_ms, "samples_ms": copy_samples, "TB_per_s_read_plus_write": copy_rate},
          "device_resident": modes, "host_fed_4K": host}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print("wrote", a.out)

"""The shot-aware cut score, timed: 4K and 1080p fp32 frames.

    python tools/bench_cut.py [--frames 256] [--host-frames 16] [--out profiles/cut_score.json]

Device-resident (HIP events around `--reps` launches after a warm-up, median of `--rounds`), per size: vrg_cut_thumbs_f32 as time per
batch, as algorithmic TB/s at 12 B per pixel (the frames read once; the 12 KB thumbnail per frame is not counted) and as a fraction of the
float4 copy of the SAME frames timed in the same run (vrg_debug_copy_f32: it reads and writes them, so it moves twice the bytes the
kernel has to read -- both fractions are reported: time against time, and rate against the copy's read + write rate); then the two small
kernels (vrg_cut_hist_u8, vrg_cut_pair_sums) and the whole of shot_cut_scores.  Host-fed (wall clock, `--host-frames` CPU 4K frames,
pageable and page-locked): shot_cut_scores against the plain upload of the same frames."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--host-frames", type=int, default=16)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_score.json"))
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


sizes = {}
for label, (H, W) in (("4K", (2160, 3840)), ("1080p", (1080, 1920))):
    F = a.frames
    x = torch.rand((F, H, W, 3), dtype=torch.float32, device=dev)
    read_bytes = F * H * W * 12
    dst = torch.empty_like(x)
    copy_ms, copy_samples = timed(lambda: _hip.check(_hip.lib().vrg_debug_copy_f32(_hip.ptr(x), _hip.ptr(dst), x.numel(), 1, _hip.current_stream()), "copy"))
    del dst
    torch.cuda.empty_cache()
    thumbs = ops.cut_thumbnails(x)
    hist = ops.cut_histograms(thumbs)
    ms, samples = timed(lambda: ops.cut_thumbnails(x, out=thumbs))
    hist_ms, hist_samples = timed(lambda: ops.cut_histograms(thumbs))
    pair_ms, pair_samples = timed(lambda: ops.cut_pair_sums(thumbs, hist))
    all_ms, all_samples = wall(lambda: FF.shot_cut_scores(x))
    copy_rate, rate = 2 * read_bytes / (copy_ms * 1e-3) / 1e12, read_bytes / (ms * 1e-3) / 1e12
    sizes[label] = {
        "frames": F, "height": H, "width": W, "algorithmic_read_bytes": read_bytes,
        "float4 copy of the same frames (reads and writes them)": {"ms": copy_ms, "samples_ms": copy_samples, "TB_per_s_read_plus_write": copy_rate},
        "vrg_cut_thumbs_f32": {"ms": ms, "samples_ms": samples, "ms_per_frame": ms / F, "algorithmic_TB_per_s": rate,
                               "time_as_fraction_of_the_copy_time": ms / copy_ms, "rate_as_fraction_of_the_copy_rate": rate / copy_rate},
        "vrg_cut_hist_u8": {"ms": hist_ms, "samples_ms": hist_samples},
        "vrg_cut_pair_sums": {"ms": pair_ms, "samples_ms": pair_samples},
        "shot_cut_scores, wall clock with the download of the sums and the host arithmetic": {"ms": all_ms, "samples_ms": all_samples},
    }
    print(f"{label} x {F}: thumbnails {ms:.3f} ms = {rate:.3f} TB/s algorithmic, {ms / copy_ms:.3f} of the copy's time ({copy_ms:.3f} ms, "
          f"{copy_rate:.3f} TB/s read + write); histograms {hist_ms:.4f} ms, pair sums {pair_ms:.4f} ms; shot_cut_scores {all_ms:.3f} ms", flush=True)
    del x, thumbs, hist
    torch.cuda.empty_cache()

# host-fed: CPU 4K frames
n, H, W = a.host_frames, 2160, 3840
host = {}
pageable = torch.rand((n, H, W, 3), dtype=torch.float32)
for label, frames in (("pageable", pageable), ("page-locked", pageable.pin_memory())):
    score_ms, score_samples = wall(lambda: FF.shot_cut_scores(frames))
    up_ms, up_samples = wall(lambda: frames.to(dev, non_blocking=True))
    host[label] = {"frames": n, "shot_cut_scores": {"ms": score_ms, "samples_ms": score_samples},
                   "plain upload of the same frames": {"ms": up_ms, "samples_ms": up_samples}}
    print(f"host-fed, {n} x 4K {label}: shot_cut_scores {score_ms:.2f} ms, plain upload {up_ms:.2f} ms", flush=True)

result = {"workload": "uniform-random fp32 RGB frames", "device": torch.cuda.get_device_name(0), "bytes_per_pixel": 12, "reps": a.reps, "rounds": a.rounds,
          "device_resident": sizes, "host_fed_4K": host}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print("wrote", a.out)

"""The multi-reference image batches, timed: 50 RGB pictures of mixed sizes (0.3 to 8 MP, six aspect ratios, seeded).

    python tools/bench_refbatch.py [--rounds 7] [--host-rounds 3] [--out profiles/refbatch.json]

Device-resident (HIP events around one call; two warm-up rounds, then the candidates alternate inside every round, median of `--rounds`):
  1. ops.scale_reference_images to 1.0 MP, each of the five methods, against the reference's sequence as eager torch ops on the same
     device tensors (F.interpolate picture by picture); for lanczos the yardstick is the reference's own route, the CPU Pillow round trip
     of every picture (download, quantise, resize, / 255, upload), timed by wall clock;
  2. ops.batch_reference_images of the 50 scaled pictures to the first one's shape (bilinear), against centre-crop view + F.interpolate
     per picture + torch.cat on the device;
  beside each a non-temporal float4 fill of the same output bytes (vrg_debug_copy_f32 mode 4), the write ceiling.
Host-fed (wall clock ending in a device synchronise):
  3. ops.scale_reference_images from 50 CPU pictures (bilinear), against the reference's sequence on this machine's CPU (F.interpolate per
     picture) followed by the upload of every result, as the encoder on the device needs them."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--host-rounds", type=int, default=3)
ap.add_argument("--pictures", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refbatch.json"))
a = ap.parse_args()

load_package()
from comfyui_vrgamedevgirl_amd import _hip, ops  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_refbatch: no GPU visible; nothing is measured without one")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
WARMUP, MEGAPIXELS = 2, 1.0
rng = np.random.default_rng(7)
ASPECTS = (16 / 9, 4 / 3, 1.0, 3 / 4, 9 / 16, 3 / 2)
shapes = []
for k in range(a.pictures):
    pixels, aspect = rng.uniform(0.3e6, 8e6), ASPECTS[k % len(ASPECTS)]
    shapes.append((1, max(1, round(math.sqrt(pixels / aspect))), max(1, round(math.sqrt(pixels * aspect))), 3))
gen = torch.Generator().manual_seed(7)
host_pictures = [torch.rand(s, generator=gen) for s in shapes]
pictures = [p.to(dev) for p in host_pictures]
sizes = [ops.total_pixels_size(s[1], s[2], MEGAPIXELS, 1) for s in shapes]


def events(candidates, rounds):
    for _ in range(WARMUP):
        for fn in candidates.values():
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in candidates}
    for _ in range(rounds):
        for name, fn in candidates.items():
            e0, e1 = ops.HipEvent(), ops.HipEvent()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            samples[name].append(e0.elapsed_ms(e1))
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
    return statistics.median(samples), samples


def filler(floats):
    buf = torch.empty((floats + 3) & ~3, dtype=torch.float32, device=dev)             # the probe takes whole float4s
    return lambda: _hip.check(_hip.lib().vrg_debug_copy_f32(_hip.ptr(buf), _hip.ptr(buf), buf.numel(), 4, _hip.current_stream()), "fill")


def eager_scale(pics, method):
    return [F.interpolate(p.movedim(-1, 1), size=size, mode=method).movedim(1, -1) for p, size in zip(pics, sizes)]


def pillow_scale(pics):
    from PIL import Image
    out = []
    for p, (h, w) in zip(pics, sizes):
        image = Image.fromarray(np.clip(255. * p[0].cpu().numpy(), 0, 255).astype(np.uint8))
        out.append(torch.from_numpy(np.array(image.resize((w, h), resample=Image.Resampling.LANCZOS)).astype(np.float32) / 255.0).unsqueeze(0).to(dev))
    return out


def eager_batch(pics):
    base = pics[0]
    kept = [base]
    for p in pics[1:]:
        if p.shape[1:] != base.shape[1:]:
            x, y, w, h = ops.center_crop_rect(int(p.shape[2]), int(p.shape[1]), int(base.shape[2]), int(base.shape[1]))
            p = F.interpolate(p.movedim(-1, 1).narrow(-2, y, h).narrow(-1, x, w), size=(base.shape[1], base.shape[2]), mode="bilinear").movedim(1, -1)
        kept.append(p)
    return torch.cat(kept, dim=0)


def rows(res, out_bytes, fill_name):
    ceiling = res[fill_name][0]
    return {name: {"ms": ms, "samples_ms": s, "output_GB_per_s": out_bytes / ms / 1e6, "fraction_of_write_ceiling": ceiling / ms}
            for name, (ms, s) in res.items()}


FILL = "non-temporal float4 fill of the output bytes"
result = {"scale": {}, "batch": {}, "host_fed": {}}
out_floats = sum(h * w * 3 for h, w in sizes)
fill = filler(out_floats)
for method in ops.REFBATCH_METHODS:
    mine = lambda m=method: ops.scale_reference_images(pictures, m, MEGAPIXELS, 1)          # noqa: E731
    if method == "lanczos":
        res = events({"ops.scale_reference_images": mine, FILL: fill}, a.rounds)
        table = rows(res, out_floats * 4, FILL)
        ms, s = wall(lambda: pillow_scale(pictures), max(1, a.host_rounds - 1))
        table["the reference's CPU Pillow round trip per picture (wall clock)"] = {"ms": ms, "samples_ms": s}
    else:
        res = events({"ops.scale_reference_images": mine, "eager torch: F.interpolate per picture on the device": lambda m=method: eager_scale(pictures, m),
                      FILL: fill}, a.rounds)
        table = rows(res, out_floats * 4, FILL)
        worst = max(float((g - w).abs().max()) for g, w in zip(mine(), eager_scale(pictures, method)))
        table["largest_difference_from_the_eager_device_sequence"] = worst
    result["scale"][method] = table
    for name, row in table.items():
        if isinstance(row, dict):
            print(f"scale {method}: {name}: {row['ms']:.3f} ms" + (f", {row['fraction_of_write_ceiling']:.3f} of the fill" if "fraction_of_write_ceiling" in row else ""), flush=True)
del fill
torch.cuda.empty_cache()

scaled = ops.scale_reference_images(pictures, "bilinear", MEGAPIXELS, 1)
batch_floats = len(scaled) * scaled[0].numel()
res = events({"ops.batch_reference_images": lambda: ops.batch_reference_images(scaled, "bilinear"),
              "eager torch: crop view + F.interpolate per picture + torch.cat on the device": lambda: eager_batch(scaled),
              FILL: filler(batch_floats)}, a.rounds)
result["batch"] = rows(res, batch_floats * 4, FILL)
result["batch"]["largest_difference_from_the_eager_device_sequence"] = float((ops.batch_reference_images(scaled, "bilinear") - eager_batch(scaled)).abs().max())
for name, row in result["batch"].items():
    if isinstance(row, dict):
        print(f"batch bilinear: {name}: {row['ms']:.3f} ms, {row['fraction_of_write_ceiling']:.3f} of the fill", flush=True)
torch.cuda.empty_cache()

for name, fn in (("ops.scale_reference_images from CPU pictures", lambda: ops.scale_reference_images(host_pictures, "bilinear", MEGAPIXELS, 1)),
                 ("the reference's sequence on this CPU plus the upload of every result", lambda: [t.to(dev) for t in eager_scale(host_pictures, "bilinear")])):
    ms, s = wall(fn, a.host_rounds)
    result["host_fed"][name] = {"ms": ms, "samples_ms": s}
    print(f"host-fed bilinear: {name}: {ms:.1f} ms", flush=True)

result.update({"workload": f"{a.pictures} uniform-random fp32 RGB pictures, {min(s[1] * s[2] for s in shapes) / 1e6:.2f} to "
                           f"{max(s[1] * s[2] for s in shapes) / 1e6:.2f} MP ({sum(s[1] * s[2] for s in shapes) / 1e6:.0f} MP in all), scaled to "
                           f"{MEGAPIXELS} MP each ({out_floats * 4 / 1e6:.0f} MB of output); the batch joins the scaled pictures at {list(scaled[0].shape[1:])}",
               "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup_rounds": WARMUP, "host_rounds": a.host_rounds,
               "cpu_threads": torch.get_num_threads(), "bicubic_form": "direct: 16 global loads a value, no LDS staging"})
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print("wrote", a.out)

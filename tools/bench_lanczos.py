"""The enhancer upscale, timed: 1080p -> 4K on uniform-random bytes.

    python tools/bench_lanczos.py [--frames 256] [--host-frames 16] [--out profiles/lanczos.json]

Device-resident (HIP events around `--reps` launches after a warm-up, median of `--rounds`): vrg_lanczos4_u8, the fused
vrg_upscale_sharpen_grain_u8 and the two-launch route, with grain on and off, each as time per batch and as a fraction of the float4
copy ceiling measured in the same run at the algorithmic bytes (0.75 B read + 3 B written per output pixel at 2x).
Host-fed (wall clock, `--host-frames` frames): _enhance_decoded from 1080p host bytes against uploading the same frames already at 4K
through _apply_effects_batch -- the route without this kernel, with its CPU upscale not even counted."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lanczos.json"))
a = ap.parse_args()

load_package()
from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneVideoEnhancerNodes as E  # noqa: E402
from comfyui_vrgamedevgirl_amd import _hip, ops  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
H, W, OH, OW = 1080, 1920, 2160, 3840
F = a.frames
x = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev)
algorithmic_bytes = F * (H * W * 3 + OH * OW * 3)


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


# the copy ceiling: a float4 copy moving the same number of bytes (half read, half written)
n4 = algorithmic_bytes // 2 // 16
src, dst = torch.empty(n4 * 4, dtype=torch.float32, device=dev).normal_(), torch.empty(n4 * 4, dtype=torch.float32, device=dev)
copy_ms, copy_samples = timed(lambda: _hip.check(_hip.lib().vrg_debug_copy_f32(_hip.ptr(src), _hip.ptr(dst), n4 * 4, 1, _hip.current_stream()), "copy"))
del src, dst
rows = {"float4 copy of the algorithmic bytes": {"ms": copy_ms, "samples_ms": copy_samples, "fraction_of_copy_ceiling": 1.0}}


def add(name, fn):
    ms, samples = timed(fn)
    rows[name] = {"ms": ms, "samples_ms": samples, "ms_per_frame": ms / F, "fraction_of_copy_ceiling": copy_ms / ms}
    print(f"{name}: {ms:.3f} ms per {F} frames, {copy_ms / ms:.3f} of the copy ceiling", flush=True)


add("vrg_lanczos4_u8", lambda: ops.resize_frames_u8(x, OW, OH))
for label, intensity in (("grain on", 0.04), ("grain off", 0.0)):
    args = (0.5, True, intensity, 0.5, 42, 0)
    add(f"fused vrg_upscale_sharpen_grain_u8, sharpen on, {label}", lambda: ops.upscale_sharpen_then_seeded_grain(x, OW, OH, *args))
    add(f"two launches (vrg_lanczos4_u8 + sharpen_then_seeded_grain), sharpen on, {label}",
        lambda: ops.sharpen_then_seeded_grain(ops.resize_frames_u8(x, OW, OH), *args))
del x
torch.cuda.empty_cache()

# host-fed
n = a.host_frames
rng = np.random.Generator(np.random.PCG64(1))
small = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]
big = [rng.integers(0, 256, (OH, OW, 3), dtype=np.uint8) for _ in range(n)]
host = {}
for label, settings in (("grain on", {"sharpen_enabled": True, "grain_enabled": True}), ("grain off", {"sharpen_enabled": True, "grain_enabled": False})):
    def new_route():
        return E._tensor_to_frames(E._enhance_decoded(small, OW, OH, settings, 0))

    def old_route():
        return E._tensor_to_frames(E._apply_effects_batch(E._frames_to_tensor(big), settings, 0))

    for name, fn in ((f"_enhance_decoded from 1080p host frames, {label}", new_route), (f"pre-upscaled 4K host frames through _apply_effects_batch, {label}", old_route)):
        fn()
        torch.cuda.synchronize()
        samples = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - t0) * 1e3)
        host[name] = {"ms": statistics.median(samples), "samples_ms": samples, "frames": n}
        print(f"{name}: {host[name]['ms']:.2f} ms per {n} frames", flush=True)

result = {"workload": f"{W}x{H} -> {OW}x{OH}, uniform-random bytes, {F} frames resident", "device": torch.cuda.get_device_name(0),
          "algorithmic_bytes": algorithmic_bytes, "bytes_per_output_pixel": 3.75, "reps": a.reps, "rounds": a.rounds,
          "enhance_decoded_routes": {"with grain": "fused" if E.FUSED_UPSCALE_WITH_GRAIN else "two launches",
                                     "without grain": "fused" if E.FUSED_UPSCALE_WITHOUT_GRAIN else "two launches"},
          "device_resident": rows, "host_fed": host}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print("wrote", a.out)

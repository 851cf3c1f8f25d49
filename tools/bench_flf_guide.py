"""The LTX First / Last guide, timed: two pictures -> 121 frames of 1280 x 736 and 257 frames of 1920 x 1080, `last` a 4000 x 3000 picture
(centre-cropped and resampled) or a picture of the frame size (taken as it is).

    python tools/bench_flf_guide.py [--rounds 8] [--reps 3] [--out profiles/flf_guide.json]

Device-resident (HIP events around `--reps` calls; two warm-up rounds, then the candidates alternate inside every round, median of
`--rounds`), side by side in the same run:
  (a) vrg_flf_guide_f32 alone (weights already on the device);
  (b) a non-temporal float4 fill of the same output bytes (vrg_debug_copy_f32 mode 4): the write ceiling the launch is bounded by;
  (c) the reference's own sequence as eager torch ops on the same device tensors: F.interpolate of the narrowed channels-last view, per
      frame first * (1.0 - amount) + last * amount, torch.cat;
  and ops.flf_guide_frames from resident pictures (the launch plus its host plan and the upload of the weights).
Host-fed (wall clock ending in a device synchronise):
  (d) ops.flf_guide_frames from two CPU pictures, against the reference's loop on this machine's CPU (interpolate, per-frame blend, cat)
      followed by the upload of the finished batch."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flf_guide.json"))
a = ap.parse_args()

load_package()
from comfyui_vrgamedevgirl_amd import _hip, ops  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_flf_guide: no GPU visible; nothing is measured without one")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
SRC_W, SRC_H, WARMUP = 4000, 3000, 2
gen = torch.Generator().manual_seed(3)


def interleaved(candidates):
    """{name: (median ms, samples)}: every round times each candidate once, `reps` calls between two events"""
    for _ in range(WARMUP):
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


def wall(fn, rounds, warm=True):
    if warm:
        fn()
        torch.cuda.synchronize()
    samples = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3)
    return {"ms": statistics.median(samples), "samples_ms": samples}


def reference_sequence(first, last, amounts):
    """the reference's expressions on whatever device the pictures live on"""
    h, w = int(first.shape[1]), int(first.shape[2])
    if (int(last.shape[1]), int(last.shape[2])) != (h, w):
        x, y, rw, rh = ops.center_crop_rect(int(last.shape[2]), int(last.shape[1]), w, h)
        view = last.movedim(-1, 1).narrow(-2, y, rh).narrow(-1, x, rw)
        last = F.interpolate(view, size=(h, w), mode="bilinear").movedim(1, -1)
    return torch.cat([first * (1.0 - amount) + last * amount for amount in amounts], dim=0)


sizes = {}
for width, height, frames in ((1280, 736, 121), (1920, 1080, 257)):
    for leg, last_shape in (("resampled", (1, SRC_H, SRC_W, 3)), ("plain", (1, height, width, 3))):
        label = f"{width}x{height}x{frames}, last {last_shape[2]}x{last_shape[1]} ({leg})"
        out_bytes = frames * height * width * 12
        host_first, host_last = torch.rand((1, height, width, 3), generator=gen), torch.rand(last_shape, generator=gen)
        first, last = host_first.to(dev), host_last.to(dev)
        rect, weights = ops.flf_plan(first.shape[1:], last.shape[1:], frames)
        amounts = [float(v) for v in weights[:, 1].astype("float64")]          # the fp32 weights as doubles: the sequence is timed, not compared bit for bit
        wd = torch.from_numpy(weights).to(dev)
        out = torch.empty((frames, height, width, 3), dtype=torch.float32, device=dev)
        fill = torch.empty(out.numel(), dtype=torch.float32, device=dev)

        def launch():
            _hip.check(_hip.lib().vrg_flf_guide_f32(_hip.ptr(first), _hip.ptr(last), _hip.ptr(wd), _hip.ptr(out), frames, height, width, 3,
                                                    last_shape[1], last_shape[2], *rect, _hip.current_stream()), "vrg_flf_guide_f32")

        def write_ceiling():
            _hip.check(_hip.lib().vrg_debug_copy_f32(_hip.ptr(fill), _hip.ptr(fill), fill.numel(), 4, _hip.current_stream()), "fill")

        def eager():
            return reference_sequence(first, last, amounts)

        def whole_op():
            return ops.flf_guide_frames(first, last, frames, out=out)

        launch()
        worst = float((out - eager()).abs().max())                             # the device's own interpolate is not the CPU kernel: a few ulp
        res = interleaved({"(a) vrg_flf_guide_f32": launch, "(b) non-temporal float4 fill of the output bytes": write_ceiling,
                           "(c) the reference's sequence as eager torch ops on the device": eager,
                           "ops.flf_guide_frames, resident pictures": whole_op})
        ceiling = res["(b) non-temporal float4 fill of the output bytes"][0]
        rows = {}
        for name, (ms, s) in res.items():
            rows[name] = {"ms": ms, "samples_ms": s, "output_TB_per_s": out_bytes / ms / 1e9, "fraction_of_write_ceiling": ceiling / ms}
            print(f"{label}: {name}: {ms:.3f} ms, {out_bytes / ms / 1e9:.2f} TB/s of output, {ceiling / ms:.3f} of the fill", flush=True)
        del fill, out
        torch.cuda.empty_cache()
        host = {"(d) ops.flf_guide_frames from two CPU pictures": wall(lambda: ops.flf_guide_frames(host_first, host_last, frames), a.host_rounds),
                "(d) the reference's loop on this CPU plus the upload of the finished batch":
                    wall(lambda: reference_sequence(host_first, host_last, amounts).to(dev), a.host_rounds, warm=False)}
        for name, row in host.items():
            print(f"{label}: {name}: {row['ms']:.1f} ms", flush=True)
        sizes[label] = {"output_bytes": out_bytes, "rectangle": list(rect), "largest_difference_from_the_eager_device_sequence": worst,
                        "device_resident": rows, "host_fed": host}
        torch.cuda.empty_cache()

result = {"workload": f"uniform-random fp32 pictures; last {SRC_W}x{SRC_H} (resampled) or of the frame size (plain); default transition and curve",
          "device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "warmup_rounds": WARMUP, "host_rounds": a.host_rounds,
          "cpu_threads": torch.get_num_threads(), "sizes": sizes}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print("wrote", a.out)

"""Time the Builder Face Fix kernels on the GPU and write profiles/facefix_builder.json.

    python tools/bench_facefix_builder.py [--frames 256] [--height 2160] [--width 3840] [--repeats 7] [--warmup 2]

256 4K byte frames in HBM, one box per frame: all 256 px, all 1024 px, and a mixed 128 ... 2160 px set; 512 x 512 repaired frames; feather
18, colour match 0.65.  Every launch is timed with HIP events after a warm-up and the median of the repeats is kept: the masks, the resize
+ statistics and the composite pass separately, the prepare-side crop (vrg_lanczos4_boxes_u8 to 512 x 512) as well, each beside a byte copy
(torch's device-to-device copy_) of the same frames timed in the same run.  The composite pass is also given in algorithmic TB/s at
6 B/px (3 in, 3 out).  A host-fed leg runs composite_frames on 16 CPU frames (wall clock around a synchronise: upload, kernels, download).
No GPU: the tool fails; it does not fall back."""
from __future__ import annotations

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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, repeats, warmup, ops):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = ops.HipEvent(), ops.HipEvent()
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_ms(stop))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def box_sets(frames, height, width):
    rng = np.random.Generator(np.random.PCG64(11))

    def place(side):
        left, top = int(rng.integers(0, width - side + 1)), int(rng.integers(0, height - side + 1))
        return (left, top, left + side, top + side)

    mixed = [int(v) for v in np.linspace(128, min(height, width), 13)]
    return {"256": [place(256) for _ in range(frames)], "1024": [place(min(1024, height, width)) for _ in range(frames)],
            "mixed_128_2160": [place(mixed[f % len(mixed)]) for f in range(frames)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "facefix_builder.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_facefix_builder: no GPU visible; nothing is measured without one")
    from conftest import load_package
    load_package()
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix as FF
    from comfyui_vrgamedevgirl_amd import ops

    F, H, W = args.frames, args.height, args.width
    gen = torch.Generator(device="cuda").manual_seed(5)
    frames = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
    enhanced = torch.randint(0, 256, (F, 512, 512, 3), dtype=torch.uint8, device="cuda", generator=gen)
    other = torch.empty_like(frames)
    pixels = F * H * W
    result = {"frames": F, "height": H, "width": W, "enhanced": [512, 512], "feather": 18, "color_match": 0.65, "repeats": args.repeats,
              "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "sets": {}}
    copy = timed(lambda: other.copy_(frames), args.repeats, args.warmup, ops)
    copy["TBps_at_6_B_per_px"] = pixels * 6 / copy["median_ms"] / 1e9
    result["byte_copy_of_the_frames"] = copy
    for name, boxes in box_sets(F, H, W).items():
        plan = FF.CompositePlan(frames, enhanced, FF._boxes(boxes, F, H, W), [1.0] * F, True, 18, 0.65)
        entry = {"box_pixels": int(sum((b[2] - b[0]) * (b[3] - b[1]) for b in boxes)), "distinct_masks": len(plan.records)}
        entry["masks"] = timed(plan.run_masks, args.repeats, args.warmup, ops)
        entry["resize_stats"] = timed(plan.run_resize_stats, args.repeats, args.warmup, ops)
        comp = timed(plan.run_composite, args.repeats, args.warmup, ops)
        comp["TBps_at_6_B_per_px"] = pixels * 6 / comp["median_ms"] / 1e9
        comp["share_of_the_byte_copy"] = copy["median_ms"] / comp["median_ms"]
        entry["composite"] = comp
        entry["whole_call"] = timed(lambda: FF.composite_frames(frames, enhanced, boxes, 1.0, 18, 0.65), max(3, args.repeats // 2), 1, ops)
        entry["crop_to_512"] = timed(lambda: FF.crop_frames(frames, boxes, 512), args.repeats, args.warmup, ops)
        result["sets"][name] = entry
        del plan
        print(name, json.dumps(entry), flush=True)
    # host-fed: 16 CPU frames, a 1024 px box each
    n = min(16, F)
    cpu_frames, cpu_enh = frames[:n].cpu(), enhanced[:n].cpu()
    boxes = box_sets(n, H, W)["1024"]
    walls = []
    for i in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        FF.composite_frames(cpu_frames, cpu_enh, boxes, 1.0, 18, 0.65)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    result["host_fed_16_frames_1024_box"] = {"wall_ms": walls[1:], "median_ms": statistics.median(walls[1:]), "first_call_ms": walls[0]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result["byte_copy_of_the_frames"]), json.dumps(result["host_fed_16_frames_1024_box"]))


if __name__ == "__main__":
    main()

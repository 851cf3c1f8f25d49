"""Time the far-face repair composite kernels on the GPU and write profiles/far_face.json.

    python tools/bench_far_face.py [--frames 256] [--height 2160] [--width 3840] [--repeats 7] [--warmup 2]

256 4K byte frames in HBM, one box per frame: all 256 px, all 1024 px, and a mixed 128 ... 2160 px set; 512 x 512 repaired crops; feather
18, colour match on.  Every launch is timed with HIP events after a warm-up and the median of the repeats is kept: the Pillow resize, the
masks, the means kernel on its own line and the paste pass, beside a byte copy (torch's device-to-device copy_) of the same frames and
beside vrg_ff_composite_u8 (the Builder's composite pass) at the same geometry, all in the same run.  The paste pass is also given in
algorithmic TB/s at 6 B/px (3 in, 3 out).  No GPU: the tool fails; it does not fall back."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "far_face.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_far_face: no GPU visible; nothing is measured without one")
    from conftest import load_package
    load_package()
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix as FF
    from comfyui_vrgamedevgirl_amd import far_face_repair as FR
    from comfyui_vrgamedevgirl_amd import ops

    F, H, W = args.frames, args.height, args.width
    gen = torch.Generator(device="cuda").manual_seed(5)
    frames = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
    repaired = torch.randint(0, 256, (F, 512, 512, 3), dtype=torch.uint8, device="cuda", generator=gen)
    crops = [repaired[f] for f in range(F)]
    other = torch.empty_like(frames)
    pixels = F * H * W
    result = {"frames": F, "height": H, "width": W, "repaired": [512, 512], "feather": 18, "color_match": True, "repeats": args.repeats,
              "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "sets": {}}
    copy = timed(lambda: other.copy_(frames), args.repeats, args.warmup, ops)
    copy["TBps_at_6_B_per_px"] = pixels * 6 / copy["median_ms"] / 1e9
    result["byte_copy_of_the_frames"] = copy
    for name, boxes in box_sets(F, H, W).items():
        plan = FR.CompositePlan(frames, FF._boxes(boxes, F, H, W), crops, 18, True)
        entry = {"box_pixels": int(sum((b[2] - b[0]) * (b[3] - b[1]) for b in boxes)), "distinct_masks": plan.mask_plan.n}
        entry["pil_resize"] = timed(plan.run_resize, args.repeats, args.warmup, ops)
        entry["masks"] = timed(plan.run_masks, args.repeats, args.warmup, ops)
        entry["means"] = timed(plan.run_means, args.repeats, args.warmup, ops)
        paste = timed(plan.run_paste, args.repeats, args.warmup, ops)
        paste["TBps_at_6_B_per_px"] = pixels * 6 / paste["median_ms"] / 1e9
        paste["share_of_the_byte_copy"] = copy["median_ms"] / paste["median_ms"]
        entry["paste"] = paste
        del plan
        builder = FF.CompositePlan(frames, repaired, FF._boxes(boxes, F, H, W), [1.0] * F, True, 18, 0.65)
        builder.run_masks()
        builder.run_resize_stats()
        comp = timed(builder.run_composite, args.repeats, args.warmup, ops)
        comp["share_of_the_byte_copy"] = copy["median_ms"] / comp["median_ms"]
        entry["vrg_ff_composite_u8_same_geometry"] = comp
        del builder
        result["sets"][name] = entry
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result["byte_copy_of_the_frames"]))


if __name__ == "__main__":
    main()

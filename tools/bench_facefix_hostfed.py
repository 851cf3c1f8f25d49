"""Time the Builder Face Fix as its routes call it -- decoded frames on the HOST -- and write profiles/facefix_hostfed.json.

    python tools/bench_facefix_hostfed.py [--frames 16] [--height 2160] [--width 3840] [--rounds 7] [--warmup 2]

16 CPU 4K byte frames (a list of numpy arrays, as cv2 hands them over), one box per frame at three geometries: all 256 px, all 1024 px and
a mixed 128 ... 2160 px set; 512 x 512 repaired frames, feather 18, colour match 0.65.  Per geometry the wall time (a host clock around
the call and a device synchronise: gather, upload, kernels, download, paste) of
    crop_frames_packed / composite_frames_packed (a copy of the originals) / composite_frames_packed(inplace=True)
beside the unchanged whole-frame crop_frames / composite_frames in the same process, the order rotated every round; median, min and max
of the rounds after the warm-up rounds, and the bytes each way from last_transfer().  The packed results are compared with the whole-frame
results once, byte for byte.  No GPU: the tool fails; it does not fall back."""
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


def box_sets(frames, height, width):
    rng = np.random.Generator(np.random.PCG64(11))

    def place(side):
        left, top = int(rng.integers(0, width - side + 1)), int(rng.integers(0, height - side + 1))
        return (left, top, left + side, top + side)

    mixed = [int(v) for v in np.linspace(128, min(height, width), 13)]
    return {"256": [place(min(256, height, width)) for _ in range(frames)], "1024": [place(min(1024, height, width)) for _ in range(frames)],
            "mixed_128_2160": [place(mixed[f % len(mixed)]) for f in range(frames)]}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "rounds": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--enhance", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "facefix_hostfed.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_facefix_hostfed: no GPU visible; nothing is measured without one")
    if args.rounds < 7 or args.warmup < 2:
        raise SystemExit("bench_facefix_hostfed: at least 7 rounds after 2 warm-up rounds")
    from conftest import load_package
    load_package()
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix as FF

    F, H, W, S = args.frames, args.height, args.width, args.enhance
    rng = np.random.Generator(np.random.PCG64(5))
    frames = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(F)]
    scratch = [f.copy() for f in frames]                                    # what the in-place leg pastes into
    enhanced = [rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8) for _ in range(F)]
    result = {"frames": F, "height": H, "width": W, "enhanced": [S, S], "feather": 18, "color_match": 0.65, "rounds": args.rounds,
              "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "frame_bytes": F * H * W * 3,
              "clock": "host perf_counter around the call and a device synchronise", "sets": {}}
    for name, boxes in box_sets(F, H, W).items():
        plan = FF.packed_plan(F, H, W, boxes, 1.0)
        moved = {}

        def crop_packed():
            FF.crop_frames_packed(frames, boxes, S)
            moved["crop"] = FF.last_transfer()

        def composite_packed():
            FF.composite_frames_packed(frames, enhanced, boxes, 1.0, 18, 0.65)
            moved["composite"] = FF.last_transfer()

        legs = {"crop_frames": lambda: FF.crop_frames(frames, boxes, S),
                "crop_frames_packed": crop_packed,
                "composite_frames": lambda: FF.composite_frames(frames, enhanced, boxes, 1.0, 18, 0.65),
                "composite_frames_packed": composite_packed,
                "composite_frames_packed_inplace": lambda: FF.composite_frames_packed(scratch, enhanced, boxes, 1.0, 18, 0.65, inplace=True)}
        same_crop = np.array_equal(np.stack(FF.crop_frames_packed(frames, boxes, S)), np.stack(FF.crop_frames(frames, boxes, S)))
        same_composite = all(np.array_equal(a, b) for a, b in zip(FF.composite_frames_packed(frames, enhanced, boxes, 1.0, 18, 0.65),
                                                                  FF.composite_frames(frames, enhanced, boxes, 1.0, 18, 0.65)))
        names, times = list(legs), {leg: [] for leg in legs}
        for r in range(args.warmup + args.rounds):
            order = names[r % len(names):] + names[:r % len(names)]          # rotated: no leg always runs behind the same one
            for leg in order:
                t = wall_ms(legs[leg])
                if r >= args.warmup:
                    times[leg].append(t)
        entry = {"box_pixels": int(sum(w * h for _, _, w, h in plan.boxes)), "box_bytes": plan.bytes_up,
                 "share_of_the_frame_bytes": plan.bytes_up / plan.frame_bytes, "tiles": plan.tiles,
                 "packed_equals_whole_frame": {"crop": bool(same_crop), "composite": bool(same_composite)},
                 "bytes_moved": {"crop_frames": {"up": plan.frame_bytes, "down": F * S * S * 3},
                                 "crop_frames_packed": moved["crop"],
                                 "composite_frames": {"up": plan.frame_bytes + F * S * S * 3, "down": plan.frame_bytes},
                                 "composite_frames_packed": moved["composite"]}}
        entry.update({leg: summary(times[leg]) for leg in names})
        for packed, whole in (("crop_frames_packed", "crop_frames"), ("composite_frames_packed", "composite_frames"),
                              ("composite_frames_packed_inplace", "composite_frames")):
            entry[packed]["whole_frame_median_over_this_median"] = entry[whole]["median_ms"] / entry[packed]["median_ms"]
            entry[packed]["slower_by_more_than_the_whole_frame_spread"] = bool(
                entry[packed]["median_ms"] - entry[whole]["median_ms"] > entry[whole]["max_ms"] - entry[whole]["min_ms"])
        result["sets"][name] = entry
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

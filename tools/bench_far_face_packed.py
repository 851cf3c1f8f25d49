"""Time the far-face repair composite as the reference calls it -- decoded frames on the HOST -- and write profiles/far_face_packed.json.

    python tools/bench_far_face_packed.py [--frames 64] [--rounds 7] [--warmup 2]

64 pageable CPU byte frames (a list of numpy arrays, as ``Image.open`` hands them over) at 1080p and again at 4K, one square box per frame
of 32 ... 320 px, repaired crops of 512 x 512, feather 18, colour match on.  Per size the wall time (a host clock around the call and a
device synchronise: gather, upload, kernels, download, paste; the result on the host on both sides) of
    composite_frames_packed (a copy of the originals) / composite_frames_packed(inplace=True)
beside the unchanged whole-frame composite_frames on the same CPU batch, alternated in one process; best, median and spread of the rounds
after the warm-up rounds, and the bytes each way from last_transfer().  What must hold is asserted from the byte counts, not from time: the
packed route moves the boxes' bytes each way and nothing of the frames.  The packed results are compared with the whole-frame results
once, byte for byte.  No GPU: the tool fails; it does not fall back."""
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

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}


def boxes_for(frames, height, width):
    rng = np.random.Generator(np.random.PCG64(17))
    sides = [int(v) for v in np.linspace(32, 320, frames)]
    out = []
    for side in sides:
        left, top = int(rng.integers(0, width - side + 1)), int(rng.integers(0, height - side + 1))
        out.append((left, top, left + side, top + side))
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(times):
    return {"best_ms": min(times), "median_ms": statistics.median(times), "max_ms": max(times), "spread_ms": max(times) - min(times),
            "rounds": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--crop", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "far_face_packed.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_far_face_packed: no GPU visible; nothing is measured without one")
    if args.rounds < 7 or args.warmup < 1:
        raise SystemExit("bench_far_face_packed: at least 7 rounds after a warm-up round")
    from conftest import load_package
    load_package()
    from comfyui_vrgamedevgirl_amd import far_face_repair as FR

    F, S = args.frames, args.crop
    result = {"frames": F, "repaired": [S, S], "feather": 18, "color_match": True, "rounds": args.rounds, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "tile": FR._hip.PIL_PACKED_TILE,
              "clock": "host perf_counter around the call and a device synchronise; pageable numpy frames in, numpy frames out", "sizes": {}}
    for name in args.sizes.split(","):
        H, W = SIZES[name]
        rng = np.random.Generator(np.random.PCG64(5))
        frames = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(F)]
        scratch = [f.copy() for f in frames]                                # what the in-place leg pastes into
        repaired = [rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8) for _ in range(F)]
        boxes = boxes_for(F, H, W)
        plan = FR.packed_plan(F, H, W, boxes)
        moved = {}

        def packed():
            FR.composite_frames_packed(frames, repaired, boxes, 18, True)
            moved["composite_frames_packed"] = FR.last_transfer()

        legs = {"composite_frames": lambda: FR.composite_frames(frames, repaired, boxes, 18, True),
                "composite_frames_packed": packed,
                "composite_frames_packed_inplace": lambda: FR.composite_frames_packed(scratch, repaired, boxes, 18, True, inplace=True)}
        whole = FR.composite_frames(frames, repaired, boxes, 18, True)
        same = all(np.array_equal(a, b) for a, b in zip(FR.composite_frames_packed(frames, repaired, boxes, 18, True), whole))
        del whole
        names, times = list(legs), {leg: [] for leg in legs}
        for r in range(args.warmup + args.rounds):
            order = names[r % len(names):] + names[:r % len(names)]          # alternated: no leg always runs behind the same one
            for leg in order:
                t = wall_ms(legs[leg])
                if r >= args.warmup:
                    times[leg].append(t)
        up = moved["composite_frames_packed"]
        # what is derivable and must hold: the boxes' bytes each way, nothing of the frames
        assert up["bytes_up"] == up["bytes_down"] == plan.bytes_up == sum(w * h * 3 for _, _, w, h in plan.boxes), up
        assert up["repaired_up"] == F * S * S * 3 and plan.bytes_up < plan.frame_bytes, up
        assert same, "the packed route and the whole-frame route gave different bytes"
        entry = {"height": H, "width": W, "box_sides": [b[2] - b[0] for b in boxes][::max(1, F // 8)], "box_bytes": plan.bytes_up,
                 "frame_bytes": plan.frame_bytes, "share_of_the_frame_bytes": plan.bytes_up / plan.frame_bytes, "tiles": plan.tiles,
                 "packed_equals_whole_frame": bool(same),
                 "bytes_moved": {"composite_frames": {"up": plan.frame_bytes + F * S * S * 3, "down": plan.frame_bytes},
                                 "composite_frames_packed": up}}
        entry.update({leg: summary(times[leg]) for leg in names})
        for leg in ("composite_frames_packed", "composite_frames_packed_inplace"):
            entry[leg]["whole_frame_median_over_this_median"] = entry["composite_frames"]["median_ms"] / entry[leg]["median_ms"]
        entry["host_copy_share_of_the_packed_median"] = 1.0 - entry["composite_frames_packed_inplace"]["median_ms"] / \
            entry["composite_frames_packed"]["median_ms"]
        result["sizes"][name] = entry
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

"""The music-video assembly against the path it replaces, on the GPU, alternating in one process.

    python tools/measure_assemble.py [--clips 16] [--frames 97] [--height 1080] [--width 1920] [--rounds 7] [--out profiles/assemble.json]

Workload: `clips` device-resident fp32 clips of `frames` x height x width x 3, trimmed to mixed targets (V5's plan).  New: ONE launch of
ops.assemble_labelled_bytes -- the joined fp32 batch and the labelled B,G,R bytes; also ops.assemble_frames alone.  Parent path: the same
products from the pack without this kernel: torch.cat of device slices, and the reference's label expressions written in torch on the
device (x * 255 -> uint8, flip, bar, flip, / 255, cat, * 255 -> uint8, flip).  A plain device copy of the joined batch (Tensor.copy_) runs
beside them as the yardstick of a streaming copy.  Times are device events around a call, best and median of `rounds` alternated rounds
after a warm-up.  The outputs of both sides are compared first.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=97)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_assemble: needs the GPU; nothing is measured without one")
    import __graft_entry__ as entry
    entry.load_package()
    from comfyui_vrgamedevgirl_amd import ops

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    clips = [torch.rand((a.frames, a.height, a.width, 3), generator=g, device=dev) for _ in range(a.clips)]
    targets = [max(1, a.frames - (i * 7) % 40) for i in range(a.clips)]                    # 97, 90, 83, ... : mixed trims
    meta = {"durations_frames": targets}
    plan = ops.assemble_plan("v5", [tuple(c.shape) for c in clips], 25.0, meta)
    n_out = len(plan)
    bar = ops.ASSEMBLE_BAR

    def new_both(cs):
        return ops.assemble_labelled_bytes(cs, plan, None, clean_out=True)

    def new_join(cs):
        return ops.assemble_frames(cs, plan)

    def old_join(cs):
        return torch.cat([c[:t] for c, t in zip(cs, targets)], dim=0)

    def old_both(cs):
        final = old_join(cs)
        labelled = []
        for c, t in zip(cs, targets):
            bgr = (c[:t] * 255).to(torch.uint8).flip(-1)
            framed = torch.zeros((t, a.height + bar, a.width, 3), dtype=torch.uint8, device=c.device)
            framed[:, :a.height] = bgr
            labelled.append(framed.flip(-1).to(torch.float32) / 255.0)
        video = torch.cat(labelled, dim=0)
        return (video * 255).to(torch.uint8).flip(-1), final

    def timed(fn, *args):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        out = fn(*args)
        stop.record()
        torch.cuda.synchronize()
        del out
        return start.elapsed_time(stop)

    def alternate(sides, *args):
        for fn in sides.values():                                   # warm-up: code objects, allocator
            timed(fn, *args)
            timed(fn, *args)
        times = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, fn in sides.items():
                times[k].append(timed(fn, *args))
        return {k: {"best_ms": min(v), "median_ms": statistics.median(v), "worst_ms": max(v), "all_ms": v} for k, v in times.items()}

    small = [c[:5, :64, :64].contiguous() for c in clips[:3]]
    small_plan = ops.assemble_plan("v5", [tuple(c.shape) for c in small], 25.0, {"durations_frames": [5, 3, 4]})
    got = ops.assemble_labelled_bytes(small, small_plan, None, clean_out=True)
    final = torch.cat([c[:t] for c, t in zip(small, (5, 3, 4))])
    u8 = (final * 255).to(torch.uint8).flip(-1).to(torch.float32).flip(-1) / 255.0
    want = torch.zeros((12, 64 + bar, 64, 3), dtype=torch.uint8, device=dev)
    want[:, :64] = (u8 * 255).to(torch.uint8).flip(-1)
    same = bool(torch.equal(got[0], want) and torch.equal(got[1], final))

    frame = a.height * a.width * 3
    bytes_join = n_out * frame * 8
    bytes_both = bytes_join + n_out * (a.height + bar) * a.width * 3
    result = {
        "workload": {"clips": a.clips, "frames": a.frames, "frame": [a.height, a.width, 3], "targets": targets, "output_frames": n_out,
                     "device": torch.cuda.get_device_name(0)},
        "outputs_equal": same,
        "both_products": alternate({"assemble_labelled_bytes": new_both, "parent_path": old_both}, clips),
        "clean_join": alternate({"assemble_frames": new_join, "torch_cat": old_join}, clips),
        "bytes": {"clean_join": bytes_join, "both_products": bytes_both},
    }
    joined = new_join(clips)
    target = torch.empty_like(joined)
    result["device_copy_of_the_joined_batch"] = alternate({"copy_": lambda cs: target.copy_(joined)}, clips)
    gbs = lambda nbytes, ms: nbytes / ms / 1e6
    result["gb_per_s"] = {
        "assemble_labelled_bytes": gbs(bytes_both, result["both_products"]["assemble_labelled_bytes"]["best_ms"]),
        "assemble_frames": gbs(bytes_join, result["clean_join"]["assemble_frames"]["best_ms"]),
        "torch_cat": gbs(bytes_join, result["clean_join"]["torch_cat"]["best_ms"]),
        "copy_": gbs(bytes_join, result["device_copy_of_the_joined_batch"]["copy_"]["best_ms"]),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"outputs_equal": same, "output_frames": n_out, "gb_per_s": result["gb_per_s"]}))
    for block in ("both_products", "clean_join", "device_copy_of_the_joined_batch"):
        print(block, {k: (round(v["best_ms"], 3), round(v["median_ms"], 3)) for k, v in result[block].items()})


if __name__ == "__main__":
    main()

"""Time the far-face repair contact sheet on the GPU and write profiles/contact_sheet.json.

    python tools/bench_contact_sheet.py [--pairs 24] [--columns 3] [--thumb-width 900] [--repeats 9] [--warmup 2]

24 pairs of 4K and of 1080p byte frames in HBM (originals and fixed frames) -> 3 columns at 900 px.  Both launches are timed with HIP
events after a warm-up and the median of the repeats is kept, beside a byte copy (torch's device-to-device copy_) of the same source bytes
in the same run; launch A is also given in algorithmic TB/s at 3 B per source pixel, read once.  The installed Pillow runs the reference's
loop over the same frames held in memory (no PNG decode) on this machine's CPU in the same run, and a host-fed leg times ``contact_sheet``
on CPU tensors, upload and download included.  The GPU sheet must equal Pillow's.  No GPU: the tool fails; it does not fall back."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=24)
    ap.add_argument("--columns", type=int, default=3)
    ap.add_argument("--thumb-width", type=int, default=900)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contact_sheet.json"))
    args = ap.parse_args()
    if args.repeats < 8:
        raise SystemExit("bench_contact_sheet: at least 8 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_contact_sheet: no GPU visible; nothing is measured without one")
    import contact_sheet_support as S
    from conftest import load_package
    load_package()
    from comfyui_vrgamedevgirl_amd import far_face_repair as FR
    from comfyui_vrgamedevgirl_amd import ops

    device = torch.device("cuda", torch.cuda.current_device())
    result = {"pairs": args.pairs, "columns": args.columns, "thumb_width": args.thumb_width, "repeats": args.repeats, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "sizes": {}}
    gen = torch.Generator(device="cuda").manual_seed(5)
    for name, (H, W) in (("4k", (2160, 3840)), ("1080p", (1080, 1920))):
        originals = torch.randint(0, 256, (args.pairs, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
        fixed = torch.randint(0, 256, (args.pairs, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
        other = torch.empty_like(originals)
        source_bytes = 2 * originals.numel()
        lefts, rights = [originals[i] for i in range(args.pairs)], [fixed[i] for i in range(args.pairs)]
        requests = [(args.thumb_width, int(args.thumb_width * H / (2 * W)))] * args.pairs
        plan = FR.ThumbPlan(lefts, rights, requests, device, columns=args.columns)
        e = plan.entries_host[0]
        entry = {"height": H, "width": W, "source_bytes": source_bytes, "factors": [int(e["fx"]), int(e["fy"])],
                 "thumbnail": [int(e["out_w"]), int(e["out_h"])], "sheet": [plan.width, plan.height], "segments_per_row": plan.max_segments}
        copy = timed(lambda: (other.copy_(originals), other.copy_(fixed)), args.repeats, args.warmup, ops)
        copy["TBps_read"] = source_bytes / copy["median_ms"] / 1e9
        entry["byte_copy_of_the_source_bytes"] = copy
        rows = timed(plan.run_rows, args.repeats, args.warmup, ops)
        rows["TBps_at_3_B_per_source_px"] = source_bytes / rows["median_ms"] / 1e9
        entry["launch_a_rows"] = rows
        entry["launch_b_compose"] = timed(plan.run_compose, args.repeats, args.warmup, ops)
        sheet = plan.run_compose().cpu().numpy()
        o_host, f_host = originals.cpu(), fixed.cpu()
        t0 = time.perf_counter()
        fed = FR.contact_sheet(o_host, f_host, args.pairs, args.columns, args.thumb_width)
        entry["host_fed_contact_sheet_ms"] = (time.perf_counter() - t0) * 1e3
        o_np, f_np = list(o_host.numpy()), list(f_host.numpy())
        t0 = time.perf_counter()
        want = S.pillow_sheet(o_np, f_np, args.pairs, args.columns, args.thumb_width)
        entry["pillow_reference_loop_ms"] = (time.perf_counter() - t0) * 1e3
        entry["equals_pillow"] = bool(np.array_equal(sheet, want) and np.array_equal(fed.numpy(), want))
        entry["gpu_both_launches_ms"] = rows["median_ms"] + entry["launch_b_compose"]["median_ms"]
        result["sizes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del originals, fixed, other, plan
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    if not all(v["equals_pillow"] for v in result["sizes"].values()):
        raise SystemExit("bench_contact_sheet: the GPU sheet differs from Pillow's")


if __name__ == "__main__":
    main()

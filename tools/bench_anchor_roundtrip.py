"""Measure the two launches of the anchor round trip on an MI355X and write profiles/anchor_roundtrip.json.

    python tools/bench_anchor_roundtrip.py [--rounds 8] [--reps 3] [--out profiles/anchor_roundtrip.json]

Shapes: 17 anchors of 768 x 432 and of 1920 x 1080, 65 of 512 x 512, each from stills that already have the size (the copy route) and
from 4000 x 3000 stills (both Lanczos passes).  Every launch is timed by HIP events (median of the rounds after a warm-up, `reps` calls
between two events) in the SAME run beside
  load    a non-temporal float4 fill of the output's bytes (vrg_debug_copy_f32, mode 4), and the reference's sequence on this machine's
          CPU: the Pillow LANCZOS loop, float32 / 255.0, and the upload of the fp32 batch;
  store   a non-temporal copy of the same number of bytes moved (fp32 in + bytes out, vrg_debug_copy_f32, mode 1), and the reference's
          sequence: the fp32 download and numpy's clip * 255, round, astype per frame.
No threshold is set: the figures are what was found."""
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
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-rounds", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_roundtrip.json"))
a = ap.parse_args()

load_package()
from comfyui_vrgamedevgirl_amd import _hip, ops  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_anchor_roundtrip: no GPU visible; nothing is measured without one")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
rng = np.random.Generator(np.random.PCG64(4))
STILL = (4000, 3000)
SHAPES = ((17, 768, 432), (17, 1920, 1080), (65, 512, 512))


def interleaved(candidates):
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
    return {name: {"ms": statistics.median(s), "samples_ms": s} for name, s in samples.items()}


def wall(fn, rounds):
    samples = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3)
    return {"ms": statistics.median(samples), "samples_ms": samples}


def copy_f32(buf, floats, mode):
    floats -= floats % 4
    return lambda: _hip.check(_hip.lib().vrg_debug_copy_f32(_hip.ptr(buf), _hip.ptr(buf[floats:]) if mode == 1 else _hip.ptr(buf), floats, mode,
                                                            _hip.current_stream()), "vrg_debug_copy_f32")


def reference_load(stills, size):
    from PIL import Image
    batch = np.stack([np.asarray(Image.fromarray(s).resize(size, Image.Resampling.LANCZOS), dtype=np.float32) / 255.0 for s in stills])
    return torch.from_numpy(batch).to(dev)


def reference_store(images):
    host = images.cpu()
    return [(frame[..., :3].clamp(0, 1).numpy() * 255).round().astype("uint8") for frame in host]


result = {"device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "reps": a.reps, "load": {}, "store": {}}
for n, width, height in SHAPES:
    out = torch.empty((n, height, width, 3), dtype=torch.float32, device=dev)
    scratch = torch.empty(2 * out.numel() + 64, dtype=torch.float32, device=dev)
    for source, size in (("equal", (width, height)), ("4000x3000", STILL)):
        label = f"{n}x{width}x{height} from {source}"
        distinct = [rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8) for _ in range(2)]
        stills = [distinct[i % 2] for i in range(n)]
        shapes = [s.shape[:2] for s in stills]
        desc, tables, src_bytes, _ = ops.anchor_plan(shapes, (width, height))
        pair = torch.cat([torch.from_numpy(s).reshape(-1) for s in distinct]).to(dev)                   # the records of n stills over two pictures
        desc["src_offset"] = [(i % 2) * distinct[0].size for i in range(n)]
        ops.anchor_check(desc, tables, pair.numel(), height, width)
        table = _hip.upload_records(desc, dev, trailing=(tables,))
        tab = (table.data_ptr() + len(desc) * ops.ANCHOR_DESC.itemsize) if tables.size else None

        def launch():
            _hip.check(_hip.lib().vrg_anchor_frames_f32(_hip.ptr(pair), pair.numel(), _hip.ptr(table), n, tab, int(tables.size), _hip.ptr(out),
                                                        height, width, _hip.current_stream()), "vrg_anchor_frames_f32")

        launch()
        check = ops.anchor_frames(stills[:2], size=(width, height))
        rec = interleaved({"launch": launch, "fill": copy_f32(scratch, out.numel(), 4)})
        rec["bits_equal_whole_op"] = bool(torch.equal(out[:2].view(torch.int32), check.view(torch.int32)))
        rec["whole_op_host_fed_wall"] = wall(lambda: ops.anchor_frames(stills, size=(width, height)), 3)
        rec["reference_cpu_wall"] = wall(lambda: reference_load(stills, (width, height)), a.host_rounds)
        rec["output_bytes"] = out.numel() * 4
        rec["launch_over_fill"] = rec["launch"]["ms"] / rec["fill"]["ms"]
        result["load"][label] = rec
        print(label, {k: (round(v["ms"], 4) if isinstance(v, dict) else v) for k, v in rec.items()}, flush=True)
    for channels in (3, 4):
        label = f"{n}x{width}x{height}x{channels}"
        images = torch.rand((n, height, width, channels), device=dev) * 1.2 - 0.1
        data = torch.empty((n, height, width, 3), dtype=torch.uint8, device=dev)
        moved = images.numel() * 4 + data.numel()
        rec = interleaved({"rgb": lambda: ops.anchor_store_bytes(images, out=data), "bgr": lambda: ops.anchor_store_bytes(images, bgr=True, out=data),
                           "copy": copy_f32(scratch, min(moved // 8, out.numel()), 1)})
        rec["copy_bytes"] = min(moved // 8, out.numel()) // 4 * 4 * 8
        rec["moved_bytes"] = moved
        rec["reference_cpu_wall"] = wall(lambda: reference_store(images), a.host_rounds)
        rec["rgb_bytes_per_s_over_copy"] = (moved / rec["rgb"]["ms"]) / (rec["copy_bytes"] / rec["copy"]["ms"])
        result["store"][label] = rec
        print(label, {k: (round(v["ms"], 4) if isinstance(v, dict) else v) for k, v in rec.items()}, flush=True)
    del out, scratch

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", a.out)

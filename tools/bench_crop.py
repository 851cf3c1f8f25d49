"""Face Fix crop sequence on frames resident in HBM: the one launch (vrg_crop_resize_f32) against the float4 copy ceiling of the same run
and against the reference's sequence restated as eager torch ops on the same device tensors (the per-frame slice / permute / bicubic
interpolate / permute / clamp loop, the hole filling, the prefix and the stack).
    python tools/bench_crop.py [--frames 256] [--iters 20] [--json profiles/crop.json]
Geometry: 4K frames, one box per frame to 512 x 512, three box populations: all 256 px, all 1024 px, mixed 128..2160 px with 10 % holes.
Legs are interleaved round by round after two warm-up rounds; a leg's figure is the median of its timed rounds (HIP events), with the
spread (min, max) beside it.  "launch": the C entry point with its table already on the device; "op": ops.crop_frames (builds and
uploads the table too).  Algorithmic bytes: the boxes read once (12 B per box pixel of every output frame) + the output written.
One host-fed figure at the end: 16 CPU 4K frames, the bytes that crossed to the GPU against the size of the frames."""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package
load_package()
from comfyui_vrgamedevgirl_amd import _hip, ops
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--eager-iters", type=int, default=3)
ap.add_argument("--host-frames", type=int, default=16)
ap.add_argument("--json", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
H, W, SIZE = 2160, 3840, 512
g = torch.Generator(device=dev).manual_seed(5)
frames = torch.rand((a.frames, H, W, 3), generator=g, device=dev)
rng = np.random.Generator(np.random.PCG64(7))


def population(kind, n):
    entries = []
    for i in range(n):
        if kind == "mixed" and i % 10 == 3:
            entries.append({"box": None})
            continue
        side = {"box256": 256, "box1024": 1024}.get(kind) or int(rng.integers(128, H + 1))
        left, top = int(rng.integers(0, W - side + 1)), int(rng.integers(0, H - side + 1))
        entries.append({"box": (left, top, left + side, top + side)})
    return entries


def eager_sequence(entries):
    """The crop lines of the reference's Prepare nodes as eager torch ops on the device tensors: one Python iteration per frame."""
    crops = []
    for index, entry in enumerate(entries):
        crop = None
        if entry["box"]:
            left, top, right, bottom = entry["box"]
            item = frames[index:index + 1, top:bottom, left:right, :3].permute(0, 3, 1, 2)
            crop = F.interpolate(item, size=(SIZE, SIZE), mode="bicubic", align_corners=False).permute(0, 2, 3, 1)[0].clamp(0, 1)
        crops.append(crop)
    last = next(c for c in crops if c is not None)
    for i in range(len(crops)):
        if crops[i] is None:
            crops[i] = last
        else:
            last = crops[i]
    offset = (-(len(crops) - 1)) % 8
    if offset:
        crops = [crops[0]] * offset + crops
    return torch.stack(crops)


pops = {kind: population(kind, a.frames) for kind in ("box256", "box1024", "mixed")}
plans = {kind: ops.crop_sequence_plan(e, a.frames, H, W) for kind, e in pops.items()}
n_out = plans["mixed"].count
out = torch.empty((n_out, SIZE, SIZE, 3), dtype=torch.float32, device=dev)
tables = {}
for kind, plan in plans.items():
    t = np.zeros(plan.count, dtype=ops._CROP_DESC)
    for k, (f, (l, tp, r, b)) in enumerate(plan.sources):
        t[k] = (((f * H + tp) * W + l) * 3, W * 3, 3, r - l, b - tp, (0, 0))
    tables[kind] = torch.from_numpy(t.view(np.uint8)).to(dev)
lib = _hip.lib()
legs = {"copy_nt": lambda: _hip.check(lib.vrg_debug_copy_f32(_hip.ptr(frames), _hip.ptr(out), out.numel(), 1, _hip.current_stream()), "copy")}
for kind in pops:
    legs[f"launch_{kind}"] = lambda kind=kind: _hip.check(lib.vrg_crop_resize_f32(_hip.ptr(frames), frames.numel(), _hip.ptr(out), _hip.ptr(tables[kind]),
                                                                               plans[kind].count, SIZE, SIZE, _hip.current_stream()), "crop")
    legs[f"op_{kind}"] = lambda kind=kind: ops.crop_frames(frames, plans[kind], out=out)
    legs[f"eager_{kind}"] = lambda kind=kind: eager_sequence(pops[kind])
ts = {k: [] for k in legs}
for rnd in range(a.iters + 2):                      # two warm-up rounds
    for name, fn in legs.items():
        if name.startswith("eager") and rnd >= a.eager_iters + 2:
            continue
        e0, e1 = ops.HipEvent(), ops.HipEvent()
        e0.record(); r = fn(); e1.record(); torch.cuda.synchronize()
        del r
        if rnd >= 2:
            ts[name].append(e0.elapsed_ms(e1))
res = {"frames": a.frames, "frame": [H, W], "size": SIZE, "output_frames": n_out, "iters": a.iters, "eager_iters": a.eager_iters}
copy_ms = statistics.median(ts["copy_nt"])
res["copy_nt_TBs"] = round(2 * out.numel() * 4 / copy_ms / 1e9, 3)
for name in legs:
    if ts[name]:
        res[name + "_ms"] = round(statistics.median(ts[name]), 3)
        res[name + "_ms_min_max"] = [round(min(ts[name]), 3), round(max(ts[name]), 3)]
for kind, plan in plans.items():
    box_bytes = sum((r - l) * (b - t) * 12 for _, (l, t, r, b) in plan.sources)
    gb = (box_bytes + out.numel() * 4) / 1e9
    res[f"{kind}_algorithmic_GB"] = round(gb, 3)
    res[f"{kind}_algorithmic_TBs"] = round(gb / res[f"launch_{kind}_ms"], 3)
    res[f"{kind}_frac_of_copy"] = round(res[f"{kind}_algorithmic_TBs"] / res["copy_nt_TBs"], 3)
    if f"eager_{kind}_ms" in res:
        res[f"{kind}_launch_over_eager"] = round(res[f"eager_{kind}_ms"] / res[f"launch_{kind}_ms"], 1)
        res[f"{kind}_op_over_eager"] = round(res[f"eager_{kind}_ms"] / res[f"op_{kind}_ms"], 1)
# host-fed: CPU frames, only the boxes cross
if a.host_frames:
    cpu = torch.rand((a.host_frames, H, W, 3))
    entries = population("mixed", a.host_frames)
    plan = ops.crop_sequence_plan(entries, a.host_frames, H, W)
    walls, whole = [], []
    for rnd in range(4):
        t0 = time.perf_counter(); r = ops.crop_frames_host(cpu, plan); walls.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); r2 = ops.crop_frames(cpu.to(dev), plan).cpu(); whole.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(r, r2)
    res["host_fed"] = {"frames": a.host_frames, "boxes": sorted(e["box"][2] - e["box"][0] for e in entries if e["box"]),
                       "frame_bytes": cpu.numel() * 4, "uploaded_bytes": ops.crop_host_bytes(plan),
                       "uploaded_fraction": round(ops.crop_host_bytes(plan) / (cpu.numel() * 4), 4),
                       "boxes_only_wall_ms": round(statistics.median(walls[1:]), 1), "whole_frames_wall_ms": round(statistics.median(whole[1:]), 1)}
print(json.dumps(res), flush=True)
if a.json:
    json.dump(res, open(a.json, "w"), indent=1)

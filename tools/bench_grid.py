"""Video Folder Grid Plot on frames resident in HBM: the one launch (vrg_grid_tiles_f32) beside the float4 copy of the same source bytes
in the same run.
    python tools/bench_grid.py [--frames 64] [--iters 10] [--json profiles/video_grid.json]
Legs: 4, 9 and 20 tiles of 1080p x `frames` frames to 480 x 270 cells; 9 tiles of 4K x frames / 4; 9 tiles of 1080p of unequal lengths
(frames, frames / 2, frames / 4, ...: the ended batches are resized again for every later output frame, so the launch reads
tiles x frames source frames although fewer are distinct); one host-fed leg (4 CPU batches of 1080p x 16 frames, wall clock).
"launch": the C entry point with its descriptors already on the device; "op": ops.video_grid (plans, builds and uploads the descriptors
too).  Legs are interleaved round by round after two warm-up rounds; a figure is the median of its timed rounds (HIP events) with the
spread (min, max) beside it.  Algorithmic bytes: 12 B per source pixel of every (output frame, tile); the grid written is small beside
it and is not counted.  The copy moves the same number of source bytes (read and written: 2 x)."""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package
load_package()
from comfyui_vrgamedevgirl_amd import _hip, ops
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--host-frames", type=int, default=16)
ap.add_argument("--json", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
F = a.frames
CELL_W, CELL_H = 480, 270
pool = torch.rand((20 * F, 1080, 1920, 3), generator=torch.Generator(device=dev).manual_seed(5), device=dev)
scratch = torch.empty_like(pool)
lib = _hip.lib()


def leg(name, tiles, shape, lengths):
    """tiles batches cut out of the pool: [lengths[i], H, W, 3] each"""
    H, W = shape
    per = H * W * 3
    slot = F * 1080 * 1920 * 3                      # tile i lives in the i-th slot of the pool
    assert all(n * per <= slot for n in lengths) and tiles <= 20
    batches = [pool.view(-1)[i * slot:i * slot + n * per].view(n, H, W, 3) for i, n in enumerate(lengths)]
    columns = max(1, int(np.ceil(np.sqrt(tiles))))
    plan = ops.grid_plan([(H, W, 3)] * tiles, CELL_W, CELL_H, columns, 0)
    frames = max(lengths)
    out = torch.empty((frames, plan.grid_h, plan.grid_w, 3), dtype=torch.float32, device=dev)
    index = [np.minimum(np.arange(frames), n - 1) for n in lengths]
    jobs = [(None, c, None, 0, np.full(frames, -1)) for c in range(tiles, plan.rows * columns)] + [(i, i, b, 0, index[i]) for i, b in enumerate(batches)]
    desc, keep = ops._grid_descriptors(plan, dev, jobs, None, [False] * tiles)
    dev_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
    read_bytes = frames * tiles * per * 4
    geometry = (frames, plan.cell_w, plan.cell_h, plan.grid_w, plan.grid_h)
    return {"name": name, "tiles": tiles, "source": [H, W], "lengths": list(lengths), "read_bytes": read_bytes, "modes": sorted({ops.GRID_MODES[t.mode] for t in plan.tiles}),
            "launch": lambda: _hip.check(lib.vrg_grid_tiles_f32(_hip.ptr(dev_desc), len(desc), _hip.ptr(out), *geometry, _hip.current_stream()), "grid"),
            "op": lambda: ops.video_grid(batches, CELL_W, CELL_H, columns, 0, None, out=out),
            "copy": lambda: _hip.check(lib.vrg_debug_copy_f32(_hip.ptr(pool), _hip.ptr(scratch), read_bytes // 4, 1, _hip.current_stream()), "copy"),
            "keep": (keep, dev_desc, out, batches)}


legs = [leg("1080p_4", 4, (1080, 1920), [F] * 4), leg("1080p_9", 9, (1080, 1920), [F] * 9), leg("1080p_20", 20, (1080, 1920), [F] * 20),
        leg("4k_9", 9, (2160, 3840), [max(1, F // 4)] * 9), leg("1080p_9_unequal", 9, (1080, 1920), [max(1, F >> i) for i in range(9)])]
ts = {(l["name"], k): [] for l in legs for k in ("launch", "op", "copy")}
for rnd in range(a.iters + 2):                      # two warm-up rounds
    for l in legs:
        for kind in ("launch", "copy", "op"):
            e0, e1 = ops.HipEvent(), ops.HipEvent()
            e0.record(); l[kind](); e1.record(); torch.cuda.synchronize()
            if rnd >= 2:
                ts[(l["name"], kind)].append(e0.elapsed_ms(e1))
res = {"frames": F, "cell": [CELL_W, CELL_H], "iters": a.iters, "legs": {}}
for l in legs:
    r = {k: l[k] for k in ("tiles", "source", "lengths", "read_bytes", "modes")}
    for kind in ("launch", "op", "copy"):
        t = ts[(l["name"], kind)]
        r[kind + "_ms"] = round(statistics.median(t), 3)
        r[kind + "_ms_min_max"] = [round(min(t), 3), round(max(t), 3)]
    r["algorithmic_TBs"] = round(l["read_bytes"] / r["launch_ms"] / 1e9, 3)
    r["copy_TBs"] = round(2 * l["read_bytes"] / r["copy_ms"] / 1e9, 3)
    r["frac_of_copy"] = round(r["algorithmic_TBs"] / r["copy_TBs"], 3)
    r["distinct_source_bytes"] = sum(l["lengths"]) * l["source"][0] * l["source"][1] * 12
    res["legs"][l["name"]] = r
if a.host_frames:
    cpu = [torch.rand((a.host_frames, 1080, 1920, 3)) for _ in range(4)]
    walls = []
    for rnd in range(3):
        t0 = time.perf_counter(); r = ops.video_grid(cpu, CELL_W, CELL_H, 2); torch.cuda.synchronize(); walls.append((time.perf_counter() - t0) * 1e3)
    want = ops.video_grid([c.to(dev) for c in cpu], CELL_W, CELL_H, 2)
    assert torch.equal(r, want)
    res["host_fed"] = {"tiles": 4, "frames": a.host_frames, "source_bytes": sum(c.numel() * 4 for c in cpu), "wall_ms": round(statistics.median(walls[1:]), 1),
                       "wall_ms_all": [round(w, 1) for w in walls]}
print(json.dumps(res), flush=True)
if a.json:
    json.dump(res, open(a.json, "w"), indent=1)

"""The landmark estimator's input on packed face bytes resident in HBM: the one launch (vrg_face_thumbs_u8) beside a copy of the same packed
buffers in the same run, and phase 1 of the landmark-aligned composite as it was (both packed buffers downloaded) beside the thumbnail
route (the launch plus the download of the thumbnails alone).
    python tools/bench_landmark_input.py [--entries 256] [--iters 10] [--json profiles/landmark_input.json]
Legs: `entries` boxes of 256 x 256, of 1024 x 1024, and of mixed sides 128 .. 2160 (seeded).  "launch": the C entry point with its
descriptors and tables already on the device (HIP events); "copy": vrg_debug_copy_f32 over the bytes of both packed buffers (read and
written: 2 x); "download_faces_ms" / "thumbs_route_ms": wall clock round work that ends in a device synchronise -- `.cpu()` of both packed
buffers, and ops.face_thumbs (descriptors, tables, check, launch) plus `.cpu()` of the thumbnails.  Legs are interleaved round by round
after two warm-up rounds; a figure is the median of its timed rounds with the spread (min, max) beside it.  Algorithmic bytes: the packed
bytes of both faces read once plus 614,400 thumbnail bytes per entry written.  Thumbnails cost 614,400 B per entry over PCIe whatever the
box: boxes under 320 x 320 download more than before, boxes above download less."""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package
load_package()
from comfyui_vrgamedevgirl_amd import _hip, ops
ap = argparse.ArgumentParser()
ap.add_argument("--entries", type=int, default=256)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--json", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
lib = _hip.lib()
N = a.entries
THUMB = ops.THUMB_SIDE * ops.THUMB_SIDE * 3


def leg(name, sides):
    sizes = [(int(s), int(s)) for s in sides]
    offsets, total = ops._pack_offsets([(0, 0, w, h) for w, h in sizes])
    gen = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(8))
    faces = ops.FaceBytes(gen, src, offsets, sizes)
    jobs = [(which, offsets[i], w, h) for i, (w, h) in enumerate(sizes) for which in (1, 0)]
    desc, tables, fix = ops.thumb_descriptors(jobs)
    records = torch.empty(desc.nbytes + tables.nbytes, dtype=torch.uint8, device=dev)
    for i, field, at in fix:
        desc[field][i] = records.data_ptr() + desc.nbytes + at
    _hip.check(lib.vrg_face_thumbs_check(desc.ctypes.data, len(desc), total, 1), "vrg_face_thumbs_check")
    records.copy_(torch.from_numpy(np.concatenate([desc.view(np.uint8), tables])))
    out = torch.empty((len(jobs), ops.THUMB_SIDE, ops.THUMB_SIDE, 3), dtype=torch.uint8, device=dev)
    scratch = torch.empty(2 * (total // 4) * 4, dtype=torch.uint8, device=dev)
    both = torch.cat([gen[:total // 4 * 4], src[:total // 4 * 4]])
    packed = sum(w * h * 3 for w, h in sizes) * 2

    def download_faces():
        return gen.cpu(), src.cpu()

    def thumbs_route():
        return ops.face_thumbs(faces)[0].cpu()

    return {"name": name, "sides": [min(sides), max(sides)], "packed_bytes": packed, "thumb_bytes": len(jobs) * THUMB, "tables": len(tables) // (ops.THUMB_SIDE * 20),
            "modes": sorted({ops.GRID_MODES[int(m)] for m in desc["mode"]}),
            "launch": lambda: _hip.check(lib.vrg_face_thumbs_u8(_hip.ptr(gen), _hip.ptr(src), total, _hip.ptr(records), len(desc), _hip.ptr(out),
                                                                _hip.current_stream()), "vrg_face_thumbs_u8"),
            "copy": lambda: _hip.check(lib.vrg_debug_copy_f32(_hip.ptr(both), _hip.ptr(scratch), both.numel() // 4, 1, _hip.current_stream()), "copy"),
            "download_faces": download_faces, "thumbs_route": thumbs_route, "keep": (records, out, scratch, both, faces)}


rng = np.random.Generator(np.random.PCG64(3))
legs = [leg("box_256", [256] * N), leg("box_1024", [1024] * N), leg("box_128_to_2160", rng.integers(128, 2161, N).tolist())]
ts = {(l["name"], k): [] for l in legs for k in ("launch", "copy", "download_faces", "thumbs_route")}
for rnd in range(a.iters + 2):                      # two warm-up rounds
    for l in legs:
        for kind in ("launch", "copy"):
            e0, e1 = ops.HipEvent(), ops.HipEvent()
            e0.record(); l[kind](); e1.record(); torch.cuda.synchronize()
            if rnd >= 2:
                ts[(l["name"], kind)].append(e0.elapsed_ms(e1))
        for kind in ("download_faces", "thumbs_route"):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); l[kind](); torch.cuda.synchronize()
            if rnd >= 2:
                ts[(l["name"], kind)].append((time.perf_counter() - t0) * 1e3)
res = {"entries": N, "iters": a.iters, "legs": {}}
for l in legs:
    r = {k: l[k] for k in ("sides", "packed_bytes", "thumb_bytes", "tables", "modes")}
    for kind in ("launch", "copy", "download_faces", "thumbs_route"):
        t = ts[(l["name"], kind)]
        r[kind + "_ms"] = round(statistics.median(t), 3)
        r[kind + "_ms_min_max"] = [round(min(t), 3), round(max(t), 3)]
    r["algorithmic_TBs"] = round((l["packed_bytes"] + l["thumb_bytes"]) / r["launch_ms"] / 1e9, 3)
    r["copy_TBs"] = round(2 * l["packed_bytes"] / r["copy_ms"] / 1e9, 3)
    r["download_bytes_before"], r["download_bytes_after"] = l["packed_bytes"], l["thumb_bytes"]
    res["legs"][l["name"]] = r
print(json.dumps(res), flush=True)
if a.json:
    json.dump(res, open(a.json, "w"), indent=1)

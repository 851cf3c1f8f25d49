"""Video Enhance Prepare against the path it replaces, on the GPU, alternating in one process.

    python tools/measure_prepare.py [--frames 64] [--host-frames 16] [--rounds 7] [--out profiles/prepare.json] [--direct-lib LIB]

Workload: `frames` x 2160 x 3840 device-resident frames -> 960 x 544 letterbox bicubic, anchors 768 x 448 every 16 frames; fp32 frames and
bytes of both sets.  New: two ops.prepare_frames calls.  Baseline (the parent path): video_frames[idx] gather, two ops.resize_frames,
(x * 255).round().to(torch.uint8) of both results on the device.  Also `host-frames` CPU frames fed through the node's host path against
the same baseline with an upload and the downloads of its results.  Times are device events around a call, best and median of `rounds`
alternated rounds after a warm-up; the spread is that of the same side across rounds.  The outputs of both sides are compared first.

--direct-lib: a variant library whose bicubic runs the direct form (rs_pixel per pixel, taps from global memory) instead of the LDS-staged
kernel -- `python tools/build_variant.py prepare_direct --unit vrg_prepare.hip --source self -DLAB_PREPARE_DIRECT_BICUBIC=1` makes
tools/ab/lib_prepare_direct.so -- is loaded beside the product library and the same two vrg_prepare_frames_f32 calls alternate between
the two ("staged_vs_direct"), outputs compared bit for bit first.
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

LETTERBOX, BICUBIC = "Fit with letterbox (preserve all)", "Bicubic (recommended)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare.json"))
    ap.add_argument("--direct-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_prepare: needs the GPU; nothing is measured without one")
    import __graft_entry__ as entry
    entry.load_package()
    from comfyui_vrgamedevgirl_amd import VRGDG_VideoEnhancePrepare as vep, ops

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand((a.frames, a.height, a.width, 3), generator=g, device=dev) * 1.2 - 0.1
    idx = vep._anchor_indices(a.frames, 16)
    g_ltx = ops.resize_geometry(a.height, a.width, 960, 544, LETTERBOX)
    g_anchor = ops.resize_geometry(a.height, a.width, 768, 448, LETTERBOX)

    def new(frames, indices):
        return ops.prepare_frames(frames, g_ltx, BICUBIC) + ops.prepare_frames(frames, g_anchor, BICUBIC, indices)

    def old(frames, indices):
        ltx = ops.resize_frames(frames, 960, 544, LETTERBOX, BICUBIC)
        anchors = ops.resize_frames(frames[torch.tensor(indices, device=frames.device, dtype=torch.long)], 768, 448, LETTERBOX, BICUBIC)
        return ltx, (ltx * 255).round().to(torch.uint8), anchors, (anchors * 255).round().to(torch.uint8)

    def host_new(frames, indices):
        return vep._prepare_pixels(frames, g_ltx, g_anchor, indices, BICUBIC)

    def host_old(frames, indices):
        out = old(frames.to(dev), indices)
        return tuple(t.cpu() for t in out)

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

    same = all(torch.equal(p.cpu(), q.cpu()) for p, q in zip(new(x[:4], [0, 3]), old(x[:4], [0, 3])))
    src_px = a.frames * a.height * a.width
    out_px = a.frames * g_ltx.out_h * g_ltx.out_w + len(idx) * g_anchor.out_h * g_anchor.out_w
    anchor_src_px = len(idx) * a.height * a.width
    result = {
        "workload": {"frames": a.frames, "source": [a.height, a.width], "ltx": [g_ltx.out_h, g_ltx.out_w], "anchors": [g_anchor.out_h, g_anchor.out_w],
                     "anchor_indices": idx, "fit_mode": LETTERBOX, "resize_method": BICUBIC, "device": torch.cuda.get_device_name(0)},
        "outputs_equal": same,
        "device_resident": alternate({"prepare_frames": new, "parent_path": old}, x, idx),
        # bytes the algorithm needs, per source pixel of the video: the new path reads every frame once per launch it takes part in and
        # writes 15 B per output pixel; the parent path copies the anchors (12 + 12), and reads and writes the fp32 results once more
        "bytes_per_source_pixel": {
            "prepare_frames": (12 * (src_px + anchor_src_px) + 15 * out_px) / src_px,
            "parent_path": (12 * (src_px + anchor_src_px) + 24 * anchor_src_px + 12 * out_px + (12 + 4) * out_px + 1 * out_px) / src_px},
    }
    host = x[:a.host_frames].cpu()
    host_idx = vep._anchor_indices(a.host_frames, 16)
    result["host_fed"] = dict(alternate({"prepare_pixels": host_new, "parent_path": host_old}, host, host_idx), frames=a.host_frames,
                              note="host clock excluded: device events around upload, kernels and downloads")
    for block in ("device_resident", "host_fed"):
        sides = [v for v in result[block].values() if isinstance(v, dict)]
        result[block]["spread_ms"] = max(v["worst_ms"] - v["best_ms"] for v in sides)
    if a.direct_lib:
        import ctypes as C
        from comfyui_vrgamedevgirl_amd import _hip
        libs = {"staged": _hip.lib(), "direct": _hip.load_library(os.path.abspath(a.direct_lib))}
        index = torch.tensor(idx, dtype=torch.int32, device=dev)
        outs = {k: [(torch.empty((n, gm.out_h, gm.out_w, 3), dtype=torch.float32, device=dev),
                     torch.empty((n, gm.out_h, gm.out_w, 3), dtype=torch.uint8, device=dev)) for n, gm in ((a.frames, g_ltx), (len(idx), g_anchor))]
                for k in libs}

        def raw(which):
            def call(frames, indices):
                for (f32, u8), gm, ix, n in zip(outs[which], (g_ltx, g_anchor), (None, index), (a.frames, len(idx))):
                    args = ops._geometry_args(frames, gm)
                    _hip.check(libs[which].vrg_prepare_frames_f32(_hip.ptr(frames), a.frames, *args[:3], C.c_void_p(0) if ix is None else _hip.ptr(ix), n,
                                                                 *args[3:], 0, _hip.ptr(f32), _hip.ptr(u8), _hip.current_stream()), which)
            return call

        result["staged_vs_direct"] = alternate({k: raw(k) for k in libs}, x, idx)
        result["staged_vs_direct"]["outputs_equal"] = all(torch.equal(p, q) for s, d in zip(outs["staged"], outs["direct"]) for p, q in zip(s, d))
        sides = [v for v in result["staged_vs_direct"].values() if isinstance(v, dict)]
        result["staged_vs_direct"]["spread_ms"] = max(v["worst_ms"] - v["best_ms"] for v in sides)
        print("staged_vs_direct", {k: (round(v["best_ms"], 3), round(v["median_ms"], 3)) for k, v in result["staged_vs_direct"].items() if isinstance(v, dict)},
              "equal", result["staged_vs_direct"]["outputs_equal"], "spread", round(result["staged_vs_direct"]["spread_ms"], 3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({k: result[k] for k in ("outputs_equal", "bytes_per_source_pixel")}))
    for block in ("device_resident", "host_fed"):
        print(block, {k: (round(v["best_ms"], 3), round(v["median_ms"], 3)) for k, v in result[block].items() if isinstance(v, dict)},
              "spread", round(result[block]["spread_ms"], 3))


if __name__ == "__main__":
    main()

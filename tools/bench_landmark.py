"""The landmark-aligned Face Fix composite on frames resident in HBM, in the geometry of tools/bench_composite.py: 4K frames, a
1024 x 1024 box per frame at varying positions, 512 x 512 work frames.
    python tools/bench_landmark.py [--frames 256] [--iters 10] [--host-frames 16] [--json profiles/landmark.json]
Legs, interleaved round by round after two warm-up rounds (median of the timed rounds, HIP events, min and max beside it):
  copy_nt         the float4 copy ceiling of the same run
  opaque          ops.composite_frames with the opaque rule
  fallback        ops.aligned_composite_frames without any transform -- the same path as `opaque`
  face_bytes      ops.face_bytes (vrg_face_bytes_u8) for every frame
  warped          ops.aligned_composite_frames with a transform on every frame (rotation 3 degrees, scale 1.02, a shift), the bytes given
and once, timed on the host clock, the node itself on `--host-frames` CPU 4K frames with a scripted estimator (host-fed leg)."""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package
load_package()
from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes as FF
from comfyui_vrgamedevgirl_amd import _hip, ops
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--host-frames", type=int, default=16)
ap.add_argument("--json", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
H, W, BOX, WORK, FEATHER = 2160, 3840, 1024, 512, 6
g = torch.Generator(device=dev).manual_seed(5)
work = torch.rand((a.frames, WORK, WORK, 3), generator=g, device=dev)
originals = torch.rand((a.frames, H, W, 3), generator=g, device=dev)
out = torch.empty_like(originals)
mask_out = torch.empty((a.frames, H, W), dtype=torch.float32, device=dev)
boxes = [((37 * i) % (W - BOX), (53 * i) % (H - BOX)) for i in range(a.frames)]
boxes = [(l, t, l + BOX, t + BOX) for l, t in boxes]
entries = [{"original": i, "crop": i, "box": boxes[i]} for i in range(a.frames)]
c, s, mid = 1.02 * np.cos(np.radians(3.0)), 1.02 * np.sin(np.radians(3.0)), (BOX - 1) / 2.0
transform = np.array([[c, -s, mid - c * mid + s * mid + 1.7], [s, c, mid - s * mid - c * mid - 2.2]], dtype=np.float32)
transforms = [transform] * a.frames
opaque = ops.CompositeRule("opaque", feather=FEATHER)
faces = ops.face_bytes(work, entries, H, W)
legs = {
    "copy_nt": lambda: _hip.check(_hip.lib().vrg_debug_copy_f32(_hip.ptr(originals), _hip.ptr(out), originals.numel(), 1, _hip.current_stream()), "copy"),
    "opaque": lambda: ops.composite_frames(originals, work, entries, opaque, 0.0, out=out, mask_out=mask_out),
    "fallback": lambda: ops.aligned_composite_frames(originals, work, entries, FEATHER, [None] * a.frames, out=out, mask_out=mask_out),
    "face_bytes": lambda: ops.face_bytes(work, entries, H, W),
    "warped": lambda: ops.aligned_composite_frames(originals, work, entries, FEATHER, transforms, generated=faces, out=out, mask_out=mask_out),
}
ts = {k: [] for k in legs}
for rnd in range(a.iters + 2):                      # two warm-up rounds
    for name, fn in legs.items():
        e0, e1 = ops.HipEvent(), ops.HipEvent()
        e0.record(); r = fn(); e1.record(); torch.cuda.synchronize()
        del r
        if rnd >= 2:
            ts[name].append(e0.elapsed_ms(e1))
res = {"frames": a.frames, "frame": [H, W], "box": BOX, "work": WORK, "iters": a.iters, "feather": FEATHER}
for name in legs:
    res[name + "_ms"] = round(statistics.median(ts[name]), 3)
    res[name + "_ms_min_max"] = [round(min(ts[name]), 3), round(max(ts[name]), 3)]
res["copy_nt_TBs"] = round(2 * originals.numel() * 4 / res["copy_nt_ms"] / 1e9, 3)
res["fallback_over_opaque"] = round(res["fallback_ms"] / res["opaque_ms"], 4)
res["warped_over_opaque"] = round(res["warped_ms"] / res["opaque_ms"], 3)
res["warped_plus_bytes_over_opaque"] = round((res["warped_ms"] + res["face_bytes_ms"]) / res["opaque_ms"], 3)
res["warped_frac_of_copy"] = round(res["copy_nt_ms"] / res["warped_ms"], 3)
res["warped_box_Gpix_s"] = round(a.frames * BOX * BOX / res["warped_ms"] / 1e6, 2)
del out, mask_out, originals, faces
torch.cuda.empty_cache()
if a.host_frames > 0:
    n = a.host_frames
    host = torch.rand((n, H, W, 3), generator=torch.Generator().manual_seed(6))
    ctx = {"original_frames": host, "entries": [{"box": boxes[i]} for i in range(n)], "ltx_frame_offset": 0}

    class Node(FF.VRGDGFaceFixCompositeLandmarkAligned):
        estimator = staticmethod(lambda source, generated: transform)

    times = []
    for _ in range(3):                               # the first call warms the staging buffers up
        t0 = time.perf_counter()
        r = Node().composite(work[:n].cpu(), ctx, FEATHER, 0.75)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        del r
    res["host_fed_frames"] = n
    res["host_fed_ms_calls"] = [round(t, 1) for t in times]
    res["host_fed_ms_per_frame"] = round(min(times[1:]) / n, 2)
print(json.dumps(res), flush=True)
if a.json:
    json.dump(res, open(a.json, "w"), indent=1)

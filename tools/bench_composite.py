"""Face Fix composite / Image Paste Back on frames resident in HBM: the new operators (ops.composite_frames) against the float4 copy
ceiling of the same run and against the reference's sequence restated as eager torch ops on the same device tensors (per-frame loop and
the .sum() synchronisation included).
    python tools/bench_composite.py [--frames 256] [--iters 10] [--json profiles/composite.json]
Geometry: 4K frames, a 1024 x 1024 box per frame at varying positions, 512 x 512 work frames.  Legs are interleaved round by round after
two warm-up rounds; a leg's figure is the median of its timed rounds (HIP events), with the spread (min, max) beside it.  Algorithmic bytes
per output pixel: 24 (image in and out) + 4 (mask); the crop reads (512 x 512 x 12 B per frame) are counted in "algorithmic_GB"."""
import argparse, json, os, statistics, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package
load_package()
from comfyui_vrgamedevgirl_amd import _hip, ops
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--eager-iters", type=int, default=3)
ap.add_argument("--json", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
H, W, BOX, WORK = 2160, 3840, 1024, 512
g = torch.Generator(device=dev).manual_seed(5)
work = torch.rand((a.frames, WORK, WORK, 3), generator=g, device=dev)
originals = torch.rand((a.frames, H, W, 3), generator=g, device=dev)
out = torch.empty_like(originals)
mask_out = torch.empty((a.frames, H, W), dtype=torch.float32, device=dev)
boxes = [((37 * i) % (W - BOX), (53 * i) % (H - BOX)) for i in range(a.frames)]
boxes = [(l, t, l + BOX, t + BOX) for l, t in boxes]
px = a.frames * H * W
FEATHER = 18


def resampled_patch(i, bh, bw):
    """work frame i at the box size: NHWC -> NCHW view, bicubic, back, clamped"""
    nchw = work[i].permute(2, 0, 1).unsqueeze(0)
    return F.interpolate(nchw, size=(bh, bw), mode="bicubic", align_corners=False).squeeze(0).permute(1, 2, 0).clamp_(0, 1)


def radial_weight(bh, bw):
    """1 at the box centre falling to 0 at radius 1 of the [-1, 1]^2 box, over the feather scale"""
    ramp_y = torch.linspace(-1, 1, bh, device=dev).unsqueeze(1)
    ramp_x = torch.linspace(-1, 1, bw, device=dev).unsqueeze(0)
    scale = max(1.0, FEATHER / max(1.0, 0.5 * min(bw, bh)))
    return (1.0 - (ramp_x * ramp_x + ramp_y * ramp_y).sqrt()).div(scale).clamp(0, 1)


def eager_face_fix(color_match):
    """The per-frame sequence of the Face Fix composite as eager torch ops on the device tensors: one Python iteration per frame, the same
    kinds of op in the same order (clone of the batch, resample, two ramps, weight, boolean gather and two means behind a host-side
    count, blend into the clone, mask write, final clamp of the batch)."""
    frames_out = originals.clone()
    mask_batch = torch.zeros((a.frames, H, W), device=dev)
    for i, (x0, y0, x1, y1) in enumerate(boxes):
        patch, weight = resampled_patch(i, y1 - y0, x1 - x0), radial_weight(y1 - y0, x1 - x0)
        region = frames_out[i, y0:y1, x0:x1]
        chosen = weight > 0.35
        if color_match > 0 and chosen.sum().item() >= 16:            # the host waits for the count here, once per frame
            patch = (patch + (region[chosen].mean(0) - patch[chosen].mean(0)) * color_match).clamp(0, 1)
        w3 = weight.unsqueeze(-1)
        region.copy_(region * (1 - w3) + patch * w3)
        mask_batch[i, y0:y1, x0:x1] = weight
    return frames_out.clamp(0, 1), mask_batch


radial = ops.CompositeRule("radial", feather=FEATHER)
ellipse = ops.CompositeRule("ellipse", feather=24, inset=8)
ff_entries = [{"original": i, "crop": i, "box": boxes[i], "strength": 1.0} for i in range(a.frames)]
legs = {"copy_nt": lambda: _hip.check(_hip.lib().vrg_debug_copy_f32(_hip.ptr(originals), _hip.ptr(out), originals.numel(), 1, _hip.current_stream()), "copy")}
for cm in (0.65, 0.0):
    legs[f"face_fix_cm{cm}"] = lambda cm=cm: ops.composite_frames(originals, work, ff_entries, radial, cm, out=out, mask_out=mask_out)
    legs[f"paste_back_cm{cm}"] = lambda cm=cm: ops.composite_frames(originals, work, ff_entries, ellipse, cm, out=out, mask_out=mask_out)
    legs[f"eager_face_fix_cm{cm}"] = lambda cm=cm: eager_face_fix(cm)
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
res = {"frames": a.frames, "frame": [H, W], "box": BOX, "work": WORK, "iters": a.iters, "eager_iters": a.eager_iters}
copy_ms = statistics.median(ts["copy_nt"])
res["copy_nt_TBs"] = round(2 * originals.numel() * 4 / copy_ms / 1e9, 3)
res["algorithmic_GB"] = round((px * 28 + a.frames * WORK * WORK * 12) / 1e9, 3)
for name in legs:
    if not ts[name]:                                 # --eager-iters 0: the eager legs were not timed
        continue
    med = statistics.median(ts[name])
    res[name + "_ms"] = round(med, 3)
    res[name + "_ms_min_max"] = [round(min(ts[name]), 3), round(max(ts[name]), 3)]
    if name != "copy_nt":
        res[name + "_Gpix_s"] = round(px / med / 1e6, 2)
for cm in (0.65, 0.0):
    for leg in ("face_fix", "paste_back"):
        res[f"{leg}_cm{cm}_frac_of_copy"] = round(copy_ms / res[f"{leg}_cm{cm}_ms"], 3)
        res[f"{leg}_cm{cm}_algorithmic_TBs"] = round(res["algorithmic_GB"] / res[f"{leg}_cm{cm}_ms"], 3)
    if f"eager_face_fix_cm{cm}_ms" in res:
        res[f"face_fix_over_eager_cm{cm}"] = round(res[f"eager_face_fix_cm{cm}_ms"] / res[f"face_fix_cm{cm}_ms"], 2)
print(json.dumps(res), flush=True)
if a.json:
    json.dump(res, open(a.json, "w"), indent=1)

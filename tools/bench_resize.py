"""Video Enhance restore (working-resolution frames -> source size, blended over the originals, clamped): the fused kernel
(ops.restore_frames) against the same work done the reference's way with eager torch ops on device tensors, against the float4 copy
ceiling of the same run, and a host-fed call of the node.
    python tools/bench_resize.py [--frames 256] [--iters 20] [--json profiles/resize_restore.json]
Legs are interleaved round by round; the figure of a leg is the median of its timed rounds (HIP events, device-resident frames)."""
import argparse, json, os, statistics, sys, time
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package
load_package()
from comfyui_vrgamedevgirl_amd import _hip, ops, VRGDG_VideoEnhanceNodes as ven
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--host-frames", type=int, default=16)
ap.add_argument("--json", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
WH, WW, SH, SW = 544, 960, 2160, 3840
FIT, METHOD = ops.FIT_LETTERBOX, "Bicubic (recommended)"
g = torch.Generator(device=dev).manual_seed(3)
work = torch.rand((a.frames, WH, WW, 3), generator=g, device=dev)
originals = torch.rand((a.frames, SH, SW, 3), generator=g, device=dev)
out = torch.empty_like(originals)
px = a.frames * SH * SW
geo = ops.restore_geometry(WH, WW, SW, SH, FIT)


def eager(strength):
    """what the reference executes, on the device: content slice -> F.interpolate -> clamp -> clone -> blend -> clamp"""
    x0, y0, w, h = geo.src
    content = work[:, y0:y0 + h, x0:x0 + w, :]
    restored = F.interpolate(content[..., :3].permute(0, 3, 1, 2), size=(SH, SW), mode="bicubic", align_corners=False).permute(0, 2, 3, 1).clamp(0, 1)
    output = originals.clone()
    output[..., :3] = originals[..., :3] * (1.0 - strength) + restored[..., :3] * strength
    return output.clamp(0, 1)


legs = {"copy_nt": lambda: _hip.check(_hip.lib().vrg_debug_copy_f32(_hip.ptr(originals), _hip.ptr(out), originals.numel(), 1, _hip.current_stream()), "copy")}
for s in (1.0, 0.5):
    legs[f"fused_s{s}"] = lambda s=s: ops.restore_frames(work, originals, SW, SH, FIT, METHOD, s, out=out)
    legs[f"eager_s{s}"] = lambda s=s: eager(s)
ts = {k: [] for k in legs}
for rnd in range(a.iters + 2):                      # two warm-up rounds
    for name, fn in legs.items():
        e0, e1 = ops.HipEvent(), ops.HipEvent()
        e0.record(); r = fn(); e1.record(); torch.cuda.synchronize()
        del r
        if rnd >= 2:
            ts[name].append(e0.elapsed_ms(e1))
res = {"frames": a.frames, "work": [WH, WW], "source": [SH, SW], "fit_mode": FIT, "method": METHOD, "iters": a.iters}
copy_ms = statistics.median(ts["copy_nt"])
res["copy_nt_TBs"] = round(2 * originals.numel() * 4 / copy_ms / 1e9, 3)
for name in legs:
    med = statistics.median(ts[name])
    res[name + "_ms"] = round(med, 3)
    if name != "copy_nt":
        res[name + "_Mpix_s"] = round(px / med / 1e3, 0)
for s in (1.0, 0.5):
    res[f"fused_s{s}_frac_of_copy"] = round(copy_ms / res[f"fused_s{s}_ms"], 3)
    res[f"fused_over_eager_s{s}"] = round(res[f"eager_s{s}_ms"] / res[f"fused_s{s}_ms"], 2)
# difference between the two (torch's device bicubic is another arithmetic than its CPU kernels): informational
d = (ops.restore_frames(work[:2], originals[:2], SW, SH, FIT, METHOD, 0.5) - eager(0.5)[:2]).abs().max().item()
res["fused_vs_eager_max_ulp1"] = round(d / 2.0 ** -23, 2)
del work, originals, out
torch.cuda.empty_cache()
# host-fed: CPU tensors through the node (pageable in, as ComfyUI hands them)
hw, ho = torch.rand(a.host_frames, WH, WW, 3), torch.rand(a.host_frames, SH, SW, 3)
node = ven.VRGDGVideoEnhanceRestoreOriginal()
ven._log = lambda message: None
ctx = {"original_frames": ho, "fit_mode": FIT, "fps": 24.0}
hts = []
for rnd in range(5):
    t0 = time.perf_counter()
    r = node.restore(hw, ctx, METHOD, 0.5)[0]
    float(r[-1, -1, -1, 0])                              # the result on the host
    hts.append(time.perf_counter() - t0)
    del r
res["host_fed_frames"] = a.host_frames
res["host_fed_ms"] = round(statistics.median(hts[1:]) * 1e3, 2)
res["host_fed_Mpix_s"] = round(a.host_frames * SH * SW / statistics.median(hts[1:]) / 1e6, 0)
print(json.dumps(res), flush=True)
if a.json:
    json.dump(res, open(a.json, "w"), indent=1)

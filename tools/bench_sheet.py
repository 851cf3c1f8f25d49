"""Reference sheets (ops.reference_sheet, csrc/vrg_sheet.hip) on one GPU.

    python tools/bench_sheet.py [--iters 8] [--json profiles/sheet.json]

Legs: six and 24 fp32 inputs at 4K and at 1080p -> 768 x 448 and -> 2048 x 1152, both fit modes (uniform grid, gutter 4, radius 3),
device-resident and host-fed.  Per leg, in one run and interleaved: the two launches by HIP events (median of --iters rounds after two
warm-up rounds), the float4 copy of the bytes of the SAME sources, the wall clock of the host-fed call, and a plain-Pillow restatement of
the same sheet on this machine's CPU (one run per leg; Pillow works on one core).  Launch A is reported in algorithmic TB/s of source
floats (every source counted whole, once) beside the copy (read + write).  The device result of every leg is checked against Pillow's."""
import argparse, json, os, statistics, sys, time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
from comfyui_vrgamedevgirl_amd import VRGDG_LTXICIngredientsGrid as grid  # noqa: E402
from comfyui_vrgamedevgirl_amd import _hip, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=8)
ap.add_argument("--json", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
lib = _hip.lib()
CELL, BACK = (184, 184, 184), (0, 0, 0)


def pillow(byte_sources, panels, canvas):
    from PIL import Image, ImageDraw
    sheet = Image.new("RGB", canvas, BACK)
    for p in panels:
        left, top, w, h = p.rect
        image = Image.fromarray(byte_sources[p.source], mode="RGB")
        sw, sh = image.size
        scale = max(w / sw, h / sh) if p.fit == "cover_crop" else min(w / sw, h / sh)
        nw, nh = max(1, int(round(sw * scale))), max(1, int(round(sh * scale)))
        resized = image.resize((nw, nh), Image.Resampling.LANCZOS)
        if p.fit == "cover_crop":
            x, y = max(0, (nw - w) // 2), max(0, (nh - h) // 2)
            panel = resized.crop((x, y, x + w, y + h))
        else:
            panel = Image.new("RGB", (w, h), CELL)
            panel.paste(resized, ((w - nw) // 2, (h - nh) // 2))
        mask = Image.new("L", (w, h), 0)
        ImageDraw.Draw(mask).rounded_rectangle((0, 0, w - 1, h - 1), radius=min(p.radius, w // 2, h // 2), fill=255)
        sheet.paste(panel, (left, top), mask)
    return np.asarray(sheet)


res = {"iters": a.iters, "legs": {}}
for count in (6, 24):
    for (H, W), tag in (((2160, 3840), "4k"), ((1080, 1920), "1080p")):
        host = [torch.rand((H, W, 3), generator=torch.Generator().manual_seed(40 + i)) for i in range(count)]
        device = [h.to(dev) for h in host]
        scratch = torch.empty_like(device[0])
        byte_sources = None
        for canvas in ((768, 448), (2048, 1152)):
            for fit in ("contain_pad", "cover_crop"):
                boxes = grid.panel_rectangles(grid.layout_rects("uniform_grid", count, 0), *canvas, 4, 4)
                panels = [ops.SheetPanel(i, b, fit, CELL, 3) for i, b in enumerate(boxes)]
                rows, compose, copy, fed = [], [], [], []
                for rnd in range(a.iters + 2):                                     # two warm-up rounds
                    t = {}
                    out = ops.reference_sheet(device, panels, canvas, BACK, out_bytes=True, timings=t)
                    e0, e1 = ops.HipEvent(), ops.HipEvent()
                    e0.record()
                    for d in device:
                        _hip.check(lib.vrg_debug_copy_f32(_hip.ptr(d), _hip.ptr(scratch), d.numel(), 1, _hip.current_stream()), "copy")
                    e1.record()
                    torch.cuda.synchronize()
                    if rnd >= 2:
                        rows.append(t["rows_ms"]); compose.append(t["compose_ms"]); copy.append(e0.elapsed_ms(e1))
                for rnd in range(3):
                    t0 = time.perf_counter()
                    got = ops.reference_sheet(host, panels, canvas, BACK, out_bytes=True).cpu()
                    fed.append((time.perf_counter() - t0) * 1e3)
                if byte_sources is None:
                    byte_sources = [np.clip(h.numpy() * 255.0, 0, 255).astype(np.uint8) for h in host]
                t0 = time.perf_counter()
                want = pillow(byte_sources, panels, canvas)
                pillow_ms = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(got.numpy(), want)
                source_bytes = count * H * W * 12
                r = {"inputs": count, "source": [H, W], "canvas": list(canvas), "fit": fit, "source_bytes": source_bytes,
                     "rows_ms": round(statistics.median(rows), 3), "rows_ms_min_max": [round(min(rows), 3), round(max(rows), 3)],
                     "compose_ms": round(statistics.median(compose), 3), "copy_ms": round(statistics.median(copy), 3),
                     "host_fed_wall_ms": round(statistics.median(fed[1:]), 1), "pillow_cpu_ms": round(pillow_ms, 1), "equals_pillow": True}
                r["rows_algorithmic_TBs"] = round(source_bytes / r["rows_ms"] / 1e9, 3)
                r["copy_TBs"] = round(2 * source_bytes / r["copy_ms"] / 1e9, 3)
                r["device_ms"] = round(r["rows_ms"] + r["compose_ms"], 3)
                r["pillow_over_device"] = round(pillow_ms / r["device_ms"], 1)
                r["pillow_over_host_fed"] = round(pillow_ms / r["host_fed_wall_ms"], 2)
                res["legs"][f"{count}x{tag}_{canvas[0]}x{canvas[1]}_{fit}"] = r
                print(json.dumps({f"{count}x{tag}_{canvas[0]}x{canvas[1]}_{fit}": r}), flush=True)
        del host, device, scratch
print(json.dumps(res), flush=True)
if a.json:
    with open(a.json, "w") as fh:                                                  # one line per leg
        fh.write('{"iters": %d, "legs": {\n' % a.iters + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in res["legs"].items()) + "\n}}\n")

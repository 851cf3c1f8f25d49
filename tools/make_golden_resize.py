"""Regenerate tests/golden/resize.npz (+ resize.json) from the reference's VRGDG_VideoEnhanceNodes.py.

    python tools/make_golden_resize.py

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT); the tests read the fixture only.  The work is done by a CHILD
process started with ATEN_CPU_CAPABILITY=default: torch's AVX2 / AVX-512 resampling kernels evaluate the source coordinate differently
from its plain build (a few ulp(1.0) in most elements), so "the reference's CPU result" depends on the machine; the plain
one-rounding-per-operation form is the reproducible one and is what csrc/vrg_resize_math.hpp restates.  The archive is written with
fixed member dates, so two runs give the same bytes.
"""
from __future__ import annotations

import io
import json
import os
import subprocess
import sys
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

FITS = ("Stretch to dimensions", "Crop to fill", "Fit with letterbox (preserve all)")
METHODS = ("Bicubic (recommended)", "Bilinear", "Area", "Nearest")
# (frames, height, width, channels) -> (target_width, target_height)
GEOMETRIES = (((2, 7, 5, 4), (13, 9)),        # up, odd sizes, RGBA in
              ((1, 1, 1, 3), (6, 4)),         # one source pixel
              ((1, 18, 24, 3), (9, 20)),      # smaller than the source on one axis only
              ((2, 30, 40, 4), (11, 7)),      # down
              ((1, 34, 36, 3), (80, 60)))     # height + width past 128 (torch picks its bilinear kernel by that sum): stretch only, the fixture stays small


def _write_npz(path, arrays):
    import numpy as np
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0))
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def child():
    import inspect

    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from oracle import reference_loader as RL

    # torch's bilinear kernel choice depends on the thread count as well: with ONE thread it always runs its channels-last kernel, with
    # several (how ComfyUI runs) the generic one once the resampled height + width passes 128.  The fixture records the usual case.
    if torch.get_num_threads() < 2:
        torch.set_num_threads(2)
    ref = RL._load_file("_vrgdg_reference_video_enhance", "VRGDG_VideoEnhanceNodes.py")
    ref._log = lambda message: None
    g = torch.Generator().manual_seed(20261016)
    flat, meta = {}, {"resize": [], "restore_batch": [], "restore": [], "errors": []}

    def frames(shape):
        return (torch.rand(shape, generator=g) * 1.2 - 0.1).contiguous()

    for gi, (shape, (tw, th)) in enumerate(GEOMETRIES):
        x = frames(shape)
        flat[f"resize.{gi}.in"] = x.numpy()
        for fi, fit in enumerate(FITS[:1] if gi == len(GEOMETRIES) - 1 else FITS):
            for mi, method in enumerate(METHODS):
                key = f"resize.{gi}.{fi}.{mi}"
                flat[key] = ref._resize_batch(x, tw, th, fit, method).contiguous().numpy()
                meta["resize"].append({"key": key, "in": f"resize.{gi}.in", "target_width": tw, "target_height": th, "fit_mode": fit,
                                       "resize_method": method, "shape": list(flat[key].shape)})

    # _restore_batch: working-resolution frames (what _resize_batch made of a source) back to the source size
    for si, (shape, (sw, sh)) in enumerate((((1, 16, 24, 3), (29, 23)), ((2, 20, 12, 4), (15, 18)))):
        x = frames(shape)
        flat[f"restore_batch.{si}.in"] = x.numpy()
        for fi, fit in enumerate(FITS):
            for mi, method in enumerate(METHODS):
                key = f"restore_batch.{si}.{fi}.{mi}"
                flat[key] = ref._restore_batch(x, sw, sh, fit, method).contiguous().numpy()
                meta["restore_batch"].append({"key": key, "in": f"restore_batch.{si}.in", "source_width": sw, "source_height": sh,
                                              "fit_mode": fit, "resize_method": method, "shape": list(flat[key].shape)})

    # the node: strength x fit mode x method, RGBA originals, frame_count - work_frames in {-2, 0, 3}
    node = ref.VRGDGVideoEnhanceRestoreOriginal()
    cases = [(0.0, FITS[0], METHODS[0], 3, 4, 4), (0.35, FITS[2], METHODS[0], 3, 4, 6), (1.0, FITS[1], METHODS[1], 3, 4, 1),
             (0.35, FITS[0], METHODS[2], 4, 3, 3), (1.0, FITS[2], METHODS[3], 4, 5, 2), (0.5, FITS[2], METHODS[1], 4, 2, 4)]
    for ci, (strength, fit, method, channels, frame_count, work_frames) in enumerate(cases):
        originals = frames((frame_count, 17, 22, channels))
        work = frames((work_frames, 10, 14, 3))
        ctx = {"original_frames": originals, "source_width": 22, "source_height": 17, "frame_count": frame_count, "fit_mode": fit, "fps": 24.0}
        out = node.restore(work, ctx, method, strength)
        flat[f"restore.{ci}.originals"], flat[f"restore.{ci}.work"] = originals.numpy(), work.numpy()
        flat[f"restore.{ci}.out"] = out[0].contiguous().numpy()
        meta["restore"].append({"key": f"restore.{ci}", "strength": strength, "fit_mode": fit, "resize_method": method,
                                "frame_count": frame_count, "returns": [out[1], out[2], out[3], out[4]]})

    for delta in (8, -8):
        originals = torch.zeros(10, 4, 4, 3)
        work = torch.zeros(10 - delta, 4, 4, 3)
        try:
            node.restore(work, {"original_frames": originals}, METHODS[0], 1.0)
            raise SystemExit("the reference accepted a frame-count difference of 8")
        except ValueError as exc:
            meta["errors"].append({"frame_count": 10, "work_frames": 10 - delta, "type": "ValueError", "text": str(exc)})
    for bad in (torch.zeros(0, 4, 4, 3), torch.zeros(4, 4, 3)):
        try:
            ref._resize_batch(bad, 8, 8, FITS[0], METHODS[0])
        except ValueError as exc:
            meta["errors"].append({"shape": list(bad.shape), "type": "ValueError", "text": str(exc)})
    try:
        node.restore(torch.zeros(1, 4, 4, 3), {"original_frames": None}, METHODS[0], 1.0)
    except ValueError as exc:
        meta["errors"].append({"original_frames": None, "type": "ValueError", "text": str(exc)})

    cls = ref.VRGDGVideoEnhanceRestoreOriginal
    meta["surface"] = {
        "class": "VRGDGVideoEnhanceRestoreOriginal", "INPUT_TYPES": cls.INPUT_TYPES(), "RETURN_TYPES": list(cls.RETURN_TYPES),
        "RETURN_NAMES": list(cls.RETURN_NAMES), "FUNCTION": cls.FUNCTION, "CATEGORY": cls.CATEGORY, "DESCRIPTION": cls.DESCRIPTION,
        "signature": list(inspect.signature(cls.restore).parameters),
        "display_name": ref.NODE_DISPLAY_NAME_MAPPINGS["VRGDGVideoEnhanceRestoreOriginal"],
        "context_type": ref.VIDEO_ENHANCE_CONTEXT,
        "helpers": {name: list(inspect.signature(getattr(ref, name)).parameters)
                    for name in ("_resize_batch", "_restore_batch", "_interpolation", "_round_dimension")},
        "interpolation": {m: ref._interpolation(m) for m in METHODS + ("anything else",)},
        "round_dimension": [[v, m, ref._round_dimension(v, m)] for v, m in ((960, 32), (543, 32), (3, 8), (100, 0), (1000.7, 64), (80, 32), (48, 32))],
    }
    meta["provenance"] = {"torch": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(),
                          "ATEN_CPU_CAPABILITY": os.environ.get("ATEN_CPU_CAPABILITY"), "threads": torch.get_num_threads(),
                          "source": "VRGDG_VideoEnhanceNodes.py of the reference, run unmodified on the CPU"}
    _write_npz(os.path.join(GOLDEN, "resize.npz"), flat)
    with open(os.path.join(GOLDEN, "resize.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print(f"resize.npz: {len(flat)} arrays, {os.path.getsize(os.path.join(GOLDEN, 'resize.npz'))} bytes; "
          f"capability {meta['provenance']['cpu_capability']}")


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        env = dict(os.environ, ATEN_CPU_CAPABILITY="default")
        raise SystemExit(subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env).returncode)

"""Regenerate tests/golden/prepare.json and tests/golden/prepare.npz from the reference's VRGDGVideoEnhancePrepare.

    python tools/record_prepare_golden.py

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT) and no GPU; the tests read the fixtures only and never import this
file.  The reference's VRGDG_VideoEnhanceNodes.py is loaded as it stands, with a stub `folder_paths` that points at a temporary
directory and `_encode_mp4` replaced by a recorder (no ffmpeg is run); `prepare` then runs on small seeded inputs and what it returns and
what it leaves in the job folder is written down.  As for resize.npz (tools/make_golden_resize.py) the work is done by a child process
started with ATEN_CPU_CAPABILITY=default: torch's plain one-rounding-per-operation kernels are the reproducible form of "the reference's
CPU result" and the one csrc/vrg_resize_math.hpp restates.  The archive is written with fixed member dates.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

LETTERBOX, CROP, STRETCH = "Fit with letterbox (preserve all)", "Crop to fill", "Stretch to dimensions"
# seed, input shape, then the arguments of prepare() after video_frames
CASES = (
    dict(seed=101, shape=(18, 24, 40, 3), anchor_interval="8 frames", anchor_width=16, anchor_height=8, ltx_width=24, ltx_height=16,
         dimension_multiple="8", fit_mode=LETTERBOX, resize_method="Bicubic (recommended)", fallback_fps=24.0, video_info={"loaded_fps": 30}),
    dict(seed=102, shape=(9, 30, 22, 4), anchor_interval="8 frames", anchor_width=8, anchor_height=16, ltx_width=16, ltx_height=16,
         dimension_multiple="8", fit_mode=CROP, resize_method="Bilinear", fallback_fps=24.0, video_info=None),
    dict(seed=103, shape=(5, 17, 23, 3), anchor_interval="16 frames (recommended)", anchor_width=11, anchor_height=9, ltx_width=20, ltx_height=12,
         dimension_multiple="8", fit_mode=STRETCH, resize_method="Area", fallback_fps=12.5, video_info={"fps": "25"}),
    dict(seed=104, shape=(3, 12, 20, 3), anchor_interval="120 frames", anchor_width=24, anchor_height=24, ltx_width=40, ltx_height=32,
         dimension_multiple="16", fit_mode=LETTERBOX, resize_method="Nearest", fallback_fps=23.976, video_info={"source_fps": 0}),
    dict(seed=105, shape=(17, 40, 64, 3), anchor_interval="8 frames", anchor_width=16, anchor_height=16, ltx_width=24, ltx_height=16,
         dimension_multiple="8", fit_mode=CROP, resize_method="Bicubic (recommended)", fallback_fps=24.0, video_info=None),
)
FPS_TABLE = (({"loaded_fps": 30, "source_fps": 25, "fps": 24}, 12.0), ({"loaded_fps": 0, "source_fps": 25.5, "fps": 24}, 12.0),
             ({"source_fps": None, "fps": "29.97"}, 12.0), ({"loaded_fps": "abc", "fps": 15}, 12.0), ({"loaded_fps": [30], "source_fps": -1}, 12.0),
             ({"loaded_fps": -5}, 48), ({}, 24.0), (None, 23.976), ("30", 10), ({"fps": True}, 7.0))


def seeded_frames(seed, shape):
    """The input of a case: values a little outside [0, 1] on both sides.  tests/prepare_support.py makes the same tensor."""
    import torch
    g = torch.Generator().manual_seed(int(seed))
    return (torch.rand(tuple(shape), generator=g) * 1.2 - 0.1).contiguous()


def child():
    import inspect

    import numpy as np
    import torch
    from PIL import Image
    sys.path.insert(0, ROOT)
    from oracle import reference_loader as RL
    from tools.make_golden_resize import _write_npz

    if torch.get_num_threads() < 2:
        torch.set_num_threads(2)
    ref = RL._load_file("_vrgdg_reference_video_enhance_prepare", "VRGDG_VideoEnhanceNodes.py")
    ref._log = lambda message: None
    cls = ref.VRGDGVideoEnhancePrepare
    flat, meta = {}, {"cases": [], "errors": []}

    with tempfile.TemporaryDirectory() as tmp:
        stub = types.ModuleType("folder_paths")
        stub.get_output_directory = lambda: tmp
        saved = sys.modules.get("folder_paths")
        sys.modules["folder_paths"] = stub
        real_encode = ref._encode_mp4
        encodes = []
        ref._encode_mp4 = lambda folder, count, fps, path: encodes.append((folder, count, fps, path))
        try:
            for ci, case in enumerate(CASES):
                x = seeded_frames(case["seed"], case["shape"])
                keep = x.clone()
                args = {k: v for k, v in case.items() if k not in ("seed", "shape")}
                out = cls().prepare(x, **args)
                assert torch.equal(x, keep) and out[8]["original_frames"] is x
                ctx = out[8]
                folders = {"anchor": ctx["anchor_sources_folder"], "frame": os.path.join(ctx["job_folder"], "ltx_working_frames")}
                names = {k: sorted(os.listdir(v)) for k, v in folders.items()}
                png = {k: np.stack([np.asarray(Image.open(os.path.join(folders[k], n)).convert("RGB")) for n in names[k]]) for k in folders}
                flat[f"case.{ci}.ltx"], flat[f"case.{ci}.anchors"] = out[0].contiguous().numpy(), out[1].contiguous().numpy()
                flat[f"case.{ci}.ltx_png"], flat[f"case.{ci}.anchors_png"] = png["frame"], png["anchor"]
                folder, count, fps, path = encodes[-1]
                meta["cases"].append({
                    "key": f"case.{ci}", "seed": case["seed"], "shape": list(case["shape"]), "args": args,
                    "resolved": {k: ctx[k] for k in ("anchor_width", "anchor_height", "ltx_width", "ltx_height")},
                    "anchor_indices": ctx["anchor_indices"], "returns": [out[2], out[3], out[5], out[6], out[7]],
                    "anchor_files": names["anchor"], "frame_files": names["frame"], "context_keys": list(ctx),
                    "context": {k: ctx[k] for k in ("version", "source_width", "source_height", "frame_count", "fps", "fit_mode", "resize_method")},
                    "job_id_pattern": r"video_enhance_\d{8}_\d{6}_[0-9a-f]{8}",
                    "layout": {"job_folder": os.path.relpath(ctx["job_folder"], tmp).replace(ctx["job_id"], "{job_id}").replace(os.sep, "/"),
                               "anchor_sources_folder": os.path.relpath(folders["anchor"], ctx["job_folder"]),
                               "ltx_working_frames": os.path.relpath(folders["frame"], ctx["job_folder"]),
                               "ltx_video_path": os.path.relpath(out[4], ctx["job_folder"])},
                    "encode": {"folder_is_ltx_working_frames": folder == folders["frame"], "frame_count": count, "fps": fps,
                               "path_is_ltx_video_path": path == out[4] == ctx["ltx_video_path"]}})

            # the five errors: two refused inputs, ffmpeg absent, ffmpeg failing, ffmpeg leaving no file
            for bad in (torch.zeros(4, 4, 3), torch.zeros(0, 4, 4, 3)):
                try:
                    cls().prepare(bad, "8 frames", 16, 16, 16, 16, "8", LETTERBOX, "Bicubic (recommended)", 24.0)
                    raise SystemExit("the reference accepted a bad batch")
                except ValueError as exc:
                    meta["errors"].append({"what": "batch", "shape": list(bad.shape), "type": "ValueError", "text": str(exc)})
            ref._encode_mp4 = real_encode
            real_which, real_run = ref.shutil.which, ref.subprocess.run
            saved_iio = sys.modules.get("imageio_ffmpeg")
            try:
                ref.shutil.which = lambda name: None
                sys.modules["imageio_ffmpeg"] = None                      # `import imageio_ffmpeg` raises ImportError
                try:
                    ref._encode_mp4(tmp, 3, 24.0, os.path.join(tmp, "none.mp4"))
                except RuntimeError as exc:
                    meta["errors"].append({"what": "ffmpeg absent", "type": "RuntimeError", "text": str(exc)})
                ref.shutil.which = lambda name: "ffmpeg"
                commands = []

                def fake_run(command, **kwargs):
                    commands.append((list(command), dict(kwargs)))
                    return types.SimpleNamespace(returncode=fake_run.code, stderr=fake_run.stderr, stdout="")

                ref.subprocess.run = fake_run
                for what, code, stderr in (("ffmpeg failed", 1, " x" * 1000 + " boom \n"), ("ffmpeg left no file", 0, "")):
                    fake_run.code, fake_run.stderr = code, stderr
                    try:
                        ref._encode_mp4(os.path.join(tmp, "frames"), 7, 29.97, os.path.join(tmp, "none.mp4"))
                    except RuntimeError as exc:
                        meta["errors"].append({"what": what, "returncode": code, "stderr": stderr, "type": "RuntimeError", "text": str(exc)})
                command, kwargs = commands[-1]
                meta["ffmpeg"] = {"frames_folder": "{frames}", "frame_count": 7, "fps": 29.97, "output_path": "{out}",
                                  "argv": [a.replace(os.path.join(tmp, "frames"), "{frames}").replace(os.path.join(tmp, "none.mp4"), "{out}")
                                           for a in command],
                                  "run_kwargs": {k: kwargs[k] for k in sorted(kwargs)}}
            finally:
                ref.shutil.which, ref.subprocess.run = real_which, real_run
                if saved_iio is None:
                    sys.modules.pop("imageio_ffmpeg", None)
                else:
                    sys.modules["imageio_ffmpeg"] = saved_iio
        finally:
            if saved is None:
                sys.modules.pop("folder_paths", None)
            else:
                sys.modules["folder_paths"] = saved
    assert len(meta["errors"]) == 5, meta["errors"]

    meta["fps"] = [[info, fallback, ref._fps(info, fallback)] for info, fallback in FPS_TABLE]
    meta["surface"] = {
        "class": cls.__name__, "INPUT_TYPES": cls.INPUT_TYPES(), "RETURN_TYPES": list(cls.RETURN_TYPES), "RETURN_NAMES": list(cls.RETURN_NAMES),
        "FUNCTION": cls.FUNCTION, "CATEGORY": cls.CATEGORY, "DESCRIPTION": cls.DESCRIPTION,
        "signature": list(inspect.signature(cls.prepare).parameters),
        "display_name": ref.NODE_DISPLAY_NAME_MAPPINGS["VRGDGVideoEnhancePrepare"], "context_type": ref.VIDEO_ENHANCE_CONTEXT,
        "helpers": {name: list(inspect.signature(getattr(ref, name)).parameters) for name in ("_fps", "_progress", "_save_image_batch", "_encode_mp4")},
    }
    meta["provenance"] = {"torch": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(),
                          "ATEN_CPU_CAPABILITY": os.environ.get("ATEN_CPU_CAPABILITY"), "threads": torch.get_num_threads(),
                          "source": "VRGDGVideoEnhancePrepare of the reference's VRGDG_VideoEnhanceNodes.py, run unmodified on the CPU; "
                                    "folder_paths stubbed, _encode_mp4 replaced by a recorder; the PNG files decoded with Pillow",
                          "recorder": "tools/record_prepare_golden.py", "covers": ["prepare.json", "prepare.npz"]}
    # the provenance of both fixtures travels inside prepare.json, as resize.json carries its own: provenance.json belongs to
    # oracle/make_golden.py, which rewrites it whole
    _write_npz(os.path.join(GOLDEN, "prepare.npz"), flat)
    with open(os.path.join(GOLDEN, "prepare.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print(f"prepare.npz: {len(flat)} arrays, {os.path.getsize(os.path.join(GOLDEN, 'prepare.npz'))} bytes; "
          f"capability {meta['provenance']['cpu_capability']}")


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        env = dict(os.environ, ATEN_CPU_CAPABILITY="default")
        raise SystemExit(subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env).returncode)

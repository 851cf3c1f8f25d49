"""Regenerate tests/golden/crop.npz (+ crop.json) from the reference's two Face Fix Prepare nodes.

    python tools/make_golden_crop.py

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT) and g++; the tests read the fixture only.  A CHILD process started
with ATEN_CPU_CAPABILITY=default (torch's plain resampling kernels, as tools/make_golden_resize.py) runs the reference's OWN
VRGDGFaceFixPrepare.prepare and VRGDGFaceFixPrepareShotAware.prepare, their text unmodified -- the classes and the helper functions they
call are taken out of the file by AST.  What cannot run here is replaced around them: `cv2` and `folder_paths` are stub modules
(cvtColor = identity, imwrite = no-op, the output directory a temporary one), `_detector` returns nothing, and `_detect_with_rotation` /
`_cut_score` are scripted functions that return the case's candidate lists and cut scores frame by frame.  Choice of the face, smoothing,
the crop box, the crop, hole filling, prefix, anchors and the stack are the reference's.

The reference's batches are 3 MB per frame and are NOT stored.  Per case the fixture keeps how the input frames are generated (shape,
seed: tests/crop_support.py make_frames), the script, the reference's entries, ltx_frame_offset and anchors, the shape of crop_batch, the
SHA-256 of its float32 bytes, of anchor_batch and of every output frame, and the values at crop_support.SAMPLES seeded positions.
"""
from __future__ import annotations

import ast
import json
import os
import subprocess
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

_HIT = 0.9      # detector score of every scripted candidate


def _face(x, y, w, h=None):
    return [(float(x), float(y), float(w), float(w if h is None else h), _HIT)]


MISS = []
# key, class, frame shape, script (candidates per frame), keyword overrides.  Defaults: padding 0, all faces repaired, anchors every 8
# frames, no short-gap tracking (a miss is a hole), ShotAware: crop_smoothing 0 (the box is the scripted face), no cuts.
CASES = (
    # scale up: boxes of 9, 17, 40, 75, 120, 200, 300, 250 and 64 px to 512; 9 frames = ltx_offset 0
    ("up_9_to_300", "shot", (9, 320, 400, 3), [_face(3, 5, 9), _face(100, 100, 17), _face(200, 150, 40), _face(10, 200, 75), _face(250, 30, 120),
                                                _face(150, 100, 200), _face(50, 10, 300), _face(140, 60, 250), _face(300, 250, 64)], {}),
    # scale down: a 700 px box (1.4x), a 2080 px box (past 4x: the direct form); 2 frames = ltx_offset 7
    ("down_700_and_2080", "shot", (2, 2100, 2200, 3), [_face(900, 1000, 700), _face(60, 10, 2080)], {}),
    ("one_by_one", "prepare", (1, 16, 20, 3), [_face(7, 5, 1)], {}),
    # the face is larger than the frame is high: the box is the whole short side
    ("whole_short_side", "shot", (3, 40, 64, 3), [_face(5, -3, 50), _face(20, 0, 44), _face(0, 0, 40)], {}),
    ("touching_each_edge", "shot", (4, 48, 64, 3), [_face(0, 10, 20), _face(20, 0, 20), _face(44, 10, 20), _face(20, 28, 20)], {}),
    ("rgba_source", "prepare", (3, 50, 60, 4), [_face(10, 8, 24, 30), _face(14, 10, 26, 28), _face(20, 12, 22)], {}),
    # leading, inner and trailing holes; 10 frames = ltx_offset 7 with a hole as output frame 0
    ("holes_everywhere", "prepare", (10, 64, 80, 3), [MISS, MISS, _face(10, 10, 30), _face(14, 12, 33), MISS, MISS, _face(40, 20, 25), MISS,
                                                      MISS, MISS], {}),
    ("single_valid_frame", "prepare", (5, 40, 40, 3), [MISS, MISS, _face(12, 9, 21), MISS, MISS], {}),
    # short-gap tracking: the missed frames keep the last box (their OWN pixels are cropped), the third miss is a hole
    ("tracked_gap", "prepare", (6, 64, 80, 3), [_face(20, 16, 28), MISS, MISS, MISS, _face(30, 20, 24), _face(33, 22, 25)],
     {"short_gap_tracking": 2, "crop_padding": 0.25}),
    # three shots (cuts at frames 3 and 6): the middle one has no face at all, the last one only at its end
    ("per_shot_fill", "shot", (9, 48, 64, 3), [MISS, _face(8, 6, 30), MISS, MISS, MISS, MISS, MISS, MISS, _face(30, 12, 26)],
     {"cuts": (3, 6), "crop_smoothing": 0.85}),
    ("per_shot_smoothed", "shot", (4, 48, 64, 4), [_face(8, 6, 30), _face(12, 8, 28), MISS, _face(20, 10, 31)],
     {"cuts": (3,), "crop_smoothing": 0.85, "crop_padding": 0.1}),
)
NO_FACE = (("prepare", (3, 24, 24, 3)), ("shot", (2, 24, 24, 3)))

FUNCTIONS = {"_iou", "_choose", "_crop_box", "_interval", "_distance_repair_strength"}
CLASSES = {"VRGDGFaceFixPrepare", "VRGDGFaceFixPrepareShotAware"}


def _load_reference(namespace):
    """The Prepare classes and the helper functions they call, taken out of the reference file by AST and executed in `namespace`;
    nothing of the file is written anywhere."""
    from oracle import reference_loader as RL
    path = os.path.join(RL.REFERENCE_ROOT, "VRGDG_StandaloneFaceFixNodes.py")
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    body = [n for n in tree.body if (isinstance(n, ast.FunctionDef) and n.name in FUNCTIONS) or (isinstance(n, ast.ClassDef) and n.name in CLASSES)]
    assert {n.name for n in body} == FUNCTIONS | CLASSES
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), namespace)
    return namespace


def child():
    import time
    import uuid

    import numpy as np
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import crop_support as CS
    from conftest import load_package
    from make_golden_composite import _write_npz

    load_package()
    from comfyui_vrgamedevgirl_amd import ops
    out_dir = tempfile.mkdtemp(prefix="crop_golden_out")
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2BGR = 4
    cv2.cvtColor = lambda image, code: image
    cv2.imwrite = lambda path, image: True
    folder_paths = types.ModuleType("folder_paths")
    folder_paths.get_output_directory = lambda: out_dir
    sys.modules["cv2"], sys.modules["folder_paths"] = cv2, folder_paths

    script = {"candidates": [], "cuts": (), "detect_calls": 0, "cut_calls": 0}

    def scripted_detect(net, bgr, confidence, minimum_pixels, rotation_assist):
        found = script["candidates"][script["detect_calls"]]
        script["detect_calls"] += 1
        return list(found)

    def scripted_cut_score(previous_rgb, current_rgb):
        script["cut_calls"] += 1                                  # called for frames 1, 2, ...
        return 1.0 if script["cut_calls"] in script["cuts"] else 0.0

    ns = {"torch": torch, "F": F, "os": os, "time": time, "uuid": uuid, "FACE_FIX_CONTEXT": "VRGDG_FACE_FIX_CONTEXT",
          "_log": lambda message: None, "_progress": lambda *a, **k: None, "_detector": lambda: {"kind": "scripted"},
          "_detect_with_rotation": scripted_detect}
    _load_reference(ns)
    ns["VRGDGFaceFixPrepareShotAware"]._cut_score = staticmethod(scripted_cut_score)
    hm = CS.build_host_lib(tempfile.mkdtemp(prefix="crop_check"))

    def run(kind, frames, candidates, options):
        script.update(candidates=candidates, cuts=tuple(options.get("cuts", ())), detect_calls=0, cut_calls=0)
        args = [frames, 0.5, float(options.get("crop_padding", 0.0)), 4, "Off (fastest)", "All detected faces", 9.0, "8 frames",
                int(options.get("short_gap_tracking", 0))]
        if kind == "shot":
            args += [0.5, float(options.get("crop_smoothing", 0.0))]
            return ns["VRGDGFaceFixPrepareShotAware"]().prepare(*args)
        return ns["VRGDGFaceFixPrepare"]().prepare(*args)

    flat, cases, problems = {}, [], []
    for i, (key, kind, shape, candidates, options) in enumerate(CASES):
        seed = 700 + i
        assert len(candidates) == shape[0], key
        x = CS.make_frames(shape, seed)
        frames = torch.from_numpy(x.copy())
        crop_batch, anchor_batch, n_anchors, anchor_text, context = run(kind, frames, candidates, options)
        assert torch.equal(frames, torch.from_numpy(x)), key
        crop = crop_batch.contiguous().numpy()
        entries = [{"index": e["index"], "box": [int(v) for v in e["box"]] if e["box"] else None, "fresh": bool(e["fresh"]),
                    "strength": float(e["strength"]), **({"shot_id": int(e["shot_id"])} if "shot_id" in e else {})} for e in context["entries"]]
        case = {"key": key, "class": "VRGDGFaceFixPrepareShotAware" if kind == "shot" else "VRGDGFaceFixPrepare", "per_shot": kind == "shot",
                "shape": list(shape), "seed": seed, "frames": "crop_support.make_frames(shape, seed)",
                "script": {"candidates": [[list(c) for c in f] for f in candidates], **{k: (list(v) if isinstance(v, tuple) else v) for k, v in options.items()}},
                "entries": entries, "ltx_frame_offset": int(context["ltx_frame_offset"]), "anchors": [int(a) for a in context["anchor_indices"]],
                "crop_shape": list(crop.shape), "crop_sha256": CS.sha(crop), "anchor_shape": list(anchor_batch.shape),
                "anchor_sha256": CS.sha(anchor_batch.contiguous().numpy()), "frame_sha256": CS.frame_shas(crop),
                "value_range": [float(crop.min()), float(crop.max())]}
        flat[key + ".samples"] = crop.reshape(-1)[CS.sample_positions(crop.size, seed)]
        # the host arithmetic of this repository on the same inputs
        plan = ops.crop_sequence_plan(CS.entries_of(case), shape[0], shape[1], shape[2], per_shot=case["per_shot"])
        got = CS.host_crop(hm, x, CS.plan_records(plan, shape[3]))
        bad = CS.mismatches(got, crop) if got.shape == crop.shape else -1
        if bad or plan.ltx_offset != case["ltx_frame_offset"]:
            problems.append(f"{key}: host arithmetic differs from the reference in {bad} elements (ltx_offset {plan.ltx_offset} / {case['ltx_frame_offset']})")
        cases.append(case)
        boxes = [e["box"][2] - e["box"][0] for e in entries if e["box"]]
        print(f"{key}: crop {list(crop.shape)}, boxes {boxes}, offset {case['ltx_frame_offset']}, anchors {case['anchors']}, host mismatches {bad}", flush=True)

    errors = []
    for kind, shape in NO_FACE:
        try:
            run(kind, torch.zeros(shape), [MISS] * shape[0], {})
            raise SystemExit("the reference accepted a video without a face")
        except ValueError as exc:
            errors.append({"class": "VRGDGFaceFixPrepareShotAware" if kind == "shot" else "VRGDGFaceFixPrepare", "per_shot": kind == "shot",
                           "shape": list(shape), "type": "ValueError", "text": str(exc)})
    for cls in ("VRGDGFaceFixPrepare",):
        try:
            ns[cls]().prepare(torch.zeros(0, 4, 4, 3), 0.5, 0.0, 4, "Off (fastest)", "All detected faces", 9.0, "8 frames", 0)
            raise SystemExit("the reference accepted an empty batch")
        except ValueError as exc:
            errors.append({"class": cls, "shape": [0, 4, 4, 3], "type": "ValueError", "text": str(exc)})

    # what the cases cover, from the reference's own boxes
    sides = [(e["box"][2] - e["box"][0], e["box"][3] - e["box"][1], c) for c in cases for e in c["entries"] if e["box"]]
    widths = [s[0] for s in sides]
    cover = {"smallest_box": min(widths), "largest_box": max(widths), "boxes_9_to_300": sorted({w for w in widths if 9 <= w <= 300}),
             "ltx_offsets": sorted({c["ltx_frame_offset"] for c in cases}), "channels": sorted({c["shape"][3] for c in cases})}
    assert cover["smallest_box"] == 1 and cover["largest_box"] > 2048 and any(512 < w <= 2048 for w in widths), cover
    assert 9 in widths and 300 in widths and {0, 7} <= set(cover["ltx_offsets"]) and cover["channels"] == [3, 4], cover
    meta = {"cases": cases, "errors": errors, "coverage": cover, "samples": CS.SAMPLES,
            "provenance": {"torch": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(),
                           "ATEN_CPU_CAPABILITY": os.environ.get("ATEN_CPU_CAPABILITY"), "threads": torch.get_num_threads(),
                           "source": "VRGDGFaceFixPrepare.prepare and VRGDGFaceFixPrepareShotAware.prepare of the reference's "
                                     "VRGDG_StandaloneFaceFixNodes.py, their text unmodified, run on the CPU with stub cv2 / folder_paths "
                                     "modules and scripted _detector / _detect_with_rotation / _cut_score"}}
    _write_npz(os.path.join(GOLDEN, "crop.npz"), flat)
    with open(os.path.join(GOLDEN, "crop.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print(f"crop.npz: {len(flat)} arrays, {os.path.getsize(os.path.join(GOLDEN, 'crop.npz'))} bytes; coverage {cover}")
    if problems:
        raise SystemExit("\n".join(problems))


if __name__ == "__main__":
    if "--child" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        child()
    else:
        env = dict(os.environ, ATEN_CPU_CAPABILITY="default")
        raise SystemExit(subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env).returncode)

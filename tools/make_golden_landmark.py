"""Regenerate tests/golden/landmark.npz (+ landmark.json) from the reference's VRGDGFaceFixCompositeLandmarkAligned.

    python tools/make_golden_landmark.py

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT); the tests read the fixture only.  A CHILD process started with
ATEN_CPU_CAPABILITY=default (torch's plain resampling kernels, as tools/make_golden_crop.py) runs the reference's OWN class, its text
unmodified -- taken out of the file by AST.  What cannot run here is replaced around it: `cv2` is a stub module whose `warpAffine` is the
numpy restatement of tests/warp_support.py (no cv2 is at hand; equality of that restatement with cv2 itself is what
tests/test_warp_host.py::test_warp_equals_cv2 pins wherever cv2 or its fixture exists) and whose `estimateAffinePartial2D` returns the
case's scripted matrix; `_detector` returns a token (or None: the case without a detector) and `_landmarks` returns a token or None as
the script says.  torch.sqrt is the correctly rounded root, as in tools/make_golden_composite.py.  Control flow, smoothing, resets, the
byte quantisation, the alpha and the blend are the reference's.

The inputs are generated from a seed (tests/warp_support.py case_inputs) and NOT stored; per case the fixture keeps the script, the
transforms the reference handed to warpAffine, its counts and log line, the SHA-256 of the float32 image and mask batches and the values
at warp_support.SAMPLES seeded positions of each.
"""
from __future__ import annotations

import ast
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
H, W = 44, 60
MISS = None


def child():
    import numpy as np
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import warp_support as WS
    from make_golden_composite import _load_classes, _write_npz

    def sim(scale, degrees, tx, ty, box):
        left, top, right, bottom = box
        return WS.similarity(scale, degrees, tx, ty, ((right - left - 1) / 2.0, (bottom - top - 1) / 2.0)).astype(np.float64).tolist()

    A, B, C4 = (6, 4, 38, 36), (10, 8, 50, 40), (20, 10, 41, 33)
    near = [sim(1.02, 3.0, 0.7, -0.4, A), sim(0.98, -2.0, -0.9, 0.6, A), sim(1.05, 5.5, 1.3, 0.2, A), sim(1.0, -4.0, 0.1, -1.1, A),
            sim(0.96, 1.5, -0.6, 0.9, A), sim(1.01, 0.5, 0.4, 0.3, A)]
    six = [{"box": list(A)} for _ in range(6)]
    # key, originals (n, channels), work (n, h, w, channels), offset, feather, smoothing, detector, entries, script (one per source frame)
    CASES = [
        ("no_detector", (4, 3), (4, 24, 20, 3), 0, 6, 0.75, False, six[:4], near[:4]),
        ("every_frame", (6, 3), (6, 24, 20, 3), 0, 6, 0.75, True, six, near),
        ("misses_reuse_previous", (6, 3), (6, 24, 20, 3), 0, 6, 0.75, True, six, [near[0], MISS, MISS, near[3], MISS, near[5]]),
        ("leading_miss", (5, 3), (5, 24, 20, 3), 0, 4, 0.75, True, six[:5], [MISS, MISS, near[2], MISS, near[4]]),
        ("smoothing_0", (6, 3), (6, 24, 20, 3), 0, 6, 0.0, True, six, near),
        ("smoothing_095_clamped_from_2", (6, 3), (6, 24, 20, 3), 0, 6, 2.0, True, six, near),
        ("resets", (8, 3), (8, 24, 20, 3), 0, 6, 0.75, True,
         [{"box": list(A), "shot_id": 0}, {"box": list(A), "shot_id": 0}, {"box": list(A), "shot_id": 0, "hard_cut": True},
          {"box": list(A), "shot_id": 0}, {"box": list(B), "shot_id": 1}, {"box": list(B), "shot_id": 1}, {"box": None, "shot_id": 2},
          {"box": list(B), "shot_id": 1}],
         [near[0], near[1], MISS, near[3], MISS, near[5], MISS, near[2]]),
        ("offset_7", (3, 3), (10, 24, 20, 3), 7, 6, 0.75, True, six[:3], near[:3]),
        ("short_ltx_tail", (6, 3), (4, 24, 20, 3), 0, 6, 0.5, True, six, near),
        ("empty_and_missing_boxes", (5, 3), (5, 24, 20, 3), 0, 6, 0.75, True,
         [{"box": list(A)}, {"box": [5, 5, 5, 9]}, {"box": None}, {"box": [7, 9, 30, 9]}, {"box": list(A)}], [near[0], near[1], near[2], near[3], near[4]]),
        ("rgba_originals_rgba_work", (4, 4), (4, 30, 34, 4), 0, 5, 0.75, True, six[:4], near[:4]),
        ("boxes_touching_each_edge", (5, 3), (5, 24, 20, 3), 0, 3, 0.25, True,
         [{"box": [0, 10, 24, 30]}, {"box": [20, 0, 44, 22]}, {"box": [36, 12, 60, 36]}, {"box": [18, 20, 40, 44]}, {"box": [0, 0, 60, 44]}],
         [sim(1.03, 4.0, 0.5, 0.5, (0, 10, 24, 30)), sim(0.97, -3.0, -0.5, 1.0, (20, 0, 44, 22)), sim(1.0, 2.0, 1.5, -0.5, (36, 12, 60, 36)),
          sim(1.04, -6.0, 0.0, 0.8, (18, 20, 40, 44)), sim(1.01, 1.0, -1.0, 0.3, (0, 0, 60, 44))]),
        ("feather_0", (3, 3), (3, 24, 20, 3), 0, 0, 0.75, True, six[:3], near[:3]),
        ("far_outside_rotation_and_shift", (4, 3), (4, 24, 20, 3), 0, 6, 0.0, True,
         [{"box": list(C4)}, {"box": list(C4)}, {"box": [30, 20, 39, 27]}, {"box": [30, 20, 32, 23]}],
         [sim(1.1, 33.0, 60.0, -45.0, C4), sim(0.9, -120.0, -75.0, 90.0, C4), sim(1.0, 33.0, 40.0, 31.0, (30, 20, 39, 27)),
          sim(1.3, 77.0, -55.0, 48.0, (30, 20, 32, 23))]),
        ("downscale_06", (3, 3), (3, 24, 20, 3), 0, 6, 0.0, True, six[:3], [sim(0.6, 0.0, 0.0, 0.0, A), sim(0.6, -12.0, 2.0, 5.0, A), sim(0.6, 8.0, -3.0, 1.0, A)]),
    ]

    state = {"script": [], "order": [], "landmark_calls": 0, "applied": [], "log": []}
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LANCZOS4, cv2.BORDER_REFLECT101, cv2.RANSAC = 4, 4, 8

    def estimate(generated_points, source_points, method=None, ransacReprojThreshold=None):
        assert generated_points[0] == "generated" and source_points[0] == "source" and generated_points[1] == source_points[1]
        return np.array(state["script"][state["order"][generated_points[1]]], dtype=np.float64), None

    def warp(image, transform, size, flags=None, borderMode=None):
        assert flags == cv2.INTER_LANCZOS4 and borderMode == cv2.BORDER_REFLECT101 and transform.dtype == np.float32
        assert image.dtype == np.uint8 and (image.shape[1], image.shape[0]) == tuple(size)
        state["applied"].append(np.array(transform, copy=True))
        return WS.restated(image, transform, size[0], size[1])

    cv2.estimateAffinePartial2D, cv2.warpAffine = estimate, warp
    sys.modules["cv2"] = cv2

    def landmarks(detector, rgb):
        k, which = divmod(state["landmark_calls"], 2)                    # the reference asks for the source first, then the generated face
        state["landmark_calls"] += 1
        assert rgb.dtype == np.uint8 and rgb.ndim == 3
        if detector is None or state["script"][state["order"][k]] is None:
            return None
        return ("generated" if which else "source", k)

    ns = {"torch": torch, "F": F, "os": os, "FACE_FIX_CONTEXT": "VRGDG_FACE_FIX_CONTEXT", "_log": state["log"].append,
          "_progress": lambda *a, **k: None}
    _load_classes("VRGDG_StandaloneFaceFixNodes.py", {"VRGDGFaceFixCompositeLandmarkAligned"}, ns)
    cls = ns["VRGDGFaceFixCompositeLandmarkAligned"]
    cls._landmarks = staticmethod(landmarks)
    vendor_sqrt = torch.sqrt
    torch.sqrt = lambda x: torch.from_numpy(np.sqrt(x.detach().numpy()))     # correctly rounded (tools/make_golden_composite.py)

    flat, cases = {}, []
    for i, (key, (n_o, ch), work_shape, offset, feather, smoothing, detector, entries, script) in enumerate(CASES):
        case = {"key": key, "seed": 900 + i, "originals_shape": [n_o, H, W, ch], "work_shape": list(work_shape), "offset": offset,
                "feather_pixels": feather, "transform_smoothing": smoothing, "detector": detector, "entries": entries, "script": script}
        assert len(script) == n_o == len(entries), key
        originals, work = WS.case_inputs(case)
        usable = min(len(entries), max(0, work_shape[0] - offset))
        order = [k for k in range(usable) if entries[k].get("box") and entries[k]["box"][2] > entries[k]["box"][0] and entries[k]["box"][3] > entries[k]["box"][1]]
        state.update(script=script, order=order, landmark_calls=0, applied=[], log=state["log"])
        del state["log"][:]
        cls._detector = staticmethod((lambda: "scripted detector") if detector else (lambda: None))
        o_t, w_t = torch.from_numpy(originals.copy()), torch.from_numpy(work.copy())
        ctx = {"original_frames": o_t, "entries": [dict(e, box=tuple(e["box"]) if e["box"] else None) for e in entries], "ltx_frame_offset": offset}
        out, masks, repaired = cls().composite(w_t, ctx, feather, smoothing)
        assert torch.equal(o_t, torch.from_numpy(originals)) and torch.equal(w_t, torch.from_numpy(work)), key
        assert state["landmark_calls"] == 2 * len(order) and len(state["log"]) == 1, key
        # which frames the reference warped: replay its bookkeeping only to place the recorded transforms on their frames
        applied, it = [None] * n_o, iter(state["applied"])
        have, shot = False, None
        for k in order:
            e = entries[k]
            if e.get("hard_cut") or (shot is not None and e.get("shot_id", 0) != shot):
                have = False
            shot = e.get("shot_id", 0)
            have = have or (detector and script[k] is not None)
            if have:
                applied[k] = [float(v) for v in next(it).reshape(-1)]
        assert next(it, None) is None, key
        out_np, mask_np = out.contiguous().numpy(), masks.contiguous().numpy()
        case.update(repaired=int(repaired), aligned=sum(a is not None for a in applied), log=state["log"][0], applied=applied,
                    out_sha256=WS.sha(out_np), mask_sha256=WS.sha(mask_np))
        flat[key + ".out_samples"] = out_np.reshape(-1)[WS.sample_positions(out_np.size, case["seed"])]
        flat[key + ".mask_samples"] = mask_np.reshape(-1)[WS.sample_positions(mask_np.size, case["seed"])]
        folds = 0
        for k, a in enumerate(applied):
            if a is not None:
                l, t, r, b = entries[k]["box"]
                sx, sy, _, _ = WS.positions(np.array(a, dtype=np.float32).reshape(2, 3), r - l, b - t)
                folds = max(folds, int(np.ceil(max(np.abs(sx).max() / max(1, r - l - 1), np.abs(sy).max() / max(1, b - t - 1)))))
        case["reflections_at_most"] = folds
        cases.append(case)
        print(f"{key}: repaired {case['repaired']}, aligned {case['aligned']}, reflections <= {folds}; {case['log']}", flush=True)
    torch.sqrt = vendor_sqrt
    assert max(c["reflections_at_most"] for c in cases) >= 3                  # the border fold really iterates somewhere
    meta = {"cases": cases, "samples": WS.SAMPLES,
            "provenance": {"torch": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(),
                           "ATEN_CPU_CAPABILITY": os.environ.get("ATEN_CPU_CAPABILITY"),
                           "sqrt": "correctly rounded (numpy), in place of torch's vendor-library sqrt",
                           "warpAffine": "tests/warp_support.py restated() -- a restatement of cv2's uint8 INTER_LANCZOS4 / BORDER_REFLECT101 "
                                         "affine remap, NOT cv2 itself: equality with cv2 is unpinned until tests/golden/warp_lanczos4_cv2.npz exists",
                           "source": "VRGDGFaceFixCompositeLandmarkAligned.composite of the reference's VRGDG_StandaloneFaceFixNodes.py, its text "
                                     "unmodified, run on the CPU with a stub cv2 module and scripted _detector / _landmarks / estimateAffinePartial2D"}}
    _write_npz(os.path.join(GOLDEN, "landmark.npz"), flat)
    with open(os.path.join(GOLDEN, "landmark.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print(f"landmark.npz: {len(flat)} arrays, {os.path.getsize(os.path.join(GOLDEN, 'landmark.npz'))} bytes")


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        env = dict(os.environ, ATEN_CPU_CAPABILITY="default")
        raise SystemExit(subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env).returncode)

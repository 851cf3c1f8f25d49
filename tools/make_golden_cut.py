"""Regenerate tests/golden/cut_score.json from the reference's own cut score.

    python tools/make_golden_cut.py

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT); the tests read the fixture only.  `_cut_score` of the reference's
VRGDGFaceFixPrepareShotAware is taken out of VRGDG_StandaloneFaceFixNodes.py by AST, its text unmodified (decorator included), and run on
the frames quantised as line :456 of the same file quantises them.  cv2 is not installed here: the `cv2` it imports is a numpy stand-in
with the five functions it calls -- resize INTER_AREA and cvtColor RGB2HSV from tests/cut_support.py (the independent restatement the
kernels are tested against), calcHist with cv2's own bin rule floor(v * bins / range) in double, normalize (L2, the scale applied in
float32) and compareHist (HISTCMP_CORREL in double over the float32 histograms).  So the fixture pins the float32 / float64 ROUTE of the
reference (thumbnails divided by 255, float32 mean, requantisation, float histograms, normalisation, correlation) against the integer form
of this repository; equality of the stand-in's resize with cv2 itself is pinned separately (tests/test_cut_host.py,
test_cut_score_equals_cv2).

Per case the fixture keeps how the video is generated (kind, shape, seed: cut_support.make_video), the reference's scores and, for one or
two thresholds, the hard_cut flags and shot ids the rule of VRGDGFaceFixPrepareShotAware.prepare (:457-459) gives.  `gap` is the largest
difference between the reference's scores and cut_scores_from_sums on the same thumbnails; the tests allow 4 x gap.
"""
from __future__ import annotations

import ast
import json
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# key, kind (cut_support.make_video), shape [F, H, W, C], seed
CASES = (
    ("hard_cuts_160x90", "hard_cuts", (9, 90, 160, 3), 1101),
    ("hard_cuts_480x270", "hard_cuts", (7, 270, 480, 3), 1102),
    ("cut_to_noise_128", "cut_to_noise", (6, 128, 128, 3), 1103),
    ("fade_320x180", "fade", (9, 180, 320, 3), 1104),
    ("fast_fade_160x90", "fast_fade", (8, 90, 160, 3), 1105),
    ("flash_130x96_rgba", "flash", (7, 96, 130, 4), 1106),
    ("flash_512", "flash", (5, 512, 512, 3), 1107),
    ("identical_67x65", "identical", (5, 65, 67, 3), 1108),
    ("single_colour_64", "single_colour", (10, 64, 64, 3), 1109),
    ("single_colour_200x120", "single_colour", (8, 120, 200, 3), 1110),
    ("black_white_96", "black_white", (6, 96, 96, 3), 1111),
    ("drift_448x256", "drift", (8, 256, 448, 3), 1112),
    ("cut_same_palette_160x90", "cut_same_palette", (6, 90, 160, 3), 1113),
    ("out_of_range_854x480", "out_of_range", (6, 480, 854, 3), 1114),
    ("one_frame", "identical", (1, 64, 80, 3), 1115),
)
DEFAULT_SENSITIVITY = 0.28


def _reference_cut_score():
    """VRGDGFaceFixPrepareShotAware._cut_score, its text unmodified: the FunctionDef (with its staticmethod decorator) is compiled inside
    an otherwise empty class; nothing of the file is written anywhere."""
    from oracle import reference_loader as RL
    path = os.path.join(RL.REFERENCE_ROOT, "VRGDG_StandaloneFaceFixNodes.py")
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "VRGDGFaceFixPrepareShotAware")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_cut_score")
    holder = ast.ClassDef(name="Holder", bases=[], keywords=[], body=[fn], decorator_list=[])
    if "type_params" in ast.ClassDef._fields:
        holder.type_params = []
    module = ast.fix_missing_locations(ast.Module(body=[holder], type_ignores=[]))
    ns = {}
    exec(compile(module, path, "exec"), ns)
    return ns["Holder"]._cut_score


def _cv2_stand_in(CS):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_AREA, cv2.COLOR_RGB2HSV, cv2.HISTCMP_CORREL = 3, 41, 0

    def resize(src, dsize, interpolation=None):
        assert tuple(dsize) == (64, 64) and interpolation == cv2.INTER_AREA and src.dtype == np.uint8
        return CS.resize_area_u8(src)

    def cvtColor(src, code):
        assert code == cv2.COLOR_RGB2HSV and src.dtype == np.uint8
        h, s = CS.hsv(src)
        return np.stack([h, s, src.max(axis=-1).astype(np.int64)], axis=-1).astype(np.uint8)

    def calcHist(images, channels, mask, histSize, ranges):
        assert len(images) == 1 and list(channels) == [0, 1] and mask is None and list(histSize) == [32, 32] and list(ranges) == [0, 180, 0, 256]
        img = images[0].astype(np.float64)
        hb = np.floor(img[..., 0] * (32 / 180.0)).astype(np.int64)
        sb = np.floor(img[..., 1] * (32 / 256.0)).astype(np.int64)
        keep = (hb >= 0) & (hb < 32) & (sb >= 0) & (sb < 32)
        return np.bincount((hb * 32 + sb)[keep].ravel(), minlength=1024).astype(np.float32).reshape(32, 32)

    def normalize(src, dst):
        assert dst is None and src.dtype == np.float32
        norm = math.sqrt(float((src.astype(np.float64) ** 2).sum()))
        scale = 1.0 / norm if norm > np.finfo(np.float64).eps else 0.0
        return (src * np.float32(scale)).astype(np.float32)

    def compareHist(a, b, method):
        assert method == cv2.HISTCMP_CORREL and a.dtype == np.float32 and b.dtype == np.float32
        h1, h2 = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
        s1, s2, s11, s22, s12 = h1.sum(), h2.sum(), (h1 * h1).sum(), (h2 * h2).sum(), (h1 * h2).sum()
        scale = 1.0 / h1.size
        num = s12 - s1 * s2 * scale
        denom2 = (s11 - s1 * s1 * scale) * (s22 - s2 * s2 * scale)
        return num / math.sqrt(denom2) if abs(denom2) > np.finfo(np.float64).eps else 1.0

    cv2.resize, cv2.cvtColor, cv2.calcHist, cv2.normalize, cv2.compareHist = resize, cvtColor, calcHist, normalize, compareHist
    return cv2


def _rule(scores, cut_sensitivity):
    """the lines of VRGDGFaceFixPrepareShotAware.prepare that turn a score into hard_cut and shot_id (:451, :457-459), frame by frame"""
    hard, shots, shot_id, previous = [], [], 0, None
    for index, score in enumerate(scores):
        hard_cut = previous is not None and score >= float(cut_sensitivity)
        if hard_cut:
            shot_id += 1
        hard.append(bool(hard_cut))
        shots.append(shot_id)
        previous = index
    return hard, shots


def main():
    import torch

    import cut_support as CS
    from conftest import load_package
    load_package()
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes as FF

    sys.modules["cv2"] = _cv2_stand_in(CS)
    cut_score = _reference_cut_score()
    cases, gap, gap_mean, gap_hist = [], 0.0, 0.0, 0.0
    for key, kind, shape, seed in CASES:
        x = CS.make_video(kind, shape, seed)
        video = torch.from_numpy(x.copy())
        scores, previous_rgb = [0.0], None
        for index in range(shape[0]):
            rgb = (video[index, ..., :3].detach().cpu().clamp(0, 1).numpy() * 255).round().astype("uint8")          # :456
            if previous_rgb is not None:
                scores.append(float(cut_score(previous_rgb, rgb)))
            previous_rgb = rgb
        assert torch.equal(video, torch.from_numpy(x))
        thumbs, hists, sums = CS.restated_sums(x)
        ours = FF.cut_scores_from_sums(sums)
        diff = float(np.abs(ours - np.asarray(scores)).max())
        gap = max(gap, diff)
        cases.append({"key": key, "kind": kind, "shape": list(shape), "seed": seed, "frames": "cut_support.make_video(kind, shape, seed)",
                      "scores": scores, "sums": [[int(v) for v in row] for row in sums]})
        print(f"{key}: scores {[round(s, 4) for s in scores]}, |ours - reference| <= {diff:.3e}", flush=True)
    bound = 4.0 * gap
    assert 0.0 < bound < 1e-5, bound
    margin = 100.0 * bound
    for case in cases:
        later = sorted(case["scores"][1:])
        thresholds = []
        if all(abs(s - DEFAULT_SENSITIVITY) >= margin for s in later):
            thresholds.append(DEFAULT_SENSITIVITY)
        # a second threshold in the middle of the widest gap between the scores: some frames on either side wherever the scores differ
        gaps = [(b - a, 0.5 * (a + b)) for a, b in zip(later, later[1:]) if b - a > 4 * margin]
        if gaps:
            thresholds.append(round(max(gaps)[1], 6))
        assert thresholds, case["key"]
        case["thresholds"] = []
        for t in thresholds:
            assert all(abs(s - t) >= margin for s in later), (case["key"], t)
            hard, shots = _rule(case["scores"], t)
            case["thresholds"].append({"cut_sensitivity": t, "hard_cut": hard, "shot_id": shots})
        print(f"{case['key']}: thresholds {thresholds}, cuts {[sum(t['hard_cut']) for t in case['thresholds']]}", flush=True)
    kinds = {c["kind"] for c in cases}
    assert len(cases) >= 12 and {"hard_cuts", "fade", "flash", "identical", "single_colour"} <= kinds
    assert any(any(t["hard_cut"]) for c in cases for t in c["thresholds"])
    meta = {"gap": gap, "bound": bound, "threshold_margin": margin, "cases": cases,
            "provenance": {"numpy": np.__version__, "torch": torch.__version__,
                           "source": "VRGDGFaceFixPrepareShotAware._cut_score of the reference's VRGDG_StandaloneFaceFixNodes.py, its text unmodified, "
                                     "run on frames quantised as its line 456 does, over a numpy stand-in for cv2 (resize INTER_AREA, cvtColor "
                                     "RGB2HSV, calcHist, normalize, compareHist); hard_cut / shot_id by the rule of its lines 457-459"}}
    with open(os.path.join(GOLDEN, "cut_score.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
        fh.write("\n")
    print(f"cut_score.json: {len(cases)} cases, gap {gap:.3e}, bound {bound:.3e}, {os.path.getsize(os.path.join(GOLDEN, 'cut_score.json'))} bytes")


if __name__ == "__main__":
    main()

"""Regenerate tests/golden/landmark_input.json / .npz from the reference's own `_landmarks`.

    python tools/make_golden_landmark_input.py [--cv2]

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT); the tests read the fixture only.  `_landmarks` is taken out of the
reference's VRGDG_StandaloneFaceFixNodes.py (class VRGDGFaceFixCompositeLandmarkAligned) by AST, its text unmodified.  cv2 is not
installed here: the `cv2` it imports is a numpy stand-in -- resize is the independent restatement of INTER_AREA in tests/grid_support.py
(the one the header and the kernel are tested against), cvtColor the channel flip.  The detector is a recorded one: its rows are a fixed
function of the bytes it is shown (tests/landmark_input_support.recorded_detector), and it notes the SHA-256 of every picture it sees.  So
the fixture pins the reference's host ROUTE -- the 2 x 2 guard, the fixed 320 x 320 input, the resize before the flip, the choice of the
best row, the scaling of the points -- and the bytes the restatement shows the detector; cv2's own pixels are not pinned by it.  Nothing of
the reference's text is written anywhere.

Per case the fixture keeps the seed, the box size, the kind of picture, the digests of the 320 x 320 B,G,R pictures the detector was shown
(none for a box below 2 x 2) and the points returned (float32, in the .npz; absent: None).

--cv2: where the cv2 package is installed, also write tests/golden/landmark_input_cv2.npz -- cv2's own thumbnails of
landmark_input_support.cv2_pin_inputs() -- for machines without it."""
from __future__ import annotations

import ast
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# key, box (h, w), kind, seed: every rule, a box below 2 x 2 and a picture without a face
SPECS = (
    ("copy_320", (320, 320), "uniform", 11),
    ("fast2x2_640", (640, 640), "uniform", 12),
    ("fast_960x1280", (960, 1280), "ramp", 13),
    ("general_321", (321, 321), "uniform", 14),
    ("general_333x517", (333, 517), "uniform", 15),
    ("general_1080x700", (1080, 700), "ramp", 16),
    ("linear_319", (319, 319), "checker", 17),
    ("linear_40", (40, 40), "uniform", 18),
    ("linear_2x2", (2, 2), "uniform", 19),
    ("linear_2x500", (2, 500), "uniform", 20),
    ("linear_200x400", (200, 400), "uniform", 21),
    ("below_2x2_1x5", (1, 5), "uniform", 22),
    ("no_face_96x80", (96, 80), "black", 23),
)


def _method(file_name, class_name, name):
    from oracle import reference_loader as RL
    path = os.path.join(RL.REFERENCE_ROOT, file_name)
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == class_name)
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == name)
    fn.decorator_list = []                                                     # a @staticmethod: called as a plain function here
    code = compile(ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[])), path, "exec")
    ns = {}
    exec(code, ns)
    return ns[name]


def _cv2_stand_in(G):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_AREA, cv2.COLOR_RGB2BGR = 3, 4

    class error(Exception):
        pass

    def resize(src, dsize, interpolation=None):
        assert interpolation == cv2.INTER_AREA and tuple(dsize) == (320, 320)
        return G.resize_area(np.ascontiguousarray(src), dsize[0], dsize[1])

    def cvtColor(src, code):
        assert code == cv2.COLOR_RGB2BGR
        return np.ascontiguousarray(src[..., ::-1])

    cv2.error, cv2.resize, cv2.cvtColor = error, resize, cvtColor
    return cv2


class RecordedDetector:
    def __init__(self, L):
        self.L, self.size, self.shown = L, None, []

    def setInputSize(self, size):
        self.size = tuple(size)

    def detect(self, bgr):
        assert self.size == (320, 320)
        self.shown.append(self.L.sha(bgr))
        return 1, self.L.recorded_detector(bgr)


def write_cv2_fixture(L):
    import cv2
    out = {key: cv2.cvtColor(cv2.resize(u8, (320, 320), interpolation=cv2.INTER_AREA), cv2.COLOR_RGB2BGR) for key, u8 in L.cv2_pin_inputs()}
    out["provenance"] = np.array(json.dumps({"cv2": cv2.__version__, "cases": [key for key, _ in L.cv2_pin_inputs()]}))
    np.savez_compressed(L.cv2_fixture_path(), **out)
    print(f"landmark_input_cv2: {len(out) - 1} thumbnails, {os.path.getsize(L.cv2_fixture_path())} bytes")


def main():
    import grid_support as G
    import landmark_input_support as L
    if "--cv2" in sys.argv:
        return write_cv2_fixture(L)
    sys.modules["cv2"] = _cv2_stand_in(G)
    landmarks = _method("VRGDG_StandaloneFaceFixNodes.py", "VRGDGFaceFixCompositeLandmarkAligned", "_landmarks")
    cases, arrays, modes = [], {}, set()
    for key, (h, w), kind, seed in SPECS:
        case = {"key": key, "box": [h, w], "kind": kind, "seed": seed}
        detector = RecordedDetector(L)
        points = landmarks(detector, L.case_image(case))
        case["shown"] = detector.shown
        case["points"] = points is not None
        if points is not None:
            assert points.dtype == np.float32 and points.shape == (5, 2)
            arrays[key] = points
        if detector.shown:
            modes.add(G.mode_of(h, w, 320, 320))
        cases.append(case)
        print(f"{key}: {h} x {w} {kind}: {len(detector.shown)} picture(s) shown, points {'yes' if points is not None else 'none'}", flush=True)
    assert modes == {G.COPY, G.FAST, G.FAST_2X2, G.GENERAL, G.LINEAR}
    assert landmarks(None, L.case_image(cases[0])) is None                     # no detector: no points
    meta = {"cases": cases,
            "provenance": {"numpy": np.__version__,
                           "source": "_landmarks of VRGDGFaceFixCompositeLandmarkAligned in the reference's VRGDG_StandaloneFaceFixNodes.py, its "
                                     "text unmodified, over a numpy stand-in for cv2 (resize = tests/grid_support.resize_area, cvtColor = the "
                                     "channel flip) and a recorded detector (tests/landmark_input_support.recorded_detector)"}}
    path_json, path_npz = L.golden_paths()
    with open(path_json, "w") as fh:
        json.dump(meta, fh, indent=1)
        fh.write("\n")
    np.savez_compressed(path_npz, **arrays)
    print(f"landmark_input: {len(cases)} cases, {os.path.getsize(path_json)} + {os.path.getsize(path_npz)} bytes")


if __name__ == "__main__":
    main()

"""Regenerate tests/golden/detect_prep.json from the reference's own face detection loop.

    python tools/make_golden_detect.py

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT); the tests read the fixture only.  Taken out of the reference's
VRGDG_StandaloneFaceFixNodes.py and VRGDG_FaceFix.py by AST, their text unmodified: `_iou`, `_detect`, `_detect_with_rotation` (and the
Builder's `_initial_regions`).  cv2 is not installed here: the `cv2` they import is a numpy stand-in -- getRotationMatrix2D,
invertAffineTransform, warpAffine, resize and dnn.blobFromImage from tests/detect_support.py (the independent restatement the header and
the kernels are tested against).  The network is a recorded fake: its outputs are fixed arrays, chosen so that the threshold, the clipping
to the region, the minimum size, both suppression passes and every angle take part; each call also checks that the blob it is fed is the
restatement's blob of that angle and region.  So the fixture pins the reference's host ROUTE (regions, decode, corner mapping, penalty,
suppression) in double; cv2's own pixels are not pinned by it.  Nothing of the reference's text is written anywhere.

Per case the fixture keeps the frame size, the mode, the caller's regions (Builder), the region lists per angle, the fake outputs per
angle and region (float32 values), the thresholds and the candidates the reference returned."""
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


def _functions(file_name, names):
    from oracle import reference_loader as RL
    path = os.path.join(RL.REFERENCE_ROOT, file_name)
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    defs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    code = compile(ast.fix_missing_locations(ast.Module(body=[defs[n] for n in names], type_ignores=[])), path, "exec")
    ns = {}
    exec(code, ns)
    return ns


def _cv2_stand_in(D):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR, cv2.BORDER_REPLICATE = 1, 1
    cv2.dnn = types.ModuleType("cv2.dnn")

    def getRotationMatrix2D(center, angle, scale):
        assert scale == 1.0
        width, height = center[0] * 2.0, center[1] * 2.0
        assert width == int(width) and height == int(height)
        return D.rotation(int(width), int(height), angle)[0]

    def _invert(matrix):
        m = np.array(matrix, dtype=np.float64)
        d = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
        d = 1.0 / d if d != 0 else 0.0
        a11, a22 = m[1, 1] * d, m[0, 0] * d
        m[0, 0] = a11
        m[0, 1] *= -d
        m[1, 0] *= -d
        m[1, 1] = a22
        b1 = -m[0, 0] * m[0, 2] - m[0, 1] * m[1, 2]
        b2 = -m[1, 0] * m[0, 2] - m[1, 1] * m[1, 2]
        m[0, 2], m[1, 2] = b1, b2
        return m

    def warpAffine(src, matrix, dsize, flags=None, borderMode=None):
        assert flags == cv2.INTER_LINEAR and borderMode == cv2.BORDER_REPLICATE and tuple(dsize) == (src.shape[1], src.shape[0])
        return D.warp_linear(src, _invert(matrix))

    def resize(src, dsize):
        assert tuple(dsize) == (300, 300)
        return D.resize_linear(np.ascontiguousarray(src))

    def blobFromImage(image, scale, size, mean, swapRB=False, crop=False):
        assert scale == 1.0 and tuple(size) == (300, 300) and tuple(mean) == D.MEAN and not swapRB and not crop
        return D.to_blob(image)[None]

    cv2.getRotationMatrix2D, cv2.invertAffineTransform, cv2.warpAffine, cv2.resize = getRotationMatrix2D, _invert, warpAffine, resize
    cv2.dnn.blobFromImage = blobFromImage
    return cv2


class FakeCaffe:
    """returns the recorded outputs in call order and checks every blob it is fed"""

    def __init__(self, outputs, blobs):
        self.outputs, self.blobs, self.calls, self.blob = list(outputs), list(blobs), 0, None

    def setInput(self, blob):
        self.blob = blob

    def forward(self):
        assert np.array_equal(self.blob[0], self.blobs[self.calls]), f"blob {self.calls} differs from the restatement"
        out = self.outputs[self.calls]
        self.calls += 1
        return out[None, None]


class FakeYuNet:
    def __init__(self, outputs, sizes):
        self.outputs, self.sizes, self.calls, self.size = list(outputs), list(sizes), 0, None

    def setInputSize(self, size):
        self.size = tuple(size)

    def detect(self, region):
        assert self.size == (region.shape[1], region.shape[0]) == self.sizes[self.calls]
        out = self.outputs[self.calls]
        self.calls += 1
        return 1, (out if len(out) else None)


def _faces(rng, width, height, count):
    out = []
    for _ in range(count):
        w = float(rng.uniform(0.06, 0.3) * min(width, height))
        h = w * float(rng.uniform(0.9, 1.4))
        out.append((float(rng.uniform(0, width - w)), float(rng.uniform(0, height - h)), w, h))
    return out


def fake_outputs(D, rng, width, height, angles, regions, kind, rows=5):
    """outputs[a][r]: float32 [rows, 7] (caffe) or [k, 15] (yunet): a few true faces seen from every angle and region they fall into --
    rotated, jittered, so that they overlap across regions and angles -- plus rows below the threshold, boxes that leave the region, tiny
    boxes and, for caffe, inverted ones"""
    faces = _faces(rng, width, height, 3)
    out = []
    for a, angle in enumerate(angles):
        forward = None if angle == 0 else D.rotation(width, height, angle)[0]
        per_angle = []
        for left, top, right, bottom in regions[a]:
            rw, rh = right - left, bottom - top
            if rw < 8 or rh < 8:
                per_angle.append(np.zeros((0, 7 if kind == "caffe" else 15), dtype=np.float32))
                continue
            items = []
            for x, y, w, h in faces:
                cx, cy = x + w / 2, y + h / 2
                if forward is not None:
                    cx, cy = forward[0, 0] * cx + forward[0, 1] * cy + forward[0, 2], forward[1, 0] * cx + forward[1, 1] * cy + forward[1, 2]
                jx, jy, jw = rng.normal(0, 0.04 * w), rng.normal(0, 0.04 * h), rng.uniform(0.9, 1.1)
                x1, y1, x2, y2 = cx - jw * w / 2 + jx, cy - jw * h / 2 + jy, cx + jw * w / 2 + jx, cy + jw * h / 2 + jy
                if x2 < left or y2 < top or x1 > right or y1 > bottom:
                    continue
                items.append((float(rng.uniform(0.35, 0.999)), x1, y1, x2, y2))
            items.append((float(rng.uniform(0.05, 0.6)), left - 0.2 * rw, top + 0.3 * rh, left + 0.15 * rw, top + 0.5 * rh))      # leaves the region
            items.append((float(rng.uniform(0.6, 0.95)), left + 0.5 * rw, top + 0.5 * rh, left + 0.5 * rw + rng.uniform(1, 30), top + 0.5 * rh + rng.uniform(1, 30)))
            items.append((float(rng.uniform(0.6, 0.95)), right - 0.1 * rw, bottom - 0.1 * rh, right + 0.3 * rw, bottom + 0.2 * rh))
            if kind == "caffe":
                items.append((0.9, left + 0.6 * rw, top + 0.6 * rh, left + 0.4 * rw, top + 0.4 * rh))                            # inverted
                arr = np.array([[0.0, 1.0, s, (x1 - left) / rw, (y1 - top) / rh, (x2 - left) / rw, (y2 - top) / rh] for s, x1, y1, x2, y2 in items],
                               dtype=np.float32)
            else:
                arr = np.array([[x1 - left, y1 - top, x2 - x1, y2 - y1] + [0.0] * 10 + [s] for s, x1, y1, x2, y2 in items], dtype=np.float32)
            per_angle.append(arr[rng.permutation(len(arr))][:rows + 3])
        out.append(per_angle)
    return out


def main():
    import detect_support as D
    sys.modules["cv2"] = _cv2_stand_in(D)
    alone = _functions("VRGDG_StandaloneFaceFixNodes.py", ["_iou", "_detect", "_detect_with_rotation"])
    builder = _functions("VRGDG_FaceFix.py", ["_iou", "_initial_regions", "_detect", "_detect_with_rotation"])
    rng = np.random.Generator(np.random.PCG64(20261017))
    cases = []
    specs = [
        ("alone_light_640x420", "alone", (420, 640), "Light: ±15°", None, "caffe", 0.5, 20),
        ("alone_strong_600x600", "alone", (600, 600), "Strong: ±15° and ±30°", None, "caffe", 0.7, 12),
        ("alone_strong_97x61", "alone", (61, 97), "Strong: ±15° and ±30°", None, "caffe", 0.4, 4),
        ("alone_off_600x400", "alone", (400, 600), "Off (fastest)", None, "caffe", 0.5, 20),
        ("alone_unknown_mode", "alone", (400, 599), "something else", None, "caffe", 0.3, 8),
        ("alone_yunet_light", "alone", (420, 640), "Light: ±15°", None, "yunet", 0.5, 16),
        ("builder_light_regions", "builder", (330, 500), "light", [(17, 23, 25, 31), (0, 0, 7, 50), (100, 20, 400, 320), (381, 241, 500, 330)], "caffe", 0.5, 0),
        ("builder_strong_800x600", "builder", (600, 800), "STRONG", None, "caffe", 0.6, 0),
        ("builder_none_mode_605x405", "builder", (405, 605), None, None, "caffe", 0.45, 0),
        ("builder_yunet_off", "builder", (400, 600), "off", [(50, 60, 350, 360), (0, 0, 600, 400)], "yunet", 0.5, 0),
    ]
    for key, module, (height, width), mode, own, kind, confidence, minimum in specs:
        is_builder = module == "builder"
        angles = (D.ANGLES.get(str(mode or "light").lower(), [0, -15, 15]) if is_builder else D.ANGLES.get(str(mode), [0]))
        initial = [tuple(r) for r in (builder["_initial_regions"](width, height) if is_builder else D.regions_of(width, height))]
        caller = initial if own is None else [tuple(r) for r in own]
        regions = [caller if (a == 0 or not is_builder) else initial for a in angles]
        outputs = fake_outputs(D, rng, width, height, angles, regions, kind)
        bgr = D.make_frames("smooth", (1, height, width, 3), "u8", 77 + len(cases))[0]
        scanned = [(a, r) for a in range(len(angles)) for r, reg in enumerate(regions[a]) if not is_builder or (reg[2] - reg[0] >= 8 and reg[3] - reg[1] >= 8)]
        flat = [outputs[a][r] for a, r in scanned]
        if kind == "caffe":
            blobs = [D.blob(bgr, None if angles[a] == 0 else D.rotation(width, height, angles[a])[1], regions[a][r]) for a, r in scanned]
            net = {"kind": "caffe", "net": FakeCaffe(flat, blobs)}
        else:
            net = {"kind": "yunet", "net": FakeYuNet(flat, [(regions[a][r][2] - regions[a][r][0], regions[a][r][3] - regions[a][r][1]) for a, r in scanned])}
        if is_builder:
            got = builder["_detect_with_rotation"](net, bgr, confidence, caller, mode)
        else:
            got = alone["_detect_with_rotation"](net, bgr, confidence, minimum, mode)
        assert net["net"].calls == len(flat), (key, net["net"].calls, len(flat))
        cases.append({"key": key, "module": module, "width": width, "height": height, "rotation_assist": mode, "regions": own and [list(r) for r in own],
                      "kind": kind, "confidence": confidence, "minimum_pixels": minimum, "angles": angles,
                      "region_lists": [[list(r) for r in per] for per in regions],
                      "outputs": [[[[float(v) for v in row] for row in arr] for arr in per] for per in outputs],
                      "candidates": [[float(v) for v in item] for item in got]})
        print(f"{key}: {len(angles)} angles, {len(flat)} scanned regions, {sum(len(o) for o in flat)} rows -> {len(got)} candidates", flush=True)
    assert any(len(c["candidates"]) >= 3 for c in cases)
    meta = {"cases": cases,
            "provenance": {"numpy": np.__version__,
                           "source": "_iou, _detect, _detect_with_rotation (and _initial_regions) of the reference's VRGDG_StandaloneFaceFixNodes.py "
                                     "and VRGDG_FaceFix.py, their text unmodified, over a numpy stand-in for cv2 (getRotationMatrix2D, "
                                     "invertAffineTransform, warpAffine, resize, dnn.blobFromImage) and a recorded fake net"}}
    path = D.golden_path()
    with open(path, "w") as fh:
        json.dump(meta, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"detect_prep: {len(cases)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

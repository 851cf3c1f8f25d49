"""Regenerate tests/golden/facefix_builder.{json,npz} from the reference's own Builder Face Fix.

    python tools/make_golden_facefix_builder.py

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT); the tests read the fixture only.  Taken out of the reference's
VRGDG_FaceFix.py by AST, their text unmodified: `_color_match`, `_soft_ellipse_mask`, `_square_crop_box`, the two assignments of
finalize_face_fix that read `feather` and `color_match` from the payload, and its `for entry in repair_entries:` loop, which is compiled on
its own and executed in a namespace that holds what the lines before it would have set.  cv2 is not installed here: the `cv2` they import
is a numpy stand-in -- resize = tests/lanczos_support.restated, ellipse and GaussianBlur from tests/facefix_builder_support.py (the
independent restatement the header and the kernels are tested against), imread / imwrite backed by a dict; `_absolute_existing_file` is the
identity.  So the fixture pins the reference's float and byte ROUTE (numpy's fp32 means in raster order, the fp32 blend, the truncations,
the paste); cv2's own ellipse rasteriser and Gaussian arithmetic are NOT pinned by it (tests/test_facefix_builder_host.py pins them
wherever cv2 or tests/golden/facefix_builder_cv2.npz is at hand).  Nothing of the reference's text is written anywhere.

Per case the fixture keeps the recipe of the inputs (kind, shape, seed: facefix_builder_support.make_frames), the boxes, strengths and
settings, and the reference route's bytes inside every box (outside it the route leaves the original).  `gap_mask` is the largest distance
of an fp32 mask of the cases from the float64 yardstick; the tests allow 4 x that.  `large_box_measurement` is a measurement, not a test:
on a 1024 x 1024 box with more than 65,793 selected pixels numpy's fp32 running mean drifts from the exact mean this repository uses; it
records the share of bytes that differ and by how many levels.
"""
from __future__ import annotations

import ast
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _reference_parts():
    from oracle import reference_loader as RL
    path = os.path.join(RL.REFERENCE_ROOT, "VRGDG_FaceFix.py")
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    defs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    finalize = defs["finalize_face_fix"]
    loop = next(n for n in finalize.body if isinstance(n, ast.For) and isinstance(n.iter, ast.Name) and n.iter.id == "repair_entries")
    settings = [n for n in finalize.body if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name)
                and n.targets[0].id in ("feather", "color_match")]
    assert [n.targets[0].id for n in settings] == ["feather", "color_match"]

    def code(nodes):
        return compile(ast.fix_missing_locations(ast.Module(body=list(nodes), type_ignores=[])), path, "exec")

    return code([defs["_color_match"], defs["_soft_ellipse_mask"], defs["_square_crop_box"]]), code(settings), code([loop])


def _cv2_stand_in(FS, LS, files):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LANCZOS4 = 4

    def imread(path):
        return files[path].copy() if path in files else None

    def imwrite(path, image):
        files[path] = np.array(image, copy=True)
        return True

    def resize(src, dsize, interpolation=None):
        assert interpolation == cv2.INTER_LANCZOS4 and src.dtype == np.uint8 and src.ndim == 3
        return np.array(LS.restated(np.ascontiguousarray(src)[None], int(dsize[0]), int(dsize[1]))[0], copy=True)

    def ellipse(img, center, axes, angle, start_angle, end_angle, color, thickness):
        assert (angle, start_angle, end_angle, thickness) == (0, 0, 360, -1) and img.dtype == np.float32
        h, w = img.shape
        img[FS.spans_to_plane(FS.ellipse_spans(w, h, tuple(center), tuple(axes)), w, np.uint8).astype(bool)] = color
        return img

    def GaussianBlur(src, ksize, sigma):
        assert src.dtype == np.float32 and ksize[0] == ksize[1] and ksize[0] % 2 == 1
        return FS.blur(src, FS.gauss_coeffs(int(ksize[0]), float(sigma)))

    cv2.imread, cv2.imwrite, cv2.resize, cv2.ellipse, cv2.GaussianBlur = imread, imwrite, resize, ellipse, GaussianBlur
    return cv2


class Route:
    """the reference's functions and loop over the stand-in"""

    def __init__(self, FS, LS):
        self.files = {}
        sys.modules["cv2"] = self.cv2 = _cv2_stand_in(FS, LS, self.files)
        functions, self.settings_code, self.loop_code = _reference_parts()
        self.ns = {"os": os, "json": json}
        exec(functions, self.ns)

    def settings(self, payload):
        ns = {"payload": payload}
        exec(self.settings_code, ns)
        return {"feather": ns["feather"], "color_match": ns["color_match"]}

    def composite(self, originals, enhanced, boxes, strengths, feather, color_match):
        """finalize_face_fix's loop over the entries of one batch -> the composited frames (the originals where the loop wrote nothing).
        `feather` and `color_match` are what the lines before the loop hand it (a 0 can only get there past the payload's `or`)."""
        self.files.clear()
        entries, k = [], 0
        for f, box in enumerate(boxes):
            if box is None:
                continue
            e, k = enhanced[k], k + 1
            self.files[f"original_{f}"], self.files[f"ltx_{f}"] = originals[f], e
            entries.append({"frame_number": f, "original_path": f"original_{f}", "ltx_frame_path": f"ltx_{f}", "crop_box": list(box),
                            "composite_strength": strengths[f]})
        repair = [entry for entry in entries if float(entry.get("composite_strength") or 0.0) > 0.0]          # :923, restated: the selection
        ns = dict(self.ns)
        ns.update({"feather": feather, "color_match": color_match})
        ns.update({"cv2": self.cv2, "np": np, "repair_entries": repair, "_absolute_existing_file": lambda value, label: value,
                   "composited_folder": "composited", "composited_by_frame": {}, "faded_frames": 0})
        exec(self.loop_code, ns)
        out = originals.copy()
        for frame, path in ns["composited_by_frame"].items():
            out[frame] = self.files[path]
        return out


def _write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps: the same bytes on every run"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    import facefix_builder_support as FS
    import lanczos_support as LS
    route = Route(FS, LS)
    arrays, gap_mask, seen = {}, 0.0, set()

    composites = []
    for key in sorted(FS.COMPOSITE_CASES):
        (eh, ew), kind, boxes, strengths, feather, cm = FS.COMPOSITE_CASES[key]
        originals, enhanced, _, _, _, _ = FS.case_inputs(key)
        keep = originals.copy()
        want = route.composite(originals, enhanced, boxes, strengths, feather, cm)
        assert np.array_equal(originals, keep)
        ours = FS.composite(originals, enhanced, boxes, strengths, feather, cm)
        assert np.array_equal(ours, want), key                              # every selected count is far below 65,793: bit-equal means
        selected_max, clipped = 0, [False, False]
        for f, box in enumerate(boxes):
            outside = np.ones(originals.shape[1:3], dtype=bool)
            if box is not None:
                left, top, right, bottom = box
                outside[top:bottom, left:right] = False
                arrays[f"composite.{key}.{f}"] = want[f, top:bottom, left:right]
                w, h = right - left, bottom - top
                mask = FS.soft_ellipse_mask(w, h, feather)
                selected_max = max(selected_max, int((mask > np.float32(0.35)).sum()))
                if (w, h, feather) not in seen:
                    seen.add((w, h, feather))
                    gap_mask = max(gap_mask, float(np.abs(mask.astype(np.float64) - FS.yardstick_mask(w, h, feather)).max()))
                if strengths[f] >= 1.0 and cm >= 1.0 and selected_max >= 16:
                    inner = want[f, top:bottom, left:right][mask >= 1.0]
                    clipped[0] |= bool((inner == 0).any())
                    clipped[1] |= bool((inner == 255).any())
            assert np.array_equal(want[f][outside], originals[f][outside])
            if box is None or strengths[f] <= 0:
                assert np.array_equal(want[f], originals[f])
        if kind == "bright":
            assert clipped[0], key
        if kind == "dark":
            assert clipped[1], key
        composites.append({"key": key, "originals": {"kind": "smooth", "shape": list(FS.FRAMES_SHAPE), "seed": FS.FRAMES_SEED},
                           "enhanced": {"kind": kind, "shape": list(enhanced.shape), "seed": 5000 + sum(map(ord, key))},
                           "boxes": [list(b) if b else None for b in boxes], "strengths": strengths, "feather": feather, "color_match": cm,
                           "selected_max": selected_max})
        print(f"{key}: {sum(b is not None for b in boxes)} boxes, at most {selected_max} selected, reference route == restatement", flush=True)

    crops = []
    frames = FS.make_frames("random", FS.FRAMES_SHAPE, FS.FRAMES_SEED + 1)
    for size in FS.CROP_SIZES:
        for name in sorted(FS.CROP_BOXES):
            boxes = FS.CROP_BOXES[name][size] if isinstance(FS.CROP_BOXES[name], dict) else FS.CROP_BOXES[name]
            out = [route.cv2.resize(frames[f][b[1]:b[3], b[0]:b[2]], (size, size), interpolation=route.cv2.INTER_LANCZOS4)     # :475-476, restated
                   for f, b in enumerate(boxes) if b is not None]
            arrays[f"crop.{name}.{size}"] = np.stack(out)
            crops.append({"key": f"{name}.{size}", "frames": {"kind": "random", "shape": list(FS.FRAMES_SHAPE), "seed": FS.FRAMES_SEED + 1},
                          "boxes": [list(b) if b else None for b in boxes], "enhance_size": size})

    # host integers
    square = route.ns["_square_crop_box"]
    rng = np.random.Generator(np.random.PCG64(99))
    rows = []
    for width, height in ((1920, 1080), (3840, 2160), (160, 90), (720, 1280), (641, 479)):
        for _ in range(10):
            fw, fh = float(rng.uniform(4, width * 0.7)), float(rng.uniform(4, height * 0.9))
            box = (round(float(rng.uniform(-0.2 * width, width)), 3), round(float(rng.uniform(-0.2 * height, height)), 3), round(fw, 3), round(fh, 3))
            padding = round(float(rng.choice([0.0, 0.15, 0.35, 0.5, 1.0, -0.3])), 2)
            rows.append({"face_box": list(box), "width": width, "height": height, "padding": padding,
                         "result": [int(v) for v in square(box, width, height, padding)]})
    rows.append({"face_box": [10.5, 20.5, 41.0, 41.0], "width": 160, "height": 90, "padding": 0.0,
                 "result": [int(v) for v in square((10.5, 20.5, 41.0, 41.0), 160, 90, 0.0)]})
    settings = []
    for payload in ({}, {"feather": 0}, {"color_match": 0}, {"feather": 0, "color_match": 0}, {"feather": 300, "color_match": 2}, {"feather": -4},
                    {"feather": "24", "color_match": "0.4"}, {"feather": 7.9, "color_match": -1}, {"feather": None, "color_match": None},
                    {"feather": 256, "color_match": 1}, {"feather": 1, "color_match": 0.001}):
        settings.append({"payload": payload, "result": route.settings(dict(payload))})

    # the measurement beyond 65,793 selected pixels
    big = FS.make_frames("smooth", (1, 1024, 1024, 3), 7001)
    face = FS.make_frames("random", (1, 512, 512, 3), 7002)
    box, feather, cm = (0, 0, 1024, 1024), 18, 0.65
    want = route.composite(big, face, [box], [1.0], feather, cm)
    ours = FS.composite(big, face, [box], [1.0], feather, cm)
    diff = np.abs(want.astype(np.int16) - ours.astype(np.int16))
    selected = int((FS.soft_ellipse_mask(1024, 1024, feather) > np.float32(0.35)).sum())
    measurement = {"box": list(box), "feather": feather, "color_match": cm, "selected": selected,
                   "share_of_bytes_that_differ": float((diff != 0).mean()), "largest_difference_levels": int(diff.max())}
    print("large box:", measurement, flush=True)
    assert selected > 65793

    meta = {"gap_mask": gap_mask, "mask_bound": 4.0 * gap_mask, "composites": composites, "crops": crops, "square_crop_box": rows,
            "settings": settings, "large_box_measurement": measurement,
            "provenance": {"numpy": np.__version__,
                           "source": "_color_match, _soft_ellipse_mask, _square_crop_box, the feather / color_match assignments and the "
                                     "`for entry in repair_entries:` loop of finalize_face_fix of the reference's VRGDG_FaceFix.py, their text "
                                     "unmodified, over a numpy stand-in for cv2 (resize, ellipse, GaussianBlur, imread, imwrite)"}}
    with open(FS.FIXTURE_JSON, "w") as fh:
        json.dump(meta, fh, indent=1)
        fh.write("\n")
    _write_npz(FS.FIXTURE_NPZ, arrays)
    print(f"facefix_builder: {len(composites)} composites, {len(crops)} crop sets, gap_mask {gap_mask:.3e}; "
          f"{os.path.getsize(FS.FIXTURE_JSON)} + {os.path.getsize(FS.FIXTURE_NPZ)} bytes")


if __name__ == "__main__":
    main()

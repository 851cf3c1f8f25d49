"""Regenerate tests/golden/video_grid.json / .npz and tests/golden/video_grid_surface.json from the reference's own node.

    python tools/make_golden_grid.py
    python tools/make_golden_grid.py --cv2      (where cv2 can be imported: writes tests/golden/video_grid_cv2.npz, the cv2 pin)

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT); the tests read the fixtures only.  `_fit_frame_to_tile`,
`_build_grid_frames_from_images`, `_resolve_cell_size_from_images`, `_get_tensor_resolution` of VRGDG_VideoFolderGridPlot and `_choose_columns`
of its parent are taken out of LTXLoraTrain.py by AST, their text unmodified, and run on seeded inputs.  cv2 is not installed here: the
`cv2` they call is a numpy stand-in -- resize is the restatement of tests/grid_support.py (the independent restatement the kernels are
tested against), cvtColor flips the channels, getTextSize / putText draw grid_support.pattern_label, a deterministic pattern confined to
the band.  So the fixture pins the ROUTE of the reference (flattening, cell size, tile geometry with Python's round, placement, held last
frames, the byte grid divided by 255) against this repository; equality of the stand-in's resize with cv2 itself is pinned separately
(tests/test_grid_host.py, test_grid_equals_cv2).  The surface file holds the node's class attributes and INPUT_TYPES as plain settings.
"""
from __future__ import annotations

import ast
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WANTED = ("_fit_frame_to_tile", "_build_grid_frames_from_images", "_resolve_cell_size_from_images", "_get_tensor_resolution")
SURFACE = ("RETURN_TYPES", "RETURN_NAMES", "FUNCTION", "CATEGORY", "DESCRIPTION", "MAX_VIDEO_SLOTS")

# key, inputs [(shape, kind)], cell_width, cell_height, label_tiles, seed; what the case is there for
CASES = (
    ("one_auto_labels", [((2, 48, 64, 3), "uniform")], 0, 0, True, 2101),                                   # auto cells, copy, labels
    ("one_explicit_2x2", [((2, 96, 128, 3), "smooth")], 64, 48, False, 2102),                               # explicit cells, 2 x 2
    ("two_fast", [((3, 96, 192, 3), "uniform"), ((1, 64, 128, 3), "smooth")], 64, 32, False, 2103),          # 3 x 3 and 2 x 2, unequal lengths
    ("two_labels_general", [((2, 70, 131, 3), "uniform"), ((3, 67, 65, 3), "special")], 57, 70, True, 2104),  # general, labels, unequal sizes
    ("five_mixed", [((3, 48, 64, 3), "uniform"), ((1, 30, 40, 3), "smooth"), ((5, 96, 128, 3), "uniform"), ((2, 70, 131, 3), "smooth"),
                    ((4, 12, 20, 3), "special")], 64, 48, False, 2105),                                     # 5 tiles in 3 columns, every rule
    ("five_auto_height", [((2, 40, 60, 3), "uniform")] * 5, 35, 0, True, 2106),                             # auto height with the band, odd cells
    ("ten_tiles", [((1 + i % 3, 24 + 2 * i, 32 + 3 * i, 3), "uniform") for i in range(10)], 40, 36, False, 2107),
    ("single_image", [((33, 47, 3), "uniform"), ((2, 33, 47, 3), "smooth")], 47, 33, False, 2108),          # an [H, W, C] input
    ("rgba", [((2, 50, 70, 4), "uniform"), ((2, 64, 120, 4), "special")], 40, 32, False, 2109),             # C = 4, fast sx != sy
    ("linear_enlarge", [((2, 12, 20, 3), "uniform"), ((2, 5, 3, 3), "smooth")], 64, 78, True, 2110),         # enlarging, labels
    ("one_axis_equal", [((2, 48, 20, 3), "uniform")], 64, 48, False, 2111),                                 # one axis equal, one enlarged
    ("tall_in_wide", [((2, 90, 30, 3), "smooth"), ((2, 30, 90, 3), "uniform")], 60, 60, True, 2112),         # bars on either side
    ("auto_width", [((2, 36, 52, 3), "uniform"), ((1, 72, 104, 3), "uniform")], 0, 58, True, 2113),          # auto width only
    ("band_too_small", [((1, 40, 60, 3), "uniform")], 60, 50, True, 2114),                                  # 50 - 40 < 16: ValueError
)


def _reference_class():
    """The wanted methods, their text unmodified, compiled inside an otherwise empty class; nothing of the file is written anywhere."""
    from oracle import reference_loader as RL
    path = os.path.join(RL.REFERENCE_ROOT, "LTXLoraTrain.py")
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    classes = {n.name: n for n in tree.body if isinstance(n, ast.ClassDef)}
    node, parent = classes["VRGDG_VideoFolderGridPlot"], classes["VRGDG_LTXPreviewXYZPlot"]
    body = [n for n in node.body if isinstance(n, ast.FunctionDef) and n.name in WANTED + ("INPUT_TYPES",)]
    body += [n for n in parent.body if isinstance(n, ast.FunctionDef) and n.name == "_choose_columns"]
    body += [n for n in node.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") in SURFACE]
    body += [n for n in parent.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") in ("LABEL_BAND_HEIGHT", "VIDEO_EXTENSIONS")]
    holder = ast.ClassDef(name="Holder", bases=[], keywords=[], body=body, decorator_list=[])
    if "type_params" in ast.ClassDef._fields:
        holder.type_params = []
    module = ast.fix_missing_locations(ast.Module(body=[holder], type_ignores=[]))
    import math
    ns = {"np": np, "torch": torch, "math": math, "os": os}
    exec(compile(module, path, "exec"), ns)
    names = {k: v for k, v in zip(("class", "display"), _mappings(tree))}
    return ns, ns["Holder"], names


def _mappings(tree):
    out = []
    for name in ("NODE_CLASS_MAPPINGS", "NODE_DISPLAY_NAME_MAPPINGS"):
        node = next(n for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == name)
        keys = [k.value for k in node.value.keys]
        if name == "NODE_CLASS_MAPPINGS":
            out.append("VRGDG_VideoFolderGridPlot" in keys)
        else:
            out.append(next(v.value for k, v in zip(node.value.keys, node.value.values) if k.value == "VRGDG_VideoFolderGridPlot"))
    return out


def _cv2_stand_in(G):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_AREA, cv2.COLOR_RGB2BGR, cv2.COLOR_BGR2RGB, cv2.FONT_HERSHEY_SIMPLEX, cv2.LINE_AA = 3, 4, 4, 0, 16

    def resize(src, dsize, interpolation=None):
        assert interpolation == cv2.INTER_AREA and src.dtype == np.uint8
        return G.resize_area(src, int(dsize[0]), int(dsize[1]))

    def cvtColor(src, code):
        assert code == 4 and src.dtype == np.uint8
        return np.ascontiguousarray(src[..., 2::-1])             # code 4 takes 3 or 4 channels and gives 3

    def getTextSize(text, font, scale, thickness):
        return (8 * len(text), 12), 5

    def putText(canvas, text, org, font, scale, colour, thickness, line):
        h, w = canvas.shape[:2]
        label = G.pattern_label(text, w, h, G.LABEL_BAND)
        canvas[:G.LABEL_BAND] = np.maximum(canvas[:G.LABEL_BAND], label[:G.LABEL_BAND][..., ::-1])       # the canvas is B,G,R
        return canvas

    cv2.resize, cv2.cvtColor, cv2.getTextSize, cv2.putText = resize, cvtColor, getTextSize, putText
    return cv2


def main():
    import grid_support as G
    ns, Holder, names = _reference_class()
    ns["cv2"] = _cv2_stand_in(G)
    node = Holder()
    cases, arrays = [], {}
    for key, inputs, cell_w, cell_h, label_tiles, seed in CASES:
        case = {"key": key, "inputs": [[list(shape), kind] for shape, kind in inputs], "cell_width": cell_w, "cell_height": cell_h,
                "label_tiles": label_tiles, "seed": seed}
        batches = [torch.from_numpy(x) for x in G.golden_inputs(case)]
        labels = [f"video{i + 1}" for i in range(len(batches))]
        cw, ch = node._resolve_cell_size_from_images(batches, cell_w, cell_h, label_tiles)
        columns = node._choose_columns(len(batches))
        case.update(resolved_cell=[int(cw), int(ch)], columns=int(columns), labels=labels)
        try:
            grid = node._build_grid_frames_from_images(batches, int(cw), int(ch), int(columns), bool(label_tiles), labels)
        except ValueError as exc:
            case["raises"] = "ValueError"
            print(f"{key}: raises ValueError ({exc})")
        else:
            grid = grid.numpy()
            assert grid.dtype == np.float32
            bytes_ = np.rint(grid * 255.0).astype(np.uint8)
            assert np.array_equal(bytes_.astype(np.float32) / np.float32(255.0), grid)
            arrays[key] = bytes_                                   # the grid is bytes / 255: kept as bytes
            case["shape"] = list(grid.shape)
            print(f"{key}: {grid.shape}, {int((bytes_ != 0).sum())} non-zero bytes")
        cases.append(case)
    json_path, npz_path = G.golden_paths()
    with open(json_path, "w") as fh:
        json.dump({"provenance": "tools/make_golden_grid.py: the reference's own methods over a numpy stand-in for cv2; grids stored as "
                                 "uint8 (every value is byte / 255 in fp32)", "band": G.LABEL_BAND, "cases": cases}, fh, indent=1)
    np.savez_compressed(npz_path, **arrays)
    surface = {name: getattr(Holder, name) for name in SURFACE}
    surface = {k: list(v) if isinstance(v, tuple) else v for k, v in surface.items()}
    surface.update(LABEL_BAND_HEIGHT=Holder.LABEL_BAND_HEIGHT, VIDEO_EXTENSIONS=sorted(Holder.VIDEO_EXTENSIONS),
                   INPUT_TYPES=json.loads(json.dumps(Holder.INPUT_TYPES())), registered=names["class"], display_name=names["display"])
    with open(G.surface_path(), "w") as fh:
        json.dump(surface, fh, indent=1)
    print("wrote", json_path, npz_path, os.path.getsize(npz_path), "bytes;", G.surface_path())


def main_cv2():
    """cv2's own resizes of grid_support.cv2_pin_inputs() -- all five rules and 953 -> 413, where the two formations of the scale part"""
    import cv2
    import grid_support as G
    arrays, keys = {}, []
    for key, u8, (h, w) in G.cv2_pin_inputs():
        arrays[key] = cv2.resize(u8, (w, h), interpolation=cv2.INTER_AREA)
        keys.append(key)
    arrays["provenance"] = np.array(json.dumps({"cv2": cv2.__version__, "cases": keys}))
    np.savez_compressed(G.cv2_fixture_path(), **arrays)
    print("wrote", G.cv2_fixture_path(), os.path.getsize(G.cv2_fixture_path()), "bytes")


if __name__ == "__main__":
    main_cv2() if "--cv2" in sys.argv else main()

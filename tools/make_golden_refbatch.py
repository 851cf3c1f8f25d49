"""Record tests/golden/multi_reference.json from the reference's own VRGDG_MultiReferenceConditioning,
VRGDG_MultiReferenceConditioningFromPaths and VRGDG_ImageBatchMultiFromPaths classes (numbers, names, texts and settings only).

    python tools/make_golden_refbatch.py       # needs the reference checkout (VRGDG_REFERENCE_ROOT); no GPU

The three classes are taken from the reference's source (VRGDG_GeneralNodes2.py) by its AST and executed as they stand, with stand-ins
for what ComfyUI brings: ``comfy.utils.common_upscale`` records the size it is asked for and resamples with F.interpolate,
``node_helpers.conditioning_set_values`` records what is appended, ``folder_paths`` names three directories that do not exist.  Recorded:
  surface   per class INPUT_TYPES, RETURN_TYPES, RETURN_NAMES, FUNCTION, CATEGORY, DESCRIPTION, the display name; the method list
  sizes     (height, width) ``_scale_to_total_pixels`` asks common_upscale for, per (height, width, megapixels, resolution_steps)
  paths     what ``_parse_image_paths`` returns for every accepted form of its input
  errors    the texts of the refusals
  flow      what one ``apply`` call hands the encoder and the appender, and what it returns
"""
import ast
import json
import math
import os
import re
import sys
import types
from typing import List

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("VRGDG_REFERENCE_ROOT", "/root/reference")
FILENAME = "VRGDG_GeneralNodes2.py"
CLASSES = ("VRGDG_MultiReferenceConditioning", "VRGDG_MultiReferenceConditioningFromPaths", "VRGDG_ImageBatchMultiFromPaths")

# (height, width, megapixels, resolution_steps): the four hand-checked rows of the issue first
SIZE_CASES = [(1080, 1920, 1.0, 1), (333, 517, 0.25, 8), (7, 5, 0.01, 1), (4000, 3000, 16.0, 64),
              (1, 1, 0.01, 1), (1, 1, 1.0, 256), (3, 1, 0.008, 1), (20, 37, 0.0005, 4), (64, 48, 0.0005, 4), (33, 29, 0.008, 1),
              (16, 16, 256.0 / (1024 * 1024), 1), (512, 768, 1.0, 1), (768, 512, 1.0, 16), (2160, 3840, 1.0, 8), (2160, 3840, 16.0, 1),
              (1500, 1000, 0.5, 2), (1000, 1500, 0.5, 3), (599, 601, 0.3, 1), (2048, 2048, 1.0, 1), (100, 4000, 2.0, 32), (4000, 100, 2.0, 32),
              (17, 31, 0.01, 7), (2, 3, 16.0, 256), (1080, 1920, 0.01, 256)]
PATH_INPUTS = ["", "   \n ", "a.png", "a.png\nb.png", " a.png \r\n\r\n 'b c.png' \n\"d.png\"", '["a.png", "b.png"]', '["a.png", "", "  ", 7]',
               '{"image_paths": ["x.png", "y.png"]}', '{"images": ["x.png"]}', '{"one": "p.png", "two": "q.png"}',
               '[{"path": "a.png"}, {"file": "b.png"}, {"image": "c.png"}, {"other": "d.png"}]', '{"image_paths": "not a list", "images": ["z.png"]}',
               '"quoted.png"', "[broken json\nsecond line", "42"]


class Recorder:
    def __init__(self):
        self.sizes, self.appended, self.encoded = [], [], []

    def common_upscale(self, samples, width, height, upscale_method, crop):
        self.sizes.append({"height": int(height), "width": int(width), "method": upscale_method, "crop": crop})
        return F.interpolate(samples, size=(height, width), mode="nearest")

    def conditioning_set_values(self, conditioning, values, append=False):
        self.appended.append({"to": conditioning, "keys": sorted(values), "append": append,
                              "shapes": [list(v.shape) for v in values["reference_latents"]]})
        return conditioning + "+"

    def encode(self, pixels):
        self.encoded.append(list(pixels.shape))
        return torch.zeros(1, 16, pixels.shape[1] // 8, pixels.shape[2] // 8)


def load_classes(rec):
    path = os.path.join(REFERENCE_ROOT, FILENAME)
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
    assert [n.name for n in body] == list(CLASSES)
    display = next(ast.literal_eval(n.value) for n in tree.body
                   if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "NODE_DISPLAY_NAME_MAPPINGS")
    nowhere = os.path.join(os.sep, "nonexistent-vrgdg")
    ns = {"torch": torch, "math": math, "json": json, "re": re, "os": os, "np": np, "List": List, "Image": None, "ImageOps": None,
          "comfy": types.SimpleNamespace(utils=types.SimpleNamespace(common_upscale=rec.common_upscale)),
          "node_helpers": types.SimpleNamespace(conditioning_set_values=rec.conditioning_set_values),
          "folder_paths": types.SimpleNamespace(get_input_directory=lambda: os.path.join(nowhere, "input"),
                                                get_output_directory=lambda: os.path.join(nowhere, "output"),
                                                get_temp_directory=lambda: os.path.join(nowhere, "temp"))}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return [ns[c] for c in CLASSES], {c: display[c] for c in CLASSES}


def message(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except (ValueError, FileNotFoundError) as exc:
        return {"type": type(exc).__name__, "message": str(exc)}
    raise AssertionError("no error")


def main():
    rec = Recorder()
    (multi, from_paths, batch_multi), display = load_classes(rec)
    out = {"provenance": {"reference_file": FILENAME, "classes": list(CLASSES), "tool": "tools/make_golden_refbatch.py"},
           "upscale_methods": list(multi.upscale_methods), "max_images": multi.MAX_IMAGES, "surface": {}}
    for cls in (multi, from_paths, batch_multi):
        out["surface"][cls.__name__] = {"INPUT_TYPES": cls.INPUT_TYPES(), "RETURN_TYPES": list(cls.RETURN_TYPES),
                                        "RETURN_NAMES": list(cls.RETURN_NAMES), "FUNCTION": cls.FUNCTION, "CATEGORY": cls.CATEGORY,
                                        "DESCRIPTION": cls.DESCRIPTION, "display_name": display[cls.__name__]}
    out["sizes"] = []
    for h, w, mp, steps in SIZE_CASES:
        del rec.sizes[:]
        multi._scale_to_total_pixels(torch.zeros(1, h, w, 3), "bilinear", mp, steps)
        assert rec.sizes[0]["crop"] == "disabled"
        out["sizes"].append({"height": h, "width": w, "megapixels": mp, "resolution_steps": steps,
                             "result": [rec.sizes[0]["height"], rec.sizes[0]["width"]]})
    out["paths"] = [{"input": text, "result": from_paths._parse_image_paths(text)} for text in PATH_INPUTS]
    vae = types.SimpleNamespace(encode=rec.encode)
    out["errors"] = {
        "no_images": message(multi().apply, "P", "N", vae, 4, "bilinear", 1.0, 1),
        "no_paths": message(from_paths().apply, "P", "N", vae, "", "bilinear", 1.0, 1),
        "no_batch_paths": message(batch_multi().load_batch, "  ", "bilinear"),
        "empty_path": message(from_paths._resolve_image_path, " '' "),
        "missing_path": message(from_paths._resolve_image_path, "no-such-picture.png"),
    }
    # one apply: image_count 3 of which image2 is not connected; 0.0005 MP in steps of 4
    del rec.sizes[:], rec.appended[:], rec.encoded[:]
    images = {"image1": torch.rand(1, 20, 37, 3), "image3": torch.rand(2, 64, 48, 3), "image4": torch.rand(1, 9, 9, 3)}
    pos, neg, batch = multi().apply("P", "N", vae, 3, "bilinear", 0.0005, 4, **images)
    out["flow"] = {"inputs": {k: list(v.shape) for k, v in images.items()}, "image_count": 3, "megapixels": 0.0005, "resolution_steps": 4,
                   "encoded": list(rec.encoded), "appended": list(rec.appended), "returns": [pos, neg], "batch_shape": list(batch.shape),
                   "upscales": list(rec.sizes)}
    path = os.path.join(ROOT, "tests", "golden", "multi_reference.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())

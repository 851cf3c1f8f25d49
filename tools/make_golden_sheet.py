"""Write tests/golden/sheet.json + sheet.npz from the reference's own code (VRGDG_LTXICIngredientsGrid.py and the three sheet builders of
VRGDG_MusicVideoBuilderNodes.py), loaded through oracle/reference_loader.py.  Works only where the reference checkout exists.

    python tools/make_golden_sheet.py

Recorded: the normalised rects of every layout x count 1 .. 24 x columns {0, 1, 3, 12} and the aspect_rows rects of the aspect lists of
tests/sheet_support.py (float64 arrays in the npz, in the order of layout_keys() / aspect_keys()); the panel rectangles and the canvases (as bytes: the node's output x 255 is an exact integer) of the node cases,
whose inputs the tests regenerate from seeds; the large case by sha256; the three Builder sheets on seeded byte inputs."""
import hashlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sheet_support as S                      # noqa: E402
from oracle import reference_loader as RL      # noqa: E402


def canvas_bytes(out):
    a = out[0].numpy() * np.float32(255.0)
    b = np.rint(a).astype(np.uint8)
    assert np.array_equal(b.astype(np.float32) / np.float32(255.0), out[0].numpy())
    return b


def run_node(ref, case, inputs):
    kwargs = {k: torch.from_numpy(v) for k, v in inputs.items()}
    (out,) = ref.VRGDG_LTXICIngredientsGrid().build(**case, **kwargs)
    return out


def main():
    from PIL import Image
    import PIL
    ref = RL._load_file("_vrgdg_reference_ingredients_grid", "VRGDG_LTXICIngredientsGrid.py")
    doc = {"pillow": PIL.__version__, "panels": {}, "builder": {}}
    arrays = {}
    rects = [ref._layout_rects(*key) for key in S.layout_keys()]
    arrays["layout.counts"] = np.array([len(r) for r in rects], dtype=np.int32)
    arrays["layout.rects"] = np.array([v for r in rects for v in r], dtype=np.float64).reshape(-1, 4)

    class Sized:
        def __init__(self, aspect):
            self.size = (aspect * 1000.0, 1000.0)

    values, rects = [], []
    for aspects, canvas in S.aspect_keys():
        values += [Sized(a).size[0] / 1000.0 for a in aspects]
        rects += ref._aspect_row_rects([Sized(a) for a in aspects], *canvas)
    arrays["aspect.values"] = np.array(values, dtype=np.float64)
    arrays["aspect.rects"] = np.array(rects, dtype=np.float64).reshape(-1, 4)
    for name, case in S.NODE_CASES.items():
        arrays[f"node.{name}"] = canvas_bytes(run_node(ref, case, S.node_inputs(case)))
        # the integer rectangles, by the reference's own lines on its own rects
        frames = S.node_frames(case)
        images = [Image.fromarray(S.quantise(f), mode="RGB") for f in frames]
        w, h, pad, gutter = case["output_width"], case["output_height"], case["outer_padding"], case["gutter"]
        rects = ref._aspect_row_rects(images, w, h) if case["layout"] == "aspect_rows" else ref._layout_rects(case["layout"], len(images), case["columns"])
        uw, uh, boxes = max(1, w - 2 * pad), max(1, h - 2 * pad), []
        for x, y, rw, rh in rects:
            left, top = pad + int(round(x * uw)) + gutter // 2, pad + int(round(y * uh)) + gutter // 2
            right, bottom = pad + int(round((x + rw) * uw)) - gutter // 2, pad + int(round((y + rh) * uh)) - gutter // 2
            boxes.append([left, top, max(1, right - left), max(1, bottom - top)])
        doc["panels"][name] = boxes
    large = run_node(ref, S.LARGE_CASE, S.large_inputs())
    doc["large_sha256"] = hashlib.sha256(np.ascontiguousarray(canvas_bytes(large)).tobytes()).hexdigest()
    ns = {"Image": Image, "math": math}
    RL._ast_extract("VRGDG_MusicVideoBuilderNodes.py", ("_combine_subject_location_images", "_combine_flux_ingredient_images",
                                                        "_combine_story_reference_batch"), ns)
    for key in S.BUILDER_SIZES:
        images = [Image.fromarray(a, mode="RGB") for a in S.builder_inputs(key)]
        if key == "subject_location":
            out = ns["_combine_subject_location_images"](*images)
        elif key.startswith("flux"):
            out = ns["_combine_flux_ingredient_images"](images)
        else:
            out = ns["_combine_story_reference_batch"](images)
        a = np.asarray(out)
        doc["builder"][key] = {"size": list(out.size), "sha256": hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()}
        arrays[f"builder.{key}"] = a[::7, ::5].copy()                     # a lattice of the sheet beside its digest: small fixtures
    with open(S.FIXTURE_JSON, "w") as fh:
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(doc[k], sort_keys=True)}" for k in sorted(doc)) + "\n}\n")
    np.savez_compressed(S.FIXTURE_NPZ, **arrays)
    print(S.FIXTURE_JSON, os.path.getsize(S.FIXTURE_JSON), S.FIXTURE_NPZ, os.path.getsize(S.FIXTURE_NPZ))


if __name__ == "__main__":
    main()

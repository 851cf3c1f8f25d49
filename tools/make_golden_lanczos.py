"""Fixtures of the enhancer upscale.

    python tools/make_golden_lanczos.py --dimensions /path/to/reference     -> tests/golden/enhancer_dimensions.json
    python tools/make_golden_lanczos.py --cv2                               -> tests/golden/lanczos4_cv2.npz (needs an importable cv2)

--dimensions evaluates the reference's own _output_dimensions and _auto_batch_size (the two functions are taken out of its
VRGDG_StandaloneVideoEnhancerNodes.py by name and executed on their own: the module around them needs a ComfyUI) on a table of inputs and
records the answers: data only.  --cv2 records cv2.resize(..., INTER_LANCZOS4) on small seeded inputs, with the cv2 version in the
provenance: the pin of csrc/vrg_lanczos_math.hpp (tests/test_lanczos_host.py::test_lanczos_equals_cv2)."""
import argparse
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CV2_CASES = (("up2", (2, 54, 96, 3), (192, 108), 11), ("up1_77", (2, 54, 96, 3), (170, 96), 12), ("up3", (1, 72, 128, 3), (384, 216), 13),
             ("up1_5", (1, 60, 80, 3), (120, 90), 14), ("down2", (1, 64, 96, 3), (48, 32), 15), ("one", (1, 1, 1, 3), (7, 5), 16),
             ("odd", (1, 37, 53, 3), (131, 89), 17))


def reference_functions(reference_dir):
    path = os.path.join(reference_dir, "VRGDG_StandaloneVideoEnhancerNodes.py")
    tree = ast.parse(open(path).read())
    wanted = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("_output_dimensions", "_auto_batch_size")]
    scope = {}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), path, "exec"), scope)
    return scope["_output_dimensions"], scope["_auto_batch_size"]


def make_dimensions(reference_dir):
    dims, batch = reference_functions(reference_dir)
    sizes = [(1920, 1080), (1080, 1920), (1280, 720), (854, 480), (480, 854), (1366, 768), (640, 360), (3840, 2160), (4096, 2160), (2560, 1440),
             (3072, 1728), (2559, 1439), (1, 1), (0, 0), (-5, 7), (3, 1000), (1000, 3), (1919, 1079), (720, 720), (333, 777), (2048, 858),
             (1998, 1080), (3839, 2160), (1440, 1080), (960, 540), (1600, 900), (3200, 1800), (3201, 1800), (2560, 1441)]
    modes = ["original", "2k", "3k", "4k", "4K", " 2k ", None, "", "8k", 0]
    out = {"provenance": "the reference's _output_dimensions / _auto_batch_size evaluated by tools/make_golden_lanczos.py --dimensions",
           "output_dimensions": [{"width": w, "height": h, "upscale_resolution": m, "result": list(dims(w, h, m))} for w, h in sizes for m in modes],
           "auto_batch_size": [{"width": w, "height": h, "result": batch(w, h)} for w, h in sizes + [(1280, 721), (1920, 1081), (3200, 1801)]]}
    with open(os.path.join(GOLDEN, "enhancer_dimensions.json"), "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")
    print("wrote enhancer_dimensions.json:", len(out["output_dimensions"]), "+", len(out["auto_batch_size"]), "rows")


def make_cv2():
    import cv2
    arrays = {}
    for key, shape, (ow, oh), seed in CV2_CASES:
        x = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=shape, dtype=np.uint8)
        arrays[key + ".in"] = x
        arrays[key + ".out"] = np.stack([cv2.resize(f, (ow, oh), interpolation=cv2.INTER_LANCZOS4) for f in x])
    arrays["provenance"] = np.array(json.dumps({"cv2": cv2.__version__, "numpy": np.__version__, "cases": [c[0] for c in CV2_CASES]}))
    np.savez_compressed(os.path.join(GOLDEN, "lanczos4_cv2.npz"), **arrays)
    print("wrote lanczos4_cv2.npz with cv2", cv2.__version__)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dimensions", metavar="REFERENCE_DIR")
    ap.add_argument("--cv2", action="store_true")
    a = ap.parse_args()
    if a.dimensions:
        make_dimensions(a.dimensions)
    if a.cv2:
        make_cv2()
    if not (a.dimensions or a.cv2):
        ap.print_help()
        sys.exit(2)

"""Writes tests/golden/contact_sheet.npz: what the REFERENCE's own ``contact_sheet`` (scripts/far_face_repair_backend.py) pastes together
for the cases of tests/contact_sheet_support.py, through the installed Pillow.

    python tools/make_golden_contact_sheet.py

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT); the tests read the fixture only.  The function's text is taken out of the reference file by AST and executed here (none of it is kept): it runs over temporary PNGs and a
manifest, with ``Image.Image.save`` intercepted so that the sheet is recorded BEFORE the JPEG encode.  Stored per sheet case: the input
frames (``in.<key>.o<i>`` / ``.f<i>``; no fixed frame: no entry), the arguments (``args.<key>`` = limit, columns, thumb_width, count;
``inputs_of.<key>``: the case whose frames it uses) and the sheet (``sheet.<key>``); and ``Image.thumbnail`` / ``Image.reduce`` of the
thumbnail and reduce cases with their inputs (``thumb_in.<i>`` -> ``thumb.<i>``, ``reduce_in.<h>x<w>`` -> ``reduce.<fx>x<fy>.<h>x<w>``).
"""
import argparse
import ast
import json
import math
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contact_sheet_support as S  # noqa: E402
from oracle import reference_loader as RL  # noqa: E402

BACKEND = os.path.join(RL.REFERENCE_ROOT, "scripts", "far_face_repair_backend.py")


def reference_contact_sheet(path=BACKEND):
    """the reference's contact_sheet as a callable(originals, fixed, limit, columns, thumb_width) -> the pasted sheet"""
    with open(path) as fh:
        tree = ast.parse(fh.read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "contact_sheet")
    space = {"Image": Image, "json": json, "math": math, "Path": Path, "argparse": argparse}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), space)
    function = space["contact_sheet"]

    def run(originals, fixed, limit, columns, thumb_width):
        recorded = []
        real_save = Image.Image.save

        def save(self, fp, *args, **kwargs):
            if "quality" in kwargs:                                          # the sheet, before it is encoded
                recorded.append(np.array(self))
                return None
            return real_save(self, fp, *args, **kwargs)

        with tempfile.TemporaryDirectory() as tmp:
            base = Path(tmp)
            (base / "composited_frames").mkdir()
            entries = []
            for i, (o, f) in enumerate(zip(originals, fixed)):
                Image.fromarray(o, "RGB").save(base / f"original_{i:06d}.png")
                if f is not None:
                    Image.fromarray(f, "RGB").save(base / "composited_frames" / f"frame_{i:06d}.png")
                entries.append({"original_frame": str(base / f"original_{i:06d}.png"), "frame": i})
            (base / "manifest.json").write_text(json.dumps({"entries": entries}), encoding="utf-8")
            args = argparse.Namespace(manifest=str(base / "manifest.json"), repaired_dir=None, out=None, limit=limit, columns=columns,
                                      thumb_width=thumb_width)
            Image.Image.save = save
            try:
                function(args)
            finally:
                Image.Image.save = real_save
        assert len(recorded) == 1
        return recorded[0]

    return run


def main():
    if not os.path.isfile(BACKEND):
        raise SystemExit(f"make_golden_contact_sheet: {BACKEND} not found (set VRGDG_REFERENCE_ROOT)")
    run = reference_contact_sheet()
    out = {}
    for key, case in S.SHEET_CASES.items():
        originals, fixed = S.make_sheet_inputs(key)
        source = case.get("inputs", key)
        if source == key:
            for i, (o, f) in enumerate(zip(originals, fixed)):
                out[f"in.{key}.o{i}"] = o
                if f is not None:
                    out[f"in.{key}.f{i}"] = f
        out[f"inputs_of.{key}"] = np.array(source)
        out[f"args.{key}"] = np.array([case["limit"], case["columns"], case["thumb_width"], len(originals)], dtype=np.int64)
        out[f"sheet.{key}"] = run(originals, fixed, case["limit"], case["columns"], case["thumb_width"])
    for i, (_, request, resample, gap) in enumerate(S.THUMB_CASES):
        out[f"thumb_in.{i}"] = S.make_thumb_input(i)
        im = Image.fromarray(out[f"thumb_in.{i}"], "RGB")
        im.thumbnail(request, Image.Resampling(resample), reducing_gap=gap)
        out[f"thumb.{i}"] = np.array(im)
    for k, (h, w) in enumerate(S.REDUCE_SIZES[:3]):
        out[f"reduce_in.{h}x{w}"] = S.make_reduce_input(k)
        for fx, fy in S.REDUCE_FACTORS:
            out[f"reduce.{fx}x{fy}.{h}x{w}"] = np.array(Image.fromarray(out[f"reduce_in.{h}x{w}"], "RGB").reduce((fx, fy)))
    np.savez_compressed(S.FIXTURE_NPZ, **out)
    print(S.FIXTURE_NPZ, os.path.getsize(S.FIXTURE_NPZ), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()

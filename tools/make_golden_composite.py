"""Regenerate tests/golden/composite.npz (+ composite.json) from the reference's VRGDG_ImagePasteBack.py and the two composite classes of
its VRGDG_StandaloneFaceFixNodes.py.

    python tools/make_golden_composite.py

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT) and g++; the tests read the fixture only.  The work is done by a
CHILD process started with ATEN_CPU_CAPABILITY=default (torch's plain resampling kernels, as tools/make_golden_resize.py).  Two more
things are pinned there:
  * torch.sqrt.  torch's CPU build hands sqrt to a vendor vector library whose result is not the correctly rounded root (off by one ulp
    in under 1 % of the elements here, in far more under other processor settings of that library), so "the reference's CPU result"
    depends on the machine.  The child runs the reference with torch.sqrt = the correctly rounded root (numpy's, exact against fp64) --
    what the GPU, libm and torch's own loop compute.  Every case is also run with torch's sqrt as it is, and how far that moves the
    blend mask is recorded in composite.json ("vendor_sqrt").
  * rounding ties of the colour statistic.  A case whose fp64 mean (crop or original, any channel) lies within a relative 2^-40 of an
    fp32 rounding tie is reseeded, so that no summation order can flip the fp32 mean the tests compare.
The reference's own fp32 means are recorded by wrapping torch.Tensor.mean.  The archive is written with fixed member dates.
"""
from __future__ import annotations

import ast
import io
import json
import os
import subprocess
import sys
import tempfile
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
H, W = 22, 26

# Paste Back: name, originals (n, channels), crops (n, h, w, channels), CROP_DATA box, inset, feather, shape, color_match, mask shape or None
PASTE = (
    ("ellipse_up", (1, 3), (1, 8, 10, 3), (4, 2, 22, 18), 2, 4, "ellipse", 0.65, None),
    ("rectangle_down", (1, 3), (1, 36, 40, 3), (3, 2, 23, 19), 1, 3, "rectangle", 1.0, None),
    ("ellipse_step", (1, 3), (1, 8, 10, 3), (4, 2, 22, 18), 1, 0, "ellipse", 0.0, None),
    ("rectangle_step", (1, 3), (1, 8, 10, 3), (4, 2, 22, 18), 2, 0, "rectangle", 0.65, None),
    ("inset_past_half_ellipse", (1, 3), (1, 8, 10, 3), (4, 2, 22, 18), 50, 5, "ellipse", 0.65, None),
    ("inset_past_half_rectangle", (1, 3), (1, 8, 10, 3), (4, 2, 22, 18), 50, 5, "rectangle", 0.65, None),
    ("cut_right", (1, 3), (1, 8, 10, 3), (14, 4, 34, 18), 1, 3, "ellipse", 0.65, None),
    ("cut_bottom", (1, 3), (1, 8, 10, 3), (3, 12, 21, 36), 1, 3, "rectangle", 0.65, None),
    ("outside", (1, 3), (1, 8, 10, 3), (26, 3, 36, 12), 1, 3, "ellipse", 0.65, None),
    ("one_original_three_crops", (1, 3), (3, 8, 10, 3), (4, 2, 22, 18), 2, 4, "ellipse", 0.65, None),
    ("three_originals_one_crop", (3, 3), (1, 8, 10, 3), (4, 2, 22, 18), 2, 4, "rectangle", 0.65, None),
    ("mask_batch_longest", (1, 3), (2, 8, 10, 3), (4, 2, 22, 18), 0, 2, "rectangle", 0.65, (3, 7, 9)),
    ("mask_with_channels", (1, 3), (1, 30, 28, 3), (4, 2, 22, 18), 1, 3, "ellipse", 0.0, (1, 40, 33, 2)),
    ("crop_rgba_on_rgb", (1, 3), (1, 8, 10, 4), (4, 2, 22, 18), 2, 4, "ellipse", 0.65, None),
    ("crop_rgb_on_rgba", (1, 4), (1, 8, 10, 3), (4, 2, 22, 18), 2, 4, "ellipse", 0.65, None),
    ("crop_rgba_on_rgba", (1, 4), (1, 8, 10, 4), (4, 2, 22, 18), 2, 4, "rectangle", 1.0, None),
    ("few_selected", (1, 3), (1, 2, 2, 3), (9, 9, 12, 12), 0, 1, "rectangle", 0.65, None),
)
# a wide frame: box height + width past 128, where torch changes its bilinear kernel for the user mask
PASTE_WIDE = ("wide_masked", (1, 3), (1, 9, 40, 3), (2, 1, 112, 27), 2, 6, "ellipse", 0.65, (1, 6, 21))
WIDE_H, WIDE_W = 28, 116

# Face Fix: name, originals (n, channels), work (n, h, w, channels), offset, feather, color_match, entries
FACEFIX = (
    ("offset_mixed", (5, 3), (6, 9, 11, 3), 1, 18, 0.65,
     [{"box": (3, 2, 23, 20), "strength": 1.0}, {"box": None, "strength": 1.0}, {"box": (3, 2, 23, 20), "strength": 0.0},
      {"box": (1, 3, 19, 21), "strength": 0.5}, {"box": (0, 0, 26, 22), "strength": 1.0}]),
    ("tail_preserved", (6, 4), (3, 40, 44, 3), 0, 4, 0.0,
     [{"box": (2, 1, 20, 17), "strength": 1.0}, {"box": (6, 5, 25, 22), "strength": 0.5}, {"box": (2, 1, 20, 17), "strength": 1.0},
      {"box": (2, 1, 20, 17), "strength": 1.0}, {"box": (2, 1, 20, 17), "strength": 1.0}, {"box": (2, 1, 20, 17), "strength": 1.0}]),
    ("extra_work_frames", (3, 3), (6, 9, 11, 4), 0, 0, 1.0,
     [{"box": (5, 7, 17, 8), "strength": 1.0}, {"box": (8, 8, 14, 13), "strength": 0.5}, {"box": (2, 2, 24, 20)}]),
)
# Opaque: name, originals, work, offset, feather, entries
OPAQUE = (
    ("step", (3, 3), (3, 9, 11, 3), 0, 0, [{"box": (3, 2, 23, 20)}, {"box": None}, {"box": (5, 7, 17, 8), "strength": 0.0}]),
    ("feathered_offset", (3, 4), (5, 30, 34, 4), 2, 6, [{"box": (0, 0, 26, 22)}, {"box": (4, 3, 15, 19)}, {"box": (7, 7, 7, 12)}]),
)


def _write_npz(path, arrays):
    import numpy as np
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0))
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def _load_classes(filename, names, namespace):
    """The named top-level classes of a reference file, taken out by AST and executed in `namespace` (oracle.reference_loader does the
    same for functions); nothing of the file is written anywhere."""
    from oracle import reference_loader as RL
    path = os.path.join(RL.REFERENCE_ROOT, filename)
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), namespace)
    return namespace


def child():
    import inspect

    import numpy as np
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import composite_support as CS
    from conftest import load_package
    from oracle import reference_loader as RL

    if torch.get_num_threads() < 2:
        torch.set_num_threads(2)
    load_package()
    from comfyui_vrgamedevgirl_amd import ops
    hm = CS.build_host_lib(tempfile.mkdtemp(prefix="composite_check"))
    paste_ref = RL._load_file("_vrgdg_reference_paste_back", "VRGDG_ImagePasteBack.py")
    ns = {"torch": torch, "F": F, "FACE_FIX_CONTEXT": "VRGDG_FACE_FIX_CONTEXT", "_log": lambda message: None,
          "_progress": lambda *a, **k: None}
    _load_classes("VRGDG_StandaloneFaceFixNodes.py", {"VRGDGFaceFixComposite", "VRGDGFaceFixCompositeOpaque"}, ns)
    with open(os.path.join(RL.REFERENCE_ROOT, "VRGDG_StandaloneFaceFixNodes.py"), "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read())
        context_type = next(ast.literal_eval(n.value) for n in tree.body
                            if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "FACE_FIX_CONTEXT")
        display_names = next(ast.literal_eval(n.value) for n in tree.body
                             if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "NODE_DISPLAY_NAME_MAPPINGS")
    ns["FACE_FIX_CONTEXT"] = context_type

    vendor_sqrt = torch.sqrt
    exact_sqrt = lambda x: torch.from_numpy(np.sqrt(x.detach().numpy()))        # noqa: E731 -- correctly rounded (checked below)
    probe = torch.rand(200000, generator=torch.Generator().manual_seed(1)) * 2
    assert np.array_equal(exact_sqrt(probe).numpy(), np.sqrt(probe.numpy().astype(np.float64)).astype(np.float32))
    tensor_mean = torch.Tensor.mean
    recorded = []

    def recording_mean(self, *a, **k):
        r = tensor_mean(self, *a, **k)
        recorded.append(r.detach().clone().numpy())
        return r

    def run(fn):
        """the reference call with the correctly rounded sqrt (means recorded), then with torch's own sqrt"""
        recorded.clear()
        torch.sqrt, torch.Tensor.mean = exact_sqrt, recording_mean
        try:
            res = fn()
        finally:
            torch.sqrt, torch.Tensor.mean = vendor_sqrt, tensor_mean
        return res, [m.copy() for m in recorded], fn()

    def originals_like(gen, shape):
        # dyadic values in [-0.1, 1.1]: the clamps act, and the archive stays small (the crops carry full mantissas)
        return (torch.randint(-102, 1127, shape, generator=gen).float() / 1024.0).contiguous()

    def noisy(gen, shape):
        return (torch.rand(shape, generator=gen) * 1.2 - 0.1).contiguous()

    flat, cases, problems = {}, [], []
    vendor = {"cases_with_a_different_mask": 0, "mask_elements_differing": 0, "largest_mask_difference_ulp1": 0.0}

    def record(case, make_inputs, call, means_order):
        seed = case["seed"]
        while True:
            gen = torch.Generator().manual_seed(seed)
            originals, crops, user_mask = make_inputs(gen)
            (out, mask), means, (_, vmask) = run(lambda: call(originals, crops, user_mask)[:2])
            key = case["key"]
            flat[key + ".originals"], flat[key + ".crops"] = originals.numpy(), crops.numpy()
            if user_mask is not None:
                flat[key + ".user_mask"] = user_mask.numpy()
            flat[key + ".out"], flat[key + ".mask"] = out.contiguous().numpy(), mask.contiguous().numpy()
            case["user_mask"] = user_mask is not None
            hc = CS.case_call(hm, ops, case, flat)
            case["rectangles"] = [[d.rule, d.flags, d.original_index, d.crop_index, d.mask_index, d.left, d.top, d.box_w, d.box_h, d.paste_w, d.paste_h]
                                  for d in list(hc.table)[:hc.frames]]
            fixture_selection = lambda f: (flat[key + ".mask"][f, hc.table[f].top:hc.table[f].top + hc.table[f].paste_h,       # noqa: E731
                                                               hc.table[f].left:hc.table[f].left + hc.table[f].paste_w] > np.float32(hc.table[f].threshold))
            rec = hc.truth_stats(fixture_selection)
            matched = [f for f in hc.match if rec[f, 1]]
            # rounding-tie guard on the fp64 means of the matched frames
            margin = 1.0
            for f in matched:
                d = hc.table[f]
                alpha, crop = hc.box(f)
                sel = fixture_selection(f)
                target = flat[key + ".originals"][d.original_index, d.top:d.top + d.paste_h, d.left:d.left + d.paste_w, :hc.nc]
                for values in (crop[..., :hc.nc][sel], target[sel]):
                    margin = min(margin, float(CS.tie_margin(values.astype(np.float64).mean(axis=0)).min()))
            if margin < 2.0 ** -40:
                seed += 1000
                continue
            break
        case["seed"], case["frames"], case["matched_frames"], case["match_channels"] = seed, hc.frames, matched, hc.nc
        case["selected"] = [int(rec[f, 0]) for f in range(hc.frames)]
        case["tie_margin_log2"] = float(np.log2(margin)) if matched else None
        if len(means) != 2 * len(matched):
            problems.append(f"{key}: the reference took {len(means)} means, {len(matched)} frames are matched here")
        else:
            ref = np.zeros((len(matched), 2, 4), dtype=np.float32)              # [matched frame][crop, original][channel]
            for k in range(len(matched)):
                a, b = means[2 * k], means[2 * k + 1]
                crop_mean, original_mean = (a, b) if means_order == "crop_first" else (b, a)
                ref[k, 0, :hc.nc], ref[k, 1, :hc.nc] = crop_mean, original_mean
            flat[key + ".ref_means"] = ref
        expected, expected_mask = hc.apply(rec)
        bad_mask = CS.mismatches(expected_mask, flat[key + ".mask"])
        if bad_mask:
            problems.append(f"{key}: host arithmetic mask differs from the reference in {bad_mask} elements")
        d_ref = CS.ulp_distance(flat[key + ".out"], expected)
        if not matched and d_ref:
            problems.append(f"{key}: no statistic takes part, yet the host arithmetic is {d_ref} ulp(1.0) from the reference")
        case["d_ref_ulp1"] = d_ref
        vdiff = int((vmask.contiguous().numpy() != flat[key + ".mask"]).sum())
        if vdiff:
            vendor["cases_with_a_different_mask"] += 1
            vendor["mask_elements_differing"] += vdiff
            vendor["largest_mask_difference_ulp1"] = max(vendor["largest_mask_difference_ulp1"], CS.ulp_distance(vmask.numpy(), flat[key + ".mask"]))
        cases.append(case)
        print(f"{key}: frames {hc.frames}, matched {matched}, selected {case['selected']}, d_ref {d_ref:.3f}, vendor-sqrt mask diffs {vdiff}, "
              f"mask mismatches {bad_mask}", flush=True)

    paste_node = paste_ref.VRGDG_ImagePasteBack()
    for i, (name, (n_o, ch), crop_shape, box, inset, feather, shape, cm, mask_shape) in enumerate(PASTE + (PASTE_WIDE,)):
        h, w = (WIDE_H, WIDE_W) if name == PASTE_WIDE[0] else (H, W)
        case = {"key": f"paste.{name}", "node": "paste", "seed": 100 + i, "crop_data": [[box[2] - box[0], box[3] - box[1]], list(box)],
                "inset_padding": inset, "feather_strength": feather, "blend_shape": shape, "color_match": cm}
        record(case,
               lambda gen: (originals_like(gen, (n_o, h, w, ch)), noisy(gen, crop_shape),
                            None if mask_shape is None else (torch.rand(mask_shape, generator=gen) * 1.6 - 0.3).contiguous()),
               lambda o, c, m: paste_node.paste_back(o, c, ((box[2] - box[0], box[3] - box[1]), box), inset, feather, shape, cm, mask=m),
               "crop_first")

    for cls_name, table, node_kind in (("VRGDGFaceFixComposite", FACEFIX, "facefix"), ("VRGDGFaceFixCompositeOpaque", OPAQUE, "opaque")):
        node = ns[cls_name]()
        for i, spec in enumerate(table):
            if node_kind == "facefix":
                name, (n_o, ch), work_shape, offset, feather, cm, entries = spec
            else:
                name, (n_o, ch), work_shape, offset, feather, entries = spec
                cm = None
            case = {"key": f"{node_kind}.{name}", "node": node_kind, "seed": 300 + i + (50 if node_kind == "opaque" else 0), "offset": offset,
                    "feather_pixels": feather, "entries": [dict(e, box=list(e["box"]) if e.get("box") else None) for e in entries]}
            if cm is not None:
                case["color_match"] = cm

            def call(o, c, m, node=node, entries=entries, offset=offset, feather=feather, cm=cm):
                ctx = {"original_frames": o, "entries": entries, "ltx_frame_offset": offset, "job_id": "golden"}
                res = node.composite(c, ctx, feather) if cm is None else node.composite(c, ctx, feather, cm)
                case["repaired"] = int(res[2])
                return res

            record(case, lambda gen, n_o=n_o, ch=ch, work_shape=work_shape: (originals_like(gen, (n_o, H, W, ch)), noisy(gen, work_shape), None),
                   call, "original_first")

    errors = []
    for node_kind, cls_name in (("facefix", "VRGDGFaceFixComposite"), ("opaque", "VRGDGFaceFixCompositeOpaque")):
        for n_entries, n_work in ((10, 2), (2, 10)):
            ctx = {"original_frames": torch.zeros(n_entries, 4, 4, 3), "entries": [{"box": None}] * n_entries}
            try:
                args = (torch.zeros(n_work, 4, 4, 3), ctx, 4) + ((0.5,) if node_kind == "facefix" else ())
                ns[cls_name]().composite(*args)
                raise SystemExit("the reference accepted a frame-count difference of 8")
            except ValueError as exc:
                errors.append({"node": node_kind, "entries": n_entries, "work_frames": n_work, "type": "ValueError", "text": str(exc)})
    for crop_data in (False, None, (1, 2, 3), ((4, 4), (5, 5, 5, 9)), ((4, 4), ("a", 1, 2, 3))):
        try:
            paste_node.paste_back(torch.zeros(1, 8, 8, 3), torch.zeros(1, 4, 4, 3), crop_data, 1, 1, "ellipse", 0.5)
            raise SystemExit(f"the reference accepted CROP_DATA {crop_data!r}")
        except ValueError as exc:
            errors.append({"node": "paste", "crop_data": crop_data, "type": "ValueError", "text": str(exc)})

    def surface(cls, function):
        s = {"INPUT_TYPES": cls.INPUT_TYPES(), "RETURN_TYPES": list(cls.RETURN_TYPES), "RETURN_NAMES": list(cls.RETURN_NAMES),
             "FUNCTION": cls.FUNCTION, "CATEGORY": cls.CATEGORY, "DESCRIPTION": cls.DESCRIPTION,
             "signature": list(inspect.signature(getattr(cls, function)).parameters)}
        if hasattr(cls, "RETURN_TOOLTIPS"):
            s["RETURN_TOOLTIPS"] = list(cls.RETURN_TOOLTIPS)
        return s

    meta = {"cases": cases, "errors": errors, "vendor_sqrt": vendor,
            "largest_d_ref_ulp1": max(c["d_ref_ulp1"] for c in cases),
            "surface": {
                "VRGDG_ImagePasteBack": dict(surface(paste_ref.VRGDG_ImagePasteBack, "paste_back"),
                                             display_name=paste_ref.NODE_DISPLAY_NAME_MAPPINGS["VRGDG_ImagePasteBack"]),
                "VRGDGFaceFixComposite": dict(surface(ns["VRGDGFaceFixComposite"], "composite"),
                                              display_name=display_names["VRGDGFaceFixComposite"]),
                "VRGDGFaceFixCompositeOpaque": dict(surface(ns["VRGDGFaceFixCompositeOpaque"], "composite"),
                                                    display_name=display_names["VRGDGFaceFixCompositeOpaque"]),
                "context_type": context_type,
                "helpers": {name: list(inspect.signature(getattr(paste_ref, name)).parameters)
                            for name in ("_batch_item", "_soft_blend_mask", "_match_color")}},
            "provenance": {"torch": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(),
                           "ATEN_CPU_CAPABILITY": os.environ.get("ATEN_CPU_CAPABILITY"), "threads": torch.get_num_threads(),
                           "sqrt": "correctly rounded (numpy), in place of torch's vendor-library sqrt",
                           "source": "VRGDG_ImagePasteBack.py and the two composite classes of VRGDG_StandaloneFaceFixNodes.py of the "
                                     "reference, their text unmodified, run on the CPU with torch.sqrt replaced as `sqrt` says"}}
    _write_npz(os.path.join(GOLDEN, "composite.npz"), flat)
    with open(os.path.join(GOLDEN, "composite.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print(f"composite.npz: {len(flat)} arrays, {os.path.getsize(os.path.join(GOLDEN, 'composite.npz'))} bytes; largest d_ref "
          f"{meta['largest_d_ref_ulp1']:.3f} ulp(1.0); vendor sqrt: {vendor}")
    if problems:
        raise SystemExit("\n".join(problems))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        env = dict(os.environ, ATEN_CPU_CAPABILITY="default")
        raise SystemExit(subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env).returncode)

"""The feathered crop composite without a GPU: csrc/vrg_composite_math.hpp compiled for the host against the recorded reference results
(tests/golden/composite.npz, made by tools/make_golden_composite.py), the descriptor tables of ops against the recorded rectangles, the
node surface, the refused inputs, and header / ctypes / library agreement for the new entry points."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import composite_support as CS
from conftest import PKG_DIR, ROOT

META = CS.meta()
CASES = META["cases"]
NEW_ENTRY_POINTS = ("vrg_composite_scratch_bytes", "vrg_composite_stats_f32", "vrg_composite_apply_f32")


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return CS.build_host_lib(tmp_path_factory.mktemp("composite_check"))


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def golden():
    return CS.arrays()


def fixture_selection(case, golden, call):
    def selection(f):
        d = call.table[f]
        return golden[case["key"] + ".mask"][f, d.top:d.top + d.paste_h, d.left:d.left + d.paste_w] > np.float32(d.threshold)
    return selection


def test_the_fixture_holds_the_cases_the_feature_was_specified_with():
    keys = {c["key"] for c in CASES}
    assert len(CASES) == 23 and {"paste.outside", "paste.cut_right", "paste.cut_bottom", "paste.few_selected", "paste.wide_masked",
                                 "facefix.tail_preserved", "facefix.extra_work_frames", "opaque.step"} <= keys
    assert any(c["matched_frames"] for c in CASES) and any(not c["matched_frames"] for c in CASES)
    assert os.path.getsize(os.path.join(CS.GOLDEN, "composite.npz")) <= os.path.getsize(os.path.join(CS.GOLDEN, "resize.npz"))


@pytest.mark.parametrize("case", CASES, ids=[c["key"] for c in CASES])
def test_descriptor_table_equals_the_recorded_rectangles(ops, golden, case):
    """A PIN, not an independent check: the recorded rectangles were written by ops.composite_table itself when the fixture was made, so
    this catches a change of the table.  That the table is what the reference computes is shown by the support of the reference's mask
    (below) and by the bit-equality of masks and images in test_host_arithmetic_against_the_fixture."""
    originals, crops = golden[case["key"] + ".originals"], golden[case["key"] + ".crops"]
    n_masks = golden[case["key"] + ".user_mask"].shape[0] if case["user_mask"] else 0
    entries, rule, color_match = CS.case_entries(ops, case, originals.shape[0], crops.shape[0], n_masks)
    table, match, _ = ops.composite_table(entries, rule, color_match, originals.shape[1], originals.shape[2])
    got = [[d.rule, d.flags, d.original_index, d.crop_index, d.mask_index, d.left, d.top, d.box_w, d.box_h, d.paste_w, d.paste_h]
           for d in list(table)[:len(entries)]]
    assert got == case["rectangles"] and len(entries) == case["frames"] == golden[case["key"] + ".out"].shape[0]
    assert set(case["matched_frames"]) <= set(match)
    # the rectangles as the reference computes them, from the recorded mask: its support lies inside the pasted region
    mask = golden[case["key"] + ".mask"]
    for f, d in enumerate(list(table)[:len(entries)]):
        outside = mask[f].copy()
        if d.rule:
            outside[d.top:d.top + d.paste_h, d.left:d.left + d.paste_w] = 0
        assert not outside.any()


@pytest.mark.parametrize("case", CASES, ids=[c["key"] for c in CASES])
def test_host_arithmetic_against_the_fixture(hm, ops, golden, case):
    """mask: bit-equal always.  image: bit-equal where no statistic takes part; where one does, the fp64 means over the fixture's own
    selection, rounded to fp32, give the expected image, and the reference's distance to it is what the fixture recorded (d_ref)."""
    call = CS.case_call(hm, ops, case, golden)
    rec = call.truth_stats(fixture_selection(case, golden, call))
    own = call.stats()                                         # the host arithmetic's own fp64 sums, raster order
    assert np.array_equal(own, rec)
    assert [int(v) for v in rec[:call.frames, 0]] == case["selected"]
    assert [f for f in call.match if rec[f, 1]] == case["matched_frames"]
    out, mask = call.apply(rec)
    assert CS.mismatches(mask, golden[case["key"] + ".mask"]) == 0
    d_ref = CS.ulp_distance(golden[case["key"] + ".out"], out)
    print(f"\n{case['key']}: d_ref = {d_ref} ulp(1.0) (recorded {case['d_ref_ulp1']})")
    assert d_ref == case["d_ref_ulp1"]
    if not case["matched_frames"]:
        assert CS.mismatches(out, golden[case["key"] + ".out"]) == 0
    else:
        # the reference's own fp32 means lie within a few fp32 roundings of the fp64 ones
        ref = golden[case["key"] + ".ref_means"]
        f32 = rec.view(np.float32)
        for k, f in enumerate(case["matched_frames"]):
            for which, lo in ((0, 2), (1, 6)):
                assert CS.ulp_distance(ref[k, which, :call.nc], f32[f, lo:lo + call.nc]) <= 8.0
        for f in case["matched_frames"]:
            d = call.table[f]
            _, crop = call.box(f)
            sel = fixture_selection(case, golden, call)(f)
            target = call.originals[d.original_index, d.top:d.top + d.paste_h, d.left:d.left + d.paste_w, :call.nc]
            for values in (crop[..., :call.nc][sel], target[sel]):
                assert CS.tie_margin(values.astype(np.float64).mean(axis=0)).min() >= 2.0 ** -40


_LINSPACE_CHILD = r"""
import sys, numpy as np, torch
sizes = [int(v) for v in sys.argv[2:]]
np.savez(sys.argv[1], capability=np.array(torch.backends.cpu.get_cpu_capability()),
         **{str(n): torch.linspace(-1, 1, n, dtype=torch.float32).numpy() for n in sizes})
"""


def test_cp_linspace_equals_torch_s_plain_kernel(hm, ops, tmp_path):
    """cp_linspace of the header (compiled for the host) against torch.linspace(-1, 1, n) run in a child process under
    ATEN_CPU_CAPABILITY=default, bit for bit, for small sizes and for those of 4K boxes."""
    sizes = list(range(1, 70)) + [127, 128, 255, 256, 511, 1000, 1023, 1024, 1025, 2047, 2160, 3840]
    env = dict(os.environ, ATEN_CPU_CAPABILITY="default")
    subprocess.run([sys.executable, "-c", _LINSPACE_CHILD, str(tmp_path / "linspace.npz")] + [str(n) for n in sizes], check=True, env=env, cwd=ROOT)
    want = np.load(tmp_path / "linspace.npz")
    assert str(want["capability"]) == "DEFAULT"
    for n in sizes:
        got = np.empty(n, dtype=np.float32)
        hm.hm_composite_linspace(n, ops._linspace_step(n), got)
        assert CS.mismatches(got, want[str(n)]) == 0, n


def test_node_surface_equals_the_reference(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_ImagePasteBack as PB
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes as FF
    surface = META["surface"]
    assert FF.FACE_FIX_CONTEXT == surface["context_type"]
    for module, name, function in ((PB, "VRGDG_ImagePasteBack", "paste_back"), (FF, "VRGDGFaceFixComposite", "composite"),
                                   (FF, "VRGDGFaceFixCompositeOpaque", "composite")):
        cls, want = getattr(module, name), surface[name]
        assert module.NODE_CLASS_MAPPINGS[name] is cls and module.NODE_DISPLAY_NAME_MAPPINGS[name] == want["display_name"]
        assert _plain(cls.INPUT_TYPES()) == want["INPUT_TYPES"]
        for attr in ("RETURN_TYPES", "RETURN_NAMES"):
            assert list(getattr(cls, attr)) == want[attr]
        for attr in ("FUNCTION", "CATEGORY", "DESCRIPTION"):
            assert getattr(cls, attr) == want[attr]
        assert list(getattr(cls, "RETURN_TOOLTIPS", [])) == want.get("RETURN_TOOLTIPS", [])
        assert list(inspect.signature(getattr(cls, function)).parameters) == want["signature"]
    for helper, params in surface["helpers"].items():
        assert list(inspect.signature(getattr(PB, helper)).parameters) == params
    # the modules carry their own mappings; the package mapping is untouched (tests/test_surface.py)
    assert not {"VRGDG_ImagePasteBack", "VRGDGFaceFixComposite", "VRGDGFaceFixCompositeOpaque"} & set(pkg.NODE_CLASS_MAPPINGS)


def _plain(value):
    if isinstance(value, dict):
        return {k: _plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    return value


def _tuples(value):
    return tuple(_tuples(v) for v in value) if isinstance(value, list) else value


def test_refused_and_invalid_inputs(pkg, ops, monkeypatch):
    from comfyui_vrgamedevgirl_amd import VRGDG_ImagePasteBack as PB
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes as FF
    monkeypatch.setattr(FF, "_log", lambda message: None)
    for e in META["errors"]:
        with pytest.raises(ValueError) as err:
            if e["node"] == "paste":
                crop_data = _tuples(e["crop_data"])          # JSON has no tuples; the message prints the box with repr()
                PB.VRGDG_ImagePasteBack().paste_back(torch.zeros(1, 8, 8, 3), torch.zeros(1, 4, 4, 3), crop_data, 1, 1, "ellipse", 0.5)
            else:
                ctx = {"original_frames": torch.zeros(e["entries"], 4, 4, 3), "entries": [{"box": None}] * e["entries"]}
                node = FF.VRGDGFaceFixComposite() if e["node"] == "facefix" else FF.VRGDGFaceFixCompositeOpaque()
                node.composite(*((torch.zeros(e["work_frames"], 4, 4, 3), ctx, 4) + ((0.5,) if e["node"] == "facefix" else ())))
        assert str(err.value) == e["text"]
    # what the reference mishandles is refused, and the message says so
    paste = PB.VRGDG_ImagePasteBack()
    for box in ((-2, 1, 4, 5), (1, -1, 4, 5)):
        with pytest.raises(ValueError, match="negative corner"):
            paste.paste_back(torch.zeros(1, 8, 8, 3), torch.zeros(1, 4, 4, 3), ((6, 4), box), 1, 1, "ellipse", 0.5)
    for o_c, c_c in ((2, 3), (3, 5), (5, 3), (3, 1)):
        with pytest.raises(ValueError, match="3 or 4 channels"):
            paste.paste_back(torch.zeros(1, 8, 8, o_c), torch.zeros(1, 4, 4, c_c), ((4, 4), (1, 1, 5, 5)), 1, 1, "ellipse", 0.5)
    for node, extra in ((FF.VRGDGFaceFixComposite(), (0.5,)), (FF.VRGDGFaceFixCompositeOpaque(), ())):
        for box in ((2, 2, 9, 6), (-1, 2, 5, 6), (2, 2, 6, 9)):
            ctx = {"original_frames": torch.zeros(1, 8, 8, 3), "entries": [{"box": box, "strength": 1.0}]}
            with pytest.raises(ValueError, match="does not lie inside"):
                node.composite(torch.zeros(1, 4, 4, 3), ctx, 4, *extra)
        ctx = {"original_frames": torch.zeros(1, 8, 8, 5), "entries": [{"box": (1, 1, 5, 5), "strength": 1.0}]}
        with pytest.raises(ValueError, match="3 or 4 channels"):
            node.composite(torch.zeros(1, 4, 4, 3), ctx, 4, *extra)
    with pytest.raises(ValueError, match="composite rule"):
        ops.composite_table([], ops.CompositeRule("triangle"), 0.0, 4, 4)


def test_a_no_face_entry_is_left_alone_whatever_its_box_says(ops):
    """The reference tests `not box or strength <= 0` before it looks at the box: a strength-0 entry (the no-face safety decision) with
    an empty or out-of-frame box is a frame returned unchanged, not a refused input.  With a positive strength the same boxes are refused."""
    rule = ops.CompositeRule("radial", feather=4)
    for box in ((5, 5, 5, 9), (6, 2, 3, 7), (-3, 1, 4, 6), (2, 2, 40, 6), (1, 1, 5, 40)):
        for entry in ({"box": box, "strength": 0.0}, {"box": box, "strength": -1.0}, {"box": box}):
            table, match, max_pixels = ops.composite_table([dict(entry, original=0, crop=0)], rule, 0.65, 8, 8)
            assert table[0].rule == 0 and table[0].flags == 0 and match == [] and max_pixels == 0
        with pytest.raises(ValueError, match="refused"):
            ops.composite_table([{"original": 0, "crop": 0, "box": box, "strength": 1.0}], rule, 0.65, 8, 8)
    rows = ops.face_fix_entries([{"box": (5, 5, 5, 9), "strength": 0.0}, {"box": (1, 1, 5, 5), "strength": 1.0}], 2, 0, 2)
    table, match, _ = ops.composite_table(rows, rule, 0.65, 8, 8)
    assert [table[0].rule, table[1].rule] == [0, ops.COMPOSITE_RULES["radial"]] and match == [1]


def test_face_fix_plan_and_log_lines(pkg, capsys):
    """offset / delta / usable as the reference derives them, and the node's log lines (part of its surface), without a GPU: the frame
    counts are refused before any pixel work"""
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes as FF
    for sources, work, offset, delta, usable in ((5, 6, 1, 0, 5), (6, 3, 0, 3, 3), (3, 6, 0, -3, 3), (4, 2, 5, 4, 0), (10, 2, 0, 8, 2), (2, 12, 2, -8, 2)):
        ctx = {"original_frames": torch.zeros(sources, 4, 4, 3), "entries": [{"box": None}] * sources, "ltx_frame_offset": offset or None}
        plan = FF._Plan(torch.zeros(work, 4, 4, 3), ctx)
        assert (plan.delta, plan.usable, plan.offset) == (delta, usable, offset)
    ctx = {"original_frames": torch.zeros(10, 4, 4, 3), "entries": [{"box": None}] * 10, "job_id": "job7"}
    with pytest.raises(ValueError, match="LTX returned 2 frames for 10 source frames."):
        FF.VRGDGFaceFixComposite().composite(torch.zeros(2, 4, 4, 3), ctx, 18, 0.65)
    assert capsys.readouterr().out == ("[VRGDG Face Fix] Composite started. Job=job7; source_frames=10, LTX_frames=2, delta=8, "
                                       "feather=18, color_match=0.65.\n")


def test_header_ctypes_and_library_agree_on_the_new_entry_points(pkg):
    from comfyui_vrgamedevgirl_amd import _hip
    with open(os.path.join(ROOT, "include", "vrgdg_hip.h")) as fh:
        header = fh.read()
    assert "#define VRG_ABI_VERSION 8" in header and _hip.ABI_VERSION == 8
    for name in NEW_ENTRY_POINTS:
        proto = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert proto, name
        params = [p.strip() for p in proto.group(2).split(",")]
        res, args = _hip._SIGNATURES[name]
        assert len(params) == len(args), (name, len(params), len(args))
        assert res is (C.c_int64 if proto.group(1) == "int64_t" else C.c_int)
        for p, a in zip(params, args):
            want = C.c_void_p if "*" in p else (C.c_int64 if p.startswith("int64_t") else C.c_int32)
            assert a is want, (name, p, a)
    # the descriptor struct: same fields, same order, same size as the C compiler lays it out
    body = re.search(r"typedef struct vrg_composite_desc \{(.*?)\} vrg_composite_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [n.strip().split("[")[0] for n in decl.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _hip.CompositeDesc._fields_]
    assert C.sizeof(_hip.CompositeDesc) == 80
    lib = os.path.join(PKG_DIR, "libvrgdg_hip.so")
    if os.path.exists(lib) and shutil.which("nm"):
        exported = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
        for name in NEW_ENTRY_POINTS:
            assert re.search(r"\bT " + name + r"\b", exported), name
        assert C.CDLL(lib).vrg_abi_version() == 8

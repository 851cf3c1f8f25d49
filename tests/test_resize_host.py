"""Frame resize / Video Enhance restore without a GPU: csrc/vrg_resize_math.hpp compiled for the host against the recorded results of
the reference's VRGDG_VideoEnhanceNodes.py (tests/golden/resize.npz: torch's CPU kernels in their plain form, ATEN_CPU_CAPABILITY=default),
the geometry helpers, the node surface and the C ABI of the two entry points.  No test here reads the reference checkout."""
import ctypes as C
import inspect
import os
import re
import shutil

import numpy as np
import pytest

import resize_support as RS
from conftest import ROOT

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return RS.build_host_lib(tmp_path_factory.mktemp("resize_check"))


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def ven(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_VideoEnhanceNodes
    return VRGDG_VideoEnhanceNodes


@pytest.fixture(scope="module")
def golden():
    return RS.arrays()


METHODS = ("Bicubic (recommended)", "Bilinear", "Area", "Nearest")


def test_fixture_was_made_by_the_plain_torch_kernels():
    prov = RS.META["provenance"]
    assert prov["ATEN_CPU_CAPABILITY"] == "default" and prov["cpu_capability"].upper() in ("DEFAULT", "NO AVX")
    assert len(RS.META["resize"]) == 4 * 3 * 4 + 4 and len(RS.META["restore_batch"]) == 2 * 3 * 4 and len(RS.META["restore"]) == 6
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "resize.npz")) < (1 << 20)


@needs_gxx
@pytest.mark.parametrize("method", METHODS)
def test_resize_batch_bit_equal_to_the_reference(hm, ops, golden, method):
    """(a) every _resize_batch case of the fixture -- 3 fit modes, up and down, odd sizes, a 1 x 1 source, RGBA in -- bit for bit"""
    cases = [c for c in RS.META["resize"] if c["resize_method"] == method]
    assert len(cases) == 13
    for c in cases:
        x = golden[c["in"]]
        g = ops.resize_geometry(x.shape[1], x.shape[2], c["target_width"], c["target_height"], c["fit_mode"])
        got = RS.host_resize(hm, ops, x, g, method)
        assert list(got.shape) == c["shape"], c
        bad = RS.mismatches(got, golden[c["key"]])
        assert bad == 0, (c, bad, float(np.abs(got - golden[c["key"]]).max()))


@needs_gxx
@pytest.mark.parametrize("method", METHODS)
def test_restore_batch_bit_equal_to_the_reference(hm, ops, golden, method):
    cases = [c for c in RS.META["restore_batch"] if c["resize_method"] == method]
    assert len(cases) == 6
    for c in cases:
        x = golden[c["in"]]
        g = ops.restore_geometry(x.shape[1], x.shape[2], c["source_width"], c["source_height"], c["fit_mode"])
        got = RS.host_resize(hm, ops, x, g, method)
        assert list(got.shape) == c["shape"], c
        assert RS.mismatches(got, golden[c["key"]]) == 0, c


@needs_gxx
def test_restore_blend_bit_equal_to_the_reference(hm, ops, golden):
    """the node's resize + blend + clamp: strength 0 / 0.35 / 0.5 / 1, RGBA originals, frame_count - work_frames in {-2, 0, 3}"""
    deltas = set()
    for c in RS.META["restore"]:
        work, originals = golden[c["key"] + ".work"], golden[c["key"] + ".originals"]
        deltas.add(c["frame_count"] - work.shape[0])
        g = ops.restore_geometry(work.shape[1], work.shape[2], originals.shape[2], originals.shape[1], c["fit_mode"])
        usable = min(c["frame_count"], work.shape[0])
        got = RS.host_restore(hm, ops, work, originals, g, c["resize_method"], c["strength"], usable)
        assert RS.mismatches(got, golden[c["key"] + ".out"]) == 0, c
    assert deltas == {-2, 0, 3}


def test_geometry_matches_the_recorded_shapes(ops):
    """(b) the rectangle integers for every fit mode: output shapes as recorded, rectangles consistent with them"""
    shapes = {"resize.0.in": (2, 7, 5, 4), "resize.1.in": (1, 1, 1, 3), "resize.2.in": (1, 18, 24, 3), "resize.3.in": (2, 30, 40, 4),
              "resize.4.in": (1, 34, 36, 3)}
    for c in RS.META["resize"]:
        s = shapes[c["in"]]
        g = ops.resize_geometry(s[1], s[2], c["target_width"], c["target_height"], c["fit_mode"])
        assert [s[0], g.out_h, g.out_w, 3] == c["shape"], c
        assert g.src == (0, 0, s[2], s[1])
        if c["fit_mode"] == ops.FIT_STRETCH:
            assert g.dst == (0, 0, c["target_width"], c["target_height"])
        elif c["fit_mode"] == ops.FIT_CROP:
            assert g.dst[0] <= 0 and g.dst[1] <= 0 and g.dst[0] + g.dst[2] >= g.out_w and g.dst[1] + g.dst[3] >= g.out_h
        else:
            assert g.dst[0] >= 0 and g.dst[1] >= 0 and g.dst[0] + g.dst[2] <= g.out_w and g.dst[1] + g.dst[3] <= g.out_h
    # 16:9 into 960 x 544 and back: the content rectangle of the letterbox is found again
    fwd = ops.resize_geometry(2160, 3840, 960, 544, ops.FIT_LETTERBOX)
    back = ops.restore_geometry(544, 960, 3840, 2160, ops.FIT_LETTERBOX)
    assert (fwd.out_h, fwd.out_w) == (544, 960) and fwd.dst == (0, 2, 960, 540) and back.src == fwd.dst
    assert back.dst == (0, 0, 3840, 2160) and (back.out_h, back.out_w) == (2160, 3840)
    assert ops.restore_geometry(544, 960, 3840, 2160, ops.FIT_CROP).src == (0, 0, 960, 544)
    # banker's rounding is inherited from Python: 5 * 0.5 = 2.5 -> 2
    assert ops.resize_geometry(5, 5, 2, 100, ops.FIT_LETTERBOX).dst[2:] == (2, 2)


def test_node_surface_equals_the_reference(ven, pkg):
    """(c) names, widget lists, defaults, tooltips, return conventions and signature order as recorded from the reference"""
    want = RS.META["surface"]
    cls = ven.VRGDGVideoEnhanceRestoreOriginal
    assert cls.__name__ == want["class"]
    got_inputs = cls.INPUT_TYPES()
    assert list(got_inputs) == list(want["INPUT_TYPES"]) and list(got_inputs["required"]) == list(want["INPUT_TYPES"]["required"])
    assert RS.json.loads(RS.json.dumps(got_inputs)) == want["INPUT_TYPES"]
    assert list(cls.RETURN_TYPES) == want["RETURN_TYPES"] and list(cls.RETURN_NAMES) == want["RETURN_NAMES"]
    assert (cls.FUNCTION, cls.CATEGORY, cls.DESCRIPTION) == (want["FUNCTION"], want["CATEGORY"], want["DESCRIPTION"])
    assert list(inspect.signature(cls.restore).parameters) == want["signature"]
    assert ven.VIDEO_ENHANCE_CONTEXT == want["context_type"]
    assert ven.NODE_CLASS_MAPPINGS == {"VRGDGVideoEnhanceRestoreOriginal": cls}
    assert ven.NODE_DISPLAY_NAME_MAPPINGS == {"VRGDGVideoEnhanceRestoreOriginal": want["display_name"]}
    for name, params in want["helpers"].items():
        assert list(inspect.signature(getattr(ven, name)).parameters) == params, name
    for mode, torch_mode in want["interpolation"].items():
        assert ven._interpolation(mode) == torch_mode
    for value, multiple, rounded in want["round_dimension"]:
        assert ven._round_dimension(value, multiple) == rounded
    # not registered in the package's mapping in this change (tests/golden/node_surface.json pins that key set)
    assert "VRGDGVideoEnhanceRestoreOriginal" not in pkg.NODE_CLASS_MAPPINGS


def test_node_errors_are_the_reference_s(ven):
    import torch
    node = ven.VRGDGVideoEnhanceRestoreOriginal()
    seen = 0
    for e in RS.META["errors"]:
        if "work_frames" in e:
            with pytest.raises(ValueError) as exc:
                node.restore(torch.zeros(e["work_frames"], 4, 4, 3), {"original_frames": torch.zeros(e["frame_count"], 4, 4, 3)},
                             "Bicubic (recommended)", 1.0)
        elif "shape" in e:
            with pytest.raises(ValueError) as exc:
                ven._resize_batch(torch.zeros(e["shape"]), 8, 8, "Stretch to dimensions", "Bicubic (recommended)")
        else:
            with pytest.raises(ValueError) as exc:
                node.restore(torch.zeros(1, 4, 4, 3), {"original_frames": None}, "Bicubic (recommended)", 1.0)
        assert str(exc.value) == e["text"]
        seen += 1
    assert seen == 5


def _prototype(name):
    header = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vrgdg_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_prototypes_match_the_ctypes_signatures(pkg):
    """(d) header <-> _hip for the two new symbols, argument by argument"""
    from comfyui_vrgamedevgirl_amd import _hip
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    for name in ("vrg_resize_f32", "vrg_restore_f32"):
        assert name in _hip.EXPORTED_SYMBOLS
        res, args = _hip._SIGNATURES[name]
        proto = _prototype(name)
        assert res is C.c_int and len(proto) == len(args), name
        for text, ctype in zip(proto, args):
            want = C.c_void_p if "*" in text else kinds[text.split()[0]]
            assert ctype is want, (name, text)
    assert [a.split()[-1] for a in _prototype("vrg_resize_f32")] == [
        "in", "out", "frames", "in_h", "in_w", "in_channels", "src_x0", "src_y0", "src_w", "src_h", "out_h", "out_w", "dst_x0", "dst_y0",
        "dst_w", "dst_h", "method", "stream"]
    assert _hip.ABI_VERSION == 8


def test_argument_validation_without_device(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    lib = _hip.load_library()
    null, one, two, three = C.c_void_p(0), C.c_void_p(16), C.c_void_p(32), C.c_void_p(48)
    ok = dict(in_h=8, in_w=8, in_c=3, src=(0, 0, 8, 8), out_h=16, out_w=16, dst=(0, 0, 16, 16))

    def resize(a=one, b=two, frames=1, method=0, **kw):
        g = dict(ok, **kw)
        return lib.vrg_resize_f32(a, b, frames, g["in_h"], g["in_w"], g["in_c"], *g["src"], g["out_h"], g["out_w"], *g["dst"], method, null)

    def restore(w=one, o=two, out=three, work_frames=1, frames=1, channels=3, method=0, **kw):
        g = dict(ok, **kw)
        return lib.vrg_restore_f32(w, o, out, work_frames, frames, g["in_h"], g["in_w"], g["in_c"], *g["src"], g["out_h"], g["out_w"], *g["dst"],
                                   channels, method, 0.5, 0.5, null)

    assert resize(frames=0) == 0 and restore(frames=0) == 0                       # zero frames: no launch
    assert resize(a=null) == 1 and resize(b=null) == 1 and resize(b=one) == 1     # null, in == out
    assert resize(method=4) == 1 and resize(method=-1) == 1 and resize(frames=-1) == 1
    assert resize(in_c=2) == 1 and resize(in_h=0) == 1 and resize(out_w=0) == 1
    assert resize(src=(1, 0, 8, 8)) == 1 and resize(src=(0, 0, 8, 9)) == 1 and resize(src=(-1, 0, 4, 4)) == 1 and resize(src=(0, 0, 0, 4)) == 1
    assert resize(dst=(16, 0, 4, 4)) == 1 and resize(dst=(-4, 0, 4, 4)) == 1 and resize(dst=(0, 0, 0, 4)) == 1
    assert resize(frames=0, dst=(-4, -2, 24, 20)) == 0 and resize(frames=0, dst=(2, 3, 8, 8)) == 0 and resize(frames=0, src=(2, 3, 6, 5)) == 0
    assert restore(w=null) == 1 and restore(o=null) == 1 and restore(out=null) == 1 and restore(out=two) == 1 and restore(out=one) == 1
    assert restore(channels=2) == 1 and restore(method=7) == 1 and restore(work_frames=-1) == 1 and restore(src=(0, 0, 9, 8)) == 1

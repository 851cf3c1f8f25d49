"""The landmark-aligned composite's warp without a GPU: csrc/vrg_warp_math.hpp compiled for the host (tests/host_math/warp_check.cpp)
against the independent numpy restatement and the float64 yardstick of tests/warp_support.py; truths that rest on nobody's memory of cv2
(identity, integer translations against np.pad(mode="reflect")); cv2 itself where a fixture or the package is at hand; the C ABI of the new
entry points and their refusals; the node's smoothing / reset bookkeeping against the transforms the reference handed to warpAffine
(tests/golden/landmark.json).  No test here reads the reference checkout."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import warp_support as WS
from conftest import ROOT

S = WS.similarity
# (source h, w), (result h, w), transform, kind of input: the geometries the limits of the yardstick were established on
CASES = (((40, 56), (40, 56), S(1, 0, 0, 0), "random"), ((40, 56), (40, 56), S(1.03, 4, 1.7, -2.2, (28, 20)), "random"),
         ((40, 56), (40, 56), S(0.6, 0, 3, 2, (28, 20)), "random"), ((40, 56), (40, 56), S(1.1, 33, 60, -45, (28, 20)), "random"),
         ((40, 56), (40, 56), S(0.6, -12, 2, 5, (28, 20)), "random"), ((64, 48), (64, 48), S(0.97, -7, -3.3, 4.1, (24, 32)), "smooth"),
         ((1, 1), (3, 4), S(1.2, 10, 0.5, 0.5), "random"), ((1, 9), (5, 9), S(0.9, 3, 0.25, 1), "random"), ((7, 1), (7, 3), S(1, 0, 0.5, 0), "random"),
         ((30, 30), (50, 70), S(2.0, 15, 5, 5), "smooth"), ((33, 47), (21, 29), S(1.0, 90, 30, 0), "random"), ((2, 2), (16, 16), S(1, 45, 8, 0), "random"),
         ((40, 56), (40, 56), np.zeros((2, 3), np.float32), "random"), ((25, 31), (25, 31), S(1.0, 0, 900.25, -1300.5), "smooth"))
IDS = [f"{k}-{c[0][0]}x{c[0][1]}-to-{c[1][0]}x{c[1][1]}-{c[3]}" for k, c in enumerate(CASES)]


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return WS.build_host_lib(tmp_path_factory.mktemp("warp_check"))


@pytest.fixture(scope="module")
def lib(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return _hip.load_library()


@pytest.mark.parametrize("src,dst,transform,kind", CASES, ids=IDS)
def test_host_header_equals_the_restatement(hm, src, dst, transform, kind):
    x = WS.frames_of(src, kind, 100 + src[0] + dst[1])
    keep = x.copy()
    want = WS.restated(x, transform, dst[1], dst[0])
    got = WS.host_warp(hm, x, transform, dst[1], dst[0])
    worst, share = WS.differences(got, want)
    print(f"{src} -> {dst} {kind}: largest difference {worst} levels, {share:.4%} of the bytes differ")
    assert np.array_equal(got, want) and np.array_equal(x, keep)


def test_phase_table(hm, pkg):
    """Every one of the 1024 kernels sums to exactly 32768; the library's table equals the header's and the restatement's.  Phase 0: the
    issue asks for a single 32768 at tap (3, 3), which an int16 table cannot hold -- its own rule saturate_cast<short>(1 * 1 * 32768)
    gives 32767 and the fix-up adds the missing 1 to tap (4, 4).  Asserted instead: exactly that split, and what a single 32768 would
    give -- phase 0 returns the centre byte for every pair of centre and (4, 4) bytes."""
    from comfyui_vrgamedevgirl_amd import ops
    table = ops.warp_phase_table()
    assert table.shape == (1024, 8, 8) and table.dtype == np.int16 and not table.flags.writeable
    assert set(table.astype(np.int64).reshape(1024, -1).sum(axis=1)) == {32768}
    header = np.zeros((1024, 8, 8), dtype=np.int16)
    hm.hm_warp_phase_table(header.reshape(-1))
    assert np.array_equal(table, header) and np.array_equal(table, WS.phase_table())
    zero = table[0].astype(np.int64)
    assert zero[3, 3] == 32767 and zero[4, 4] == 1 and np.count_nonzero(zero) == 2
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal((a * 32767 + b * 1 + (1 << 14)) >> 15, a)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (6, 1), (9, 13), (40, 56)])
def test_identity_returns_the_input(hm, shape):
    x = WS.frames_of(shape, "random", 3)
    ident = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32)
    assert np.array_equal(WS.host_warp(hm, x, ident, shape[1], shape[0]), x) and np.array_equal(WS.restated(x, ident, shape[1], shape[0]), x)


def test_integer_translations_equal_reflect_padding(hm):
    """warpAffine by (tx, ty) reads source pixel (x - tx, y - ty): the slice of np.pad(mode="reflect") -- numpy's reflect is REFLECT101"""
    h, w, pad = 11, 14, 9                                              # pad < min(h, w): one reflection, which np.pad does in one step
    x = WS.frames_of((h, w), "random", 4)
    padded = np.pad(x, ((pad, pad), (pad, pad), (0, 0)), mode="reflect")
    for ty in range(-pad, pad + 1):
        for tx in range(-pad, pad + 1):
            t = np.array([[1, 0, tx], [0, 1, ty]], dtype=np.float32)
            want = padded[pad - ty:pad - ty + h, pad - tx:pad - tx + w]
            assert np.array_equal(WS.host_warp(hm, x, t, w, h), want), (tx, ty)
    for tx, ty in ((-9, 9), (0, -7), (5, 0), (9, -9)):
        t = np.array([[1, 0, tx], [0, 1, ty]], dtype=np.float32)
        assert np.array_equal(WS.restated(x, t, w, h), padded[pad - ty:pad - ty + h, pad - tx:pad - tx + w])


@pytest.mark.parametrize("src,dst,transform,kind", CASES, ids=IDS)
def test_float64_yardstick(hm, src, dst, transform, kind):
    """the byte output is at most YARDSTICK_MAX_LEVELS from the float64 Lanczos-4 filter at the same quantised coordinates, on at most
    YARDSTICK_MAX_SHARE of the values (tests/warp_support.py says where the two constants come from)"""
    x = WS.frames_of(src, kind, 7)
    got = WS.host_warp(hm, x, transform, dst[1], dst[0])
    worst, share = WS.differences(got, WS.yardstick64(x, transform, dst[1], dst[0]))
    print(f"{src} -> {dst} {kind}: largest difference {worst} levels, {share:.4%} of the bytes differ")
    assert worst <= WS.YARDSTICK_MAX_LEVELS and share <= WS.YARDSTICK_MAX_SHARE


def test_warp_equals_cv2(hm):
    """the pin: cv2's own bytes, from the fixture if it was made, else from an importable cv2; neither is at hand everywhere"""
    if os.path.exists(WS.cv2_fixture_path()):
        data = np.load(WS.cv2_fixture_path())
        keys = json.loads(str(data["provenance"]))["cases"]
        cases = [(data[k + ".in"], data[k + ".transform"], data[k + ".out"]) for k in keys]
    else:
        cv2 = pytest.importorskip("cv2", reason="neither tests/golden/warp_lanczos4_cv2.npz nor the cv2 package (opencv-python) is available")
        cases = []
        for (h, w), (oh, ow), t, kind in CASES:
            x = WS.frames_of((h, w), kind, 31)
            cases.append((x, t, cv2.warpAffine(x, t, (ow, oh), flags=cv2.INTER_LANCZOS4, borderMode=cv2.BORDER_REFLECT101)))
    for x, t, want in cases:
        got = WS.host_warp(hm, x, t, want.shape[1], want.shape[0])
        worst, share = WS.differences(got, want)
        print(f"{x.shape} -> {want.shape}: largest difference {worst} levels, {share:.4%} of the bytes differ")
        assert np.array_equal(got, want)
        assert np.array_equal(WS.restated(x, t, want.shape[1], want.shape[0]), want)


def test_quantisation(hm):
    v = np.concatenate([np.linspace(-0.2, 1.2, 5001, dtype=np.float32), (np.arange(512, dtype=np.float32) + np.float32(0.5)) / np.float32(255.0),
                        np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, 0.5 / 255, 1.5 / 255, 2.5 / 255], dtype=np.float32)])
    got = np.zeros(v.size, dtype=np.uint8)
    hm.hm_warp_quantise(v, got, v.size)
    assert np.array_equal(got, WS.quantise(v))
    with np.errstate(invalid="ignore"):
        ref = (v[:-8] * 255).round().clip(0, 255).astype(np.uint8)               # the reference's own expression, where it is defined
    assert np.array_equal(got[:-8], ref) and got[-8] == 0


def _prototype(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vrgdg_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


NEW_SYMBOLS = ("vrg_warp_phase_table", "vrg_warp_record", "vrg_face_bytes_u8", "vrg_warp_affine_u8", "vrg_composite_warp_apply_f32")


def test_library_exports_the_symbols_and_the_abi_is_8(hm, lib):
    from comfyui_vrgamedevgirl_amd import _hip
    assert lib.vrg_abi_version() == 8 == _hip.ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read(), flags=re.S)
    assert "#define VRG_ABI_VERSION 8" in header
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    for name in NEW_SYMBOLS:
        assert name in _hip.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        proto = _prototype(header, name)
        res, args = _hip._SIGNATURES[name]
        assert res is C.c_int and len(proto) == len(args), name
        for text, ctype in zip(proto, args):
            assert ctype is (C.c_void_p if "*" in text else kinds[text.split()[0]]), (name, text)
    assert C.sizeof(_hip.WarpDesc) == 72 == hm.hm_warp_desc_bytes()
    assert C.sizeof(_hip.CompositeDesc) == 80                                   # untouched
    assert _hip.WARP_TABLE_BYTES == 1024 * 64 * 2
    fields = re.search(r"typedef struct vrg_warp_desc \{(.*?)\} vrg_warp_desc;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?[,;]", fields) == ["m", "src_offset", "src_w", "src_h", "set", "reserved"]
    assert [f[0] for f in _hip.WarpDesc._fields_] == ["m", "src_offset", "src_w", "src_h", "set", "reserved"]


def test_records_of_the_library_equal_the_header(hm, lib):
    from comfyui_vrgamedevgirl_amd import _hip
    for (h, w), (oh, ow), t, _ in CASES:
        a, b = _hip.WarpDesc(), _hip.WarpDesc()
        m = np.ascontiguousarray(t, dtype=np.float32).reshape(6)
        assert lib.vrg_warp_record(C.c_void_p(m.ctypes.data), ow, oh, w, h, 48, C.cast(C.byref(a), C.c_void_p)) == _hip.VRG_OK
        assert hm.hm_warp_record(m, ow, oh, w, h, 48, C.cast(C.byref(b), C.c_void_p)) == 1
        assert bytes(a) == bytes(b) and a.set == 1 and (a.src_w, a.src_h, a.src_offset) == (w, h, 48)
        assert list(a.m) == WS.inverted(t)                                      # the double inversion, bit for bit


def test_refusals_without_device(lib):
    from comfyui_vrgamedevgirl_amd import _hip
    null, a, b, t, r = C.c_void_p(0), C.c_void_p(64), C.c_void_p(128), C.c_void_p(256), C.c_void_p(512)
    OK, BAD = _hip.VRG_OK, _hip.VRG_ERR_BAD_ARG

    def warp(i=a, n=4096, o=b, rec=r, table=t, frames=1, oh=4, ow=4):
        return lib.vrg_warp_affine_u8(i, n, o, rec, table, frames, oh, ow, null)

    assert warp(frames=0) == OK                                                  # zero frames: no launch
    assert warp(i=null) == warp(o=null) == warp(rec=null) == warp(table=null) == BAD
    assert warp(o=a) == BAD and warp(frames=-1) == BAD and warp(n=-1) == BAD     # in == out, negative counts
    assert warp(oh=0) == warp(ow=0) == warp(oh=-3) == warp(ow=-3) == BAD
    assert warp(i=null, frames=0) == BAD and warp(table=C.c_void_p(260)) == BAD  # the table is read in 16-byte pieces

    def faces(c=a, o=null, d=r, offs=t, g=b, s=null, cap=4096, mp=16, frames=1, n_orig=1, n_crop=1, ch=8, cw=8, cc=3, H=16, W=16, Cc=3):
        return lib.vrg_face_bytes_u8(c, o, d, offs, g, s, cap, mp, frames, n_orig, n_crop, ch, cw, cc, H, W, Cc, null)

    assert faces(frames=0) == OK and faces(mp=0) == OK
    assert faces(c=null) == faces(d=null) == faces(offs=null) == faces(g=null) == BAD
    assert faces(s=a) == BAD                                                     # a source without originals
    assert faces(o=a, s=b) == BAD                                                # source == generated
    assert faces(frames=-1) == faces(cap=-1) == faces(mp=-1) == BAD
    for key in ("ch", "cw", "H", "W", "n_orig", "n_crop"):
        assert faces(**{key: 0}) == BAD and faces(**{key: -2}) == BAD
    assert faces(cc=2) == BAD and faces(Cc=5) == BAD

    def apply(c=a, o=b, d=r, st=t, rec=r, by=a, n=4096, table=t, out=C.c_void_p(1024), m=C.c_void_p(2048), frames=1, H=16, W=16):
        return lib.vrg_composite_warp_apply_f32(c, o, null, d, st, rec, by, n, table, out, m, frames, 1, 1, 0, 8, 8, 3, H, W, 3, 0, 0, 0, 3, null)

    assert apply(frames=0) == OK
    for key in ("c", "o", "d", "st", "rec", "by", "table", "out", "m"):
        assert apply(**{key: null}) == BAD, key
    assert apply(out=b) == BAD and apply(out=a) == BAD                           # out == originals / crops
    assert apply(frames=-1) == apply(n=-1) == apply(H=0) == apply(W=-4) == BAD
    assert lib.vrg_warp_phase_table(null) == BAD
    rec = _hip.WarpDesc()
    good = np.array([1, 0, 0, 0, 1, 0], dtype=np.float32)
    p = lambda m: C.c_void_p(m.ctypes.data)                                      # noqa: E731
    assert lib.vrg_warp_record(null, 4, 4, 4, 4, 0, C.cast(C.byref(rec), C.c_void_p)) == BAD
    assert lib.vrg_warp_record(p(good), 4, 4, 4, 4, 0, null) == BAD
    for w, h, sw, sh, off in ((0, 4, 4, 4, 0), (4, -1, 4, 4, 0), (4, 4, 0, 4, 0), (4, 4, 4, 0, 0), (4, 4, 4, 4, -1)):
        assert lib.vrg_warp_record(p(good), w, h, sw, sh, off, C.cast(C.byref(rec), C.c_void_p)) == BAD and rec.set == 0


REFUSED = ([[np.nan, 0, 0], [0, 1, 0]], [[1, 0, np.inf], [0, 1, 0]], [[1, 0, 0], [0, 1, -np.inf]],
           [[1, 0, 3.0e6], [0, 1, 0]],            # the shift times 1024 leaves int32
           [[1e-7, 0, 0], [0, 1e-7, 0]],          # the inverse scale times the last column times 1024 leaves int32
           [[1, 0, 0], [0, 1, -2.2e6]])
ACCEPTED = ([[1, 0, 2.0e6], [0, 1, -2.0e6]], [[0, 0, 0], [0, 0, 0]], [[1e-3, 0, 0], [0, 1e-3, 0]])


def test_python_surface(pkg):
    import torch
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes as FF
    from comfyui_vrgamedevgirl_amd import ops
    assert list(inspect.signature(ops.warp_phase_table).parameters) == []
    assert list(inspect.signature(ops.warp_records).parameters) == ["transforms", "boxes"]
    assert list(inspect.signature(ops.warp_affine_u8).parameters) == ["frames_u8", "transforms", "out_w", "out_h"]
    assert list(inspect.signature(ops.aligned_composite_frames).parameters) == [
        "originals", "crops", "entries", "feather", "transforms", "generated", "out", "mask_out"]
    assert list(inspect.signature(ops.face_bytes).parameters) == ["crops", "entries", "height", "width", "originals"]
    box = (2, 3, 402, 303)
    for t in REFUSED:
        assert WS.refused(t, 400, 300)
        with pytest.raises(ValueError):
            ops.warp_records([np.array(t, dtype=np.float32)], [box])
    for t in ACCEPTED:
        assert not WS.refused(t, 400, 300)
        table, offsets, total = ops.warp_records([t, None, t], [box, box, None])
        assert [table[i].set for i in range(3)] == [1, 0, 0] and offsets == [0, 400 * 300 * 3, -1] and total == 2 * 400 * 300 * 3
    with pytest.raises(ValueError):
        ops.warp_records([None], [box, box])
    with pytest.raises(ValueError):
        ops.warp_records([np.eye(3, dtype=np.float32)], [box])
    with pytest.raises(ValueError):
        ops.warp_affine_u8(torch.zeros(1, 4, 4, 3), [None], 4, 4)                 # fp32 frames are refused before any device work
    node = FF.VRGDGFaceFixCompositeLandmarkAligned
    assert node.estimator is None and node.FUNCTION == "composite" and node.CATEGORY == "VRGameDevGirl/Face Fix"
    assert node.RETURN_TYPES == ("IMAGE", "MASK", "INT") and node.RETURN_NAMES == FF.VRGDGFaceFixCompositeOpaque.RETURN_NAMES
    assert list(node.INPUT_TYPES()["required"]) == ["ltx_face_frames", "face_fix_context", "feather_pixels", "transform_smoothing"]
    assert node.INPUT_TYPES()["required"]["transform_smoothing"][1] == dict(node.INPUT_TYPES()["required"]["transform_smoothing"][1], default=0.75, min=0.0, max=0.95, step=0.05)
    assert list(inspect.signature(node.composite).parameters) == ["self", "ltx_face_frames", "face_fix_context", "feather_pixels", "transform_smoothing"]
    assert FF.LANDMARK_NODE_CLASS_MAPPINGS == {"VRGDGFaceFixCompositeLandmarkAligned": node}
    assert set(FF.LANDMARK_NODE_DISPLAY_NAME_MAPPINGS) == set(FF.LANDMARK_NODE_CLASS_MAPPINGS)
    assert "VRGDGFaceFixCompositeLandmarkAligned" not in pkg.NODE_CLASS_MAPPINGS
    with pytest.raises(ValueError, match="LTX returned 2 frames for 10 source frames."):
        node().composite(torch.zeros(2, 4, 4, 3), {"original_frames": torch.zeros(10, 4, 4, 3), "entries": [{"box": None}] * 10}, 6, 0.75)


CASES_GOLDEN = WS.meta()["cases"] if os.path.exists(os.path.join(WS.GOLDEN, "landmark.json")) else []


@pytest.mark.parametrize("case", CASES_GOLDEN, ids=[c["key"] for c in CASES_GOLDEN])
def test_transform_bookkeeping_equals_the_reference(pkg, case):
    """aligned_transforms (the node's host loop) fed the case's script gives, bit for bit, the float32 transforms the reference handed to
    warpAffine, on the same frames, and the same `aligned` count -- no GPU, no pixels"""
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes as FF
    entries = WS.case_entries(case)
    usable = min(len(entries), max(0, case["work_shape"][0] - case["offset"]))
    asked = []

    def estimate(index):
        asked.append(index)
        return case["script"][index] if case["detector"] else None

    got, aligned = FF.aligned_transforms(entries, usable, case["transform_smoothing"], estimate)
    assert asked == [i for i in range(usable) if FF._has_area(entries[i])]
    assert aligned == case["aligned"] and len(got) == usable
    for i, want in enumerate(case["applied"][:usable]):
        if want is None:
            assert got[i] is None, i
        else:
            assert got[i].dtype == np.float32 and got[i].shape == (2, 3)
            assert got[i].tobytes() == np.array(want, dtype=np.float32).tobytes(), i
    assert all(a is None for a in case["applied"][usable:])


def test_fixture_covers_what_the_issue_lists():
    cases = {c["key"]: c for c in CASES_GOLDEN}
    assert len(cases) >= 14 and not cases["no_detector"]["detector"] and cases["no_detector"]["aligned"] == 0
    assert {c["transform_smoothing"] for c in cases.values()} >= {0.0, 0.75} and cases["smoothing_095_clamped_from_2"]["log"].endswith("smoothing=0.95.")
    assert cases["offset_7"]["offset"] == 7 and cases["short_ltx_tail"]["work_shape"][0] < cases["short_ltx_tail"]["originals_shape"][0]
    assert cases["leading_miss"]["applied"][:2] == [None, None] and cases["leading_miss"]["aligned"] == 3
    assert any(e.get("hard_cut") for e in cases["resets"]["entries"]) and len({e["shot_id"] for e in cases["resets"]["entries"]}) > 1
    assert cases["resets"]["applied"][2] is None and cases["resets"]["applied"][4] is None          # a miss right after each reset: no transform
    assert cases["rgba_originals_rgba_work"]["originals_shape"][3] == 4 and cases["feather_0"]["feather_pixels"] == 0
    assert cases["far_outside_rotation_and_shift"]["reflections_at_most"] >= 3

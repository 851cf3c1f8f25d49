"""The landmark estimator's input without a GPU: csrc/vrg_thumbs_math.hpp over csrc/vrg_grid_math.hpp compiled for the host
(tests/host_math/thumbs_check.cpp) against the independent numpy restatement of cv2's INTER_AREA (tests/grid_support.py) with the channels
flipped, byte for byte, and against the float64 filters; the refusals of the two new entry points; `landmark_points` and the restatement's
thumbnails against the reference's own `_landmarks` as recorded in tests/golden/landmark_input.json / .npz; the node's surface; cv2 itself
where a fixture or the package is at hand.  No test here reads the reference checkout."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import grid_support as G
import landmark_input_support as L
from conftest import PKG_DIR, ROOT

SWEEP = [(box, mode, kind) for box, mode, _ in L.GEOMETRIES for kind in L.KINDS] + [(box, mode, "uniform") for box, mode, _ in L.SEGMENTED]
IDS = [f"{h}x{w}-{kind}" for (h, w), _, kind in SWEEP]


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return L.build_host_lib(tmp_path_factory.mktemp("thumbs_check"))


@pytest.fixture(scope="module")
def FF(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes
    return VRGDG_StandaloneFaceFixNodes


@pytest.fixture(scope="module")
def hip(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return _hip


@functools.lru_cache(maxsize=None)
def box_and_restatement(h, w, kind):
    """computed once, shared by the tests below, never written"""
    u8 = L.make_box(kind, h, w, 7)
    want = L.restated(u8)
    u8.setflags(write=False)
    want.setflags(write=False)
    return u8, want


@pytest.mark.parametrize("box,mode,kind", SWEEP, ids=IDS)
def test_host_header_equals_the_restatement(hm, box, mode, kind):
    h, w = box
    assert G.mode_of(h, w, L.SIDE, L.SIDE) == mode == L.host_plan(hm, h, w)[0]
    u8, want = box_and_restatement(h, w, kind)
    keep = u8.copy()
    got = L.host_thumb(hm, u8)
    worst, share = G.differences(got, want)
    print(f"{h} x {w} {L.mode_name(mode)} {kind}: largest difference {worst} levels, {share:.4%} of the bytes differ")
    assert np.array_equal(got, want) and np.array_equal(u8, keep)
    assert np.array_equal(got[..., ::-1], G.resize_area(u8, L.SIDE, L.SIDE))                       # channel c is channel 2 - c of the resize


def test_every_rule_occurs():
    assert {mode for _, mode, _ in L.GEOMETRIES} == {G.COPY, G.FAST, G.FAST_2X2, G.GENERAL, G.LINEAR}
    assert {G.mode_of(h, w, L.SIDE, L.SIDE) for (h, w), _, node in L.GEOMETRIES if node} == {G.COPY, G.FAST, G.FAST_2X2, G.GENERAL, G.LINEAR}


@pytest.mark.parametrize("box,mode,kind", SWEEP, ids=IDS)
def test_float64_yardstick(box, mode, kind):
    """one final rounding: at most 1 level from the exact float64 area average (area rules) or from float64 bilinear at the same s, f (linear
    rule), everywhere.  The share of differing bytes is capped at 1.5 x grid_support's AREA_WORST_SHARE / LINEAR_WORST_SHARE, except at the
    two geometries whose restatement alone passes that cap (landmark_input_support.SHARE_EXEMPT; DESIGN.md section 4 has the measured table:
    319 x 319 12.7 .. 12.9 %, 200 x 400 up to 6.84 % against a cap of 6.68 %); the header's bytes are the restatement's (the test above)"""
    h, w = box
    u8, want = box_and_restatement(h, w, kind)
    worst, share = G.differences(want, L.yardstick(u8))
    cap = L.share_cap(mode)
    print(f"{h} x {w} {L.mode_name(mode)} {kind}: largest difference {worst} levels, {share:.4%} of the bytes differ (cap {cap:.4%})")
    assert worst <= G.YARDSTICK_MAX_LEVELS
    if box not in L.SHARE_EXEMPT:
        assert share <= cap


def test_plan_is_the_grid_plan(hm, hip, pkg):
    from comfyui_vrgamedevgirl_amd import ops
    lib = hip.load_library()
    for (h, w), mode, _ in L.GEOMETRIES + (((32767, 32767), G.GENERAL, False), ((1, 32767), G.LINEAR, False)):
        m, cps, inv = C.c_int32(), C.c_int32(), C.c_float()
        assert lib.vrg_grid_plan(h, w, 3, L.SIDE, L.SIDE, C.byref(m), C.byref(cps), C.byref(inv)) == hip.VRG_OK
        assert (m.value, cps.value, inv.value) == L.host_plan(hm, h, w) == ops.thumb_plan(h, w) and m.value == mode and 1 <= cps.value <= 64
    assert L.host_plan(hm, 2160, 2160)[1] == 64 and L.host_plan(hm, 960, 1280) == (G.FAST, 64, np.float32(1.0) / np.float32(12.0))
    assert all(L.host_plan(hm, h, w)[0] == mode and L.host_plan(hm, h, w)[1] < 64 for (h, w), mode, _ in L.SEGMENTED)
    assert hm.hm_thumb_desc_bytes() == C.sizeof(hip.ThumbDesc) == C.sizeof(L.ThumbDesc) == ops.THUMB_DESC.itemsize == 48
    header = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    fields = header[header.index("typedef struct vrg_thumb_desc"):header.index("} vrg_thumb_desc;")]
    for (name, _), (other, _) in zip(hip.ThumbDesc._fields_, L.ThumbDesc._fields_):
        assert name == other and name in fields and name in ops.THUMB_DESC.names


def good_descriptor(ops, h=333, w=517, which=0, offset=5):
    desc, tables, fix = ops.thumb_descriptors([(which, offset, w, h)])
    assert len(tables) == (1 if h == w else 2) * L.SIDE * 20 and [f for _, f, _ in fix] == ["xtab", "ytab"]      # one table per distinct (n_in, mode)
    desc["xtab"], desc["ytab"] = 4096, 8192                                    # never dereferenced on the host
    return desc


def test_check_refuses_without_device(hip, pkg):
    from comfyui_vrgamedevgirl_amd import ops
    lib = hip.load_library()
    d = good_descriptor(ops)
    n_bytes = 5 + 333 * 517 * 3
    check = lambda n=n_bytes, has_source=0: lib.vrg_face_thumbs_check(C.c_void_p(d.ctypes.data), 1, n, has_source)
    assert check() == hip.VRG_OK == check(has_source=1)
    assert lib.vrg_face_thumbs_check(None, 0, 0, 0) == hip.VRG_OK and lib.vrg_face_thumbs_check(None, 1, n_bytes, 0) == hip.VRG_ERR_BAD_ARG
    assert lib.vrg_face_thumbs_check(C.c_void_p(d.ctypes.data), -1, n_bytes, 0) == check(n=-1) == hip.VRG_ERR_BAD_ARG
    assert check(n=n_bytes - 1) == hip.VRG_ERR_BAD_ARG                         # the image does not end inside n_bytes
    plan_2x2 = ops.thumb_plan(2, 2)
    for field, value in (("box_w", 0), ("box_h", 0), ("box_w", 32768), ("box_h", 32768), ("box_w", -517), ("which", 2), ("which", -1), ("offset", -1),
                         ("offset", 6), ("mode", hip.GRID_LINEAR), ("mode", 7), ("cps", 0), ("cps", 32), ("inv", 0.5), ("xtab", 0), ("ytab", 0)):
        keep = d[field][0]
        d[field] = value
        assert check() == hip.VRG_ERR_BAD_ARG, (field, value)
        d[field] = keep
    assert check() == hip.VRG_OK
    d["which"] = 1
    assert check() == hip.VRG_ERR_BAD_ARG and check(has_source=1) == hip.VRG_OK                    # which == 1 wants a source buffer
    # the fast rules carry inv = 1 / (sx * sy); another one is refused
    f = good_descriptor(ops, 960, 1280, offset=0)
    big = 960 * 1280 * 3
    assert f["mode"][0] == hip.GRID_FAST and lib.vrg_face_thumbs_check(C.c_void_p(f.ctypes.data), 1, big, 0) == hip.VRG_OK
    f["inv"] = 1.0
    assert lib.vrg_face_thumbs_check(C.c_void_p(f.ctypes.data), 1, big, 0) == hip.VRG_ERR_BAD_ARG
    # the smallest and the largest sides pass
    for h, w in ((1, 1), (2, 2), (1, 32767)):
        e = good_descriptor(ops, h, w, offset=3)
        assert lib.vrg_face_thumbs_check(C.c_void_p(e.ctypes.data), 1, 3 + h * w * 3, 0) == hip.VRG_OK
    assert plan_2x2[0] == hip.GRID_LINEAR


def test_entry_point_refuses_without_device(hip, pkg):
    lib = hip.load_library()
    null, gen, src, desc, out = C.c_void_p(0), C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(64), C.c_void_p(1 << 24)
    entry = lib.vrg_face_thumbs_u8
    assert entry(gen, src, 1000, desc, 0, out, null) == hip.VRG_OK == entry(null, null, 0, null, 0, null, null)        # nothing to do: no launch
    assert entry(gen, src, 1000, desc, 1, null, null) == hip.VRG_ERR_BAD_ARG                                            # null out
    assert entry(gen, src, 1000, desc, 1, C.c_void_p((1 << 24) + 8), null) == hip.VRG_ERR_BAD_ARG                       # misaligned out
    assert entry(gen, src, 1000, desc, 1, gen, null) == entry(gen, src, 1000, desc, 1, src, null) == hip.VRG_ERR_BAD_ARG            # out is an input
    assert entry(gen, null, 1000, desc, 1, gen, null) == hip.VRG_ERR_BAD_ARG
    assert entry(gen, src, 1 << 20, desc, 1, C.c_void_p(4096 + 1024), null) == hip.VRG_ERR_BAD_ARG                      # out inside an input
    assert entry(null, src, 1000, desc, 1, out, null) == entry(gen, src, 1000, null, 1, out, null) == hip.VRG_ERR_BAD_ARG
    assert entry(gen, src, 1000, C.c_void_p(68), 1, out, null) == hip.VRG_ERR_BAD_ARG                                   # misaligned records
    assert entry(gen, src, -1, desc, 1, out, null) == entry(gen, src, 1000, desc, -1, out, null) == hip.VRG_ERR_BAD_ARG


def test_library_exports_the_symbols_and_the_abi_is_8(hip, pkg):
    from comfyui_vrgamedevgirl_amd import build_ext
    lib = hip.load_library()
    assert lib.vrg_abi_version() == 8 == hip.ABI_VERSION
    for name in ("vrg_face_thumbs_check", "vrg_face_thumbs_u8"):
        assert name in hip.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert "vrg_thumbs_math.hpp" in build_ext.HEADERS and "vrg_thumbs.hip" in build_ext.SOURCES


def test_golden_cases_pin_the_route_of_the_reference(FF):
    """what the reference's `_landmarks` showed its detector and returned (tools/make_golden_landmark_input.py), against the restatement's
    thumbnails and landmark_points: digests and float32 bits"""
    meta, points = L.golden()
    cases = meta["cases"]
    assert len(cases) >= 12
    modes, tied, several = set(), 0, 0
    for case in cases:
        h, w = case["box"]
        image = L.case_image(case)
        if h < 2 or w < 2:
            assert case["shown"] == [] and not case["points"] and case["key"] not in points.files
            continue
        thumb = L.restated(image)
        assert case["shown"] == [L.sha(thumb)], case["key"]
        modes.add(G.mode_of(h, w, L.SIDE, L.SIDE))
        rows = L.recorded_detector(thumb)
        got = FF.landmark_points(rows, w, h)
        if not case["points"]:
            assert rows is None and got is None and case["key"] not in points.files
            continue
        several += len(rows) > 1
        tied += len(rows) > 1 and float(rows[0][-1]) == float(rows[1][-1])
        want = points[case["key"]]
        assert got.dtype == np.float32 and got.shape == (5, 2) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), case["key"]
    assert modes == {G.COPY, G.FAST, G.FAST_2X2, G.GENERAL, G.LINEAR}
    assert any(not c["points"] and c["shown"] for c in cases) and any(not c["shown"] for c in cases)      # no face; a box below 2 x 2
    assert several >= 2 and tied >= 1                                                                    # the best row, the first on ties


def test_landmark_points(FF):
    rows = np.zeros((3, 15), dtype=np.float32)
    rows[:, 4:14] = np.arange(30, dtype=np.float32).reshape(3, 10) + np.float32(0.3)
    rows[:, -1] = (0.5, 0.9, 0.9)
    got = FF.landmark_points(rows, 517, 333)
    want = rows[1, 4:14].reshape(5, 2).copy()
    want[:, 0] *= np.float32(517.0 / 320.0)
    want[:, 1] *= np.float32(333.0 / 320.0)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))           # the first of the tied rows
    assert FF.landmark_points(None, 10, 10) is None and FF.landmark_points(np.zeros((0, 15), dtype=np.float32), 10, 10) is None
    assert FF.landmark_points([], 10, 10) is None
    got[0, 0] = 0                                                                                          # a copy: the rows stay
    assert rows[1, 4] == np.float32(10.3)


def test_surface(FF, pkg):
    node = FF.VRGDGFaceFixCompositeLandmarkAligned
    assert node.estimator is None and node.landmark_detector is None and node.transform_fit is None
    try:
        import cv2  # noqa: F401
        have_cv2 = True
    except Exception:
        have_cv2 = False
    model = os.path.join(PKG_DIR, "assets", "face_detection_yunet_2023mar.onnx")
    if not have_cv2 or not os.path.isfile(model):
        assert FF.cv2_landmark_seams() is None
    assert not os.path.isfile(model)                                                                      # the model file is not shipped
    assert FF.NODE_CLASS_MAPPINGS == {"VRGDGFaceFixComposite": FF.VRGDGFaceFixComposite, "VRGDGFaceFixCompositeOpaque": FF.VRGDGFaceFixCompositeOpaque}
    assert FF.LANDMARK_NODE_CLASS_MAPPINGS == {"VRGDGFaceFixCompositeLandmarkAligned": node}
    assert FF.LANDMARK_NODE_DISPLAY_NAME_MAPPINGS == {"VRGDGFaceFixCompositeLandmarkAligned": "Face Fix - Composite Landmark Aligned"}
    assert "VRGDGFaceFixCompositeLandmarkAligned" not in pkg.NODE_CLASS_MAPPINGS


def test_fit_stand_in_recovers_a_similarity():
    """the numpy stand-in for estimateAffinePartial2D that the GPU test hands the node: exact on points that are a similarity apart"""
    rng = np.random.Generator(np.random.PCG64(3))
    g = rng.uniform(0, 300, (5, 2))
    m = np.array([[0.9, -0.2, 4.0], [0.2, 0.9, -7.0]])
    s = g @ m[:, :2].T + m[:, 2]
    assert np.allclose(L.similarity_fit(g.astype(np.float32), s.astype(np.float32)), m, atol=1e-4)
    rows = L.steady_detector(np.full((L.SIDE, L.SIDE, 3), 90, dtype=np.uint8))
    assert rows.shape == (2, 15) and rows[1, -1] > rows[0, -1] and len(L.steady_detector(np.zeros((L.SIDE, L.SIDE, 3), dtype=np.uint8))) == 0


def test_check_program_under_the_sanitizers(tmp_path):
    """the check program as a stand-alone executable with the address and undefined-behaviour sanitizers: every rule once"""
    exe = str(tmp_path / "thumbs_check")
    cmd = ["g++", *G.HOST_FLAGS, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DTHUMBS_CHECK_MAIN",
           "-I", os.path.join(PKG_DIR, "csrc"), L.host_source(), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr + built.stdout and ("cannot find" in built.stderr or "unrecognized" in built.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("thumbs_check:"), run.stderr


def test_thumbs_equal_cv2(hm):
    """the pin: cv2's own resize and flip, from the fixture if it was made, else from an importable cv2; neither is at hand everywhere"""
    inputs = L.cv2_pin_inputs()
    if os.path.exists(L.cv2_fixture_path()):
        data = np.load(L.cv2_fixture_path())
        cases = [(u8, data[key]) for key, u8 in inputs]
    else:
        cv2 = pytest.importorskip("cv2", reason="neither tests/golden/landmark_input_cv2.npz nor the cv2 package (opencv-python) is available")
        cases = [(u8, cv2.cvtColor(cv2.resize(u8, (L.SIDE, L.SIDE), interpolation=cv2.INTER_AREA), cv2.COLOR_RGB2BGR)) for _, u8 in inputs]
    assert {G.mode_of(u8.shape[0], u8.shape[1], L.SIDE, L.SIDE) for u8, _ in cases} == {G.COPY, G.FAST, G.FAST_2X2, G.GENERAL, G.LINEAR}
    for u8, want in cases:
        got = L.restated(u8)
        worst, share = G.differences(got, want)
        print(f"{u8.shape}: largest difference {worst} levels, {share:.4%} of the bytes differ")
        assert np.array_equal(got, want) and np.array_equal(L.host_thumb(hm, u8), want)

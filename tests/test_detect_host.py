"""The detector-input arithmetic of csrc/vrg_detect_math.hpp without a GPU: the header compiled for the host equals the independent numpy
restatement of tests/detect_support.py byte for byte (warp, resize, taps, the fused blob) on the geometries of the issue; properties that
rest on nobody's memory of cv2; float64 yardsticks; the ABI; and detection_plan / candidates_from_outputs of both modules against the
reference's recorded route (tests/golden/detect_prep.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import detect_support as D


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return D.build_host_lib(tmp_path_factory.mktemp("detect_host"))


@pytest.fixture(scope="module")
def hip(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return _hip


@pytest.fixture(scope="module")
def FF(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes
    return VRGDG_StandaloneFaceFixNodes


@pytest.fixture(scope="module")
def BF(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix
    return VRGDG_FaceFix


@pytest.fixture(scope="module")
def golden():
    with open(D.golden_path()) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def restated():
    """key -> (frames, blobs [1, A, R, 3, 300, 300], rotated [1, A, H, W, 3]) of frame 0, computed once"""
    out = {}
    for key, (_, _, mode, regions) in D.CASES.items():
        x = D.case_frames(key)[:1]
        out[key] = (x,) + D.restated_blobs(x, mode, regions)
    return out


def plan_of(FF, BF, key):
    shape, _, mode, regions = D.CASES[key]
    if regions is not None:
        return BF.detection_plan(shape[2], shape[1], mode, regions)
    return FF.detection_plan(shape[2], shape[1], mode)


@pytest.mark.parametrize("key", sorted(D.CASES))
def test_header_equals_the_restatement(lib, FF, BF, restated, key):
    x, blobs, rotated = restated[key]
    plan = plan_of(FF, BF, key)
    bgr = D.as_bgr(x)[0]
    if x.dtype != np.uint8:
        assert np.array_equal(D.host_quantise(lib, x[0]), bgr)
    seen = set()
    for a, angle in enumerate(plan.angles):
        if angle:
            assert np.array_equal(plan.inverse[a], D.rotation(plan.width, plan.height, angle)[1])
            assert np.array_equal(plan.forward[a], D.rotation(plan.width, plan.height, angle)[0])
            warped = D.host_warp(lib, bgr, plan.inverse[a])
            worst, share = D.differences(warped, rotated[0, a])
            print(f"{key} {angle:+d}: warp: largest difference {worst} levels, {share:.4%} of the bytes differ")
            assert worst == 0
        for r in range(plan.slots):
            got, ok = D.host_blob(lib, x, plan.transforms, (0, plan.transform_index[a]) + tuple(plan.regions[a][r]) if r < len(plan.regions[a]) else (0, -1, 0, 0, 0, 0))
            assert ok == plan.scanned[a][r]
            assert np.array_equal(got, blobs[0, a, r]), (key, angle, r)
            if ok and angle == 0:
                left, top, right, bottom = plan.regions[a][r]
                if (bottom - top, right - left) not in seen:
                    seen.add((bottom - top, right - left))
                    assert np.array_equal(D.host_resize(lib, bgr[top:bottom, left:right]), D.resize_linear(bgr[top:bottom, left:right]))


@pytest.mark.parametrize("kind", ("smooth", "special"))
def test_header_equals_the_restatement_on_other_frames(lib, FF, kind):
    x = D.make_frames(kind, (1, 61, 97, 4), "f32", 31)
    want, _ = D.restated_blobs(x, "Strong: ±15° and ±30°")
    plan = FF.detection_plan(97, 61, "Strong: ±15° and ±30°")
    for a in range(5):
        got, ok = D.host_blob(lib, x, plan.transforms, (0, plan.transform_index[a], 0, 0, 97, 61))
        assert ok and np.array_equal(got, want[0, a, 0])
    if kind == "special":
        assert np.isnan(x).any() and np.isinf(x).any()


@pytest.mark.parametrize("n_in", (8, 61, 97, 294, 299, 300, 301, 384, 420, 600, 640, 2160, 3840, 32767))
def test_taps(lib, pkg, hip, n_in):
    from comfyui_vrgamedevgirl_amd import ops
    ofs, coef = D.host_taps(lib, n_in)
    table = ops.linear_taps(n_in)
    for axis, (name, horizontal) in enumerate((("h", True), ("v", False))):
        s, _, c0, c1 = D.axis_taps(n_in, 300, horizontal)
        assert np.array_equal(ofs[axis * 300:(axis + 1) * 300], s) and np.array_equal(coef[axis, :, 0], c0) and np.array_equal(coef[axis, :, 1], c1)
        assert np.array_equal(table[name + "_ofs"], s) and np.array_equal(table[name + "_coef"], np.stack([c0, c1], axis=1))
        assert (c0 + c1 == 2048).all()
    assert table["h_ofs"].min() >= 0 and table["h_ofs"].max() <= n_in - 1
    assert table["v_ofs"].min() >= -1 and table["v_ofs"].max() <= n_in - 1


def test_header_matrices_equal_the_plan(lib, FF):
    """dt_rotation / dt_invert of the header (cosine and sine from this libm) against the restatement and detection_plan"""
    import math
    for width, height in ((640, 420), (97, 61), (3840, 2160), (601, 33)):
        for angle in (-30, -15, 15, 30, 7, 90):
            forward, inverse = np.zeros((2, 3)), np.zeros((2, 3))
            radians = angle * math.pi / 180.0
            lib.hm_detect_rotation(math.cos(radians), math.sin(radians), width, height, forward.ctypes.data, inverse.ctypes.data)
            want = D.rotation(width, height, angle)
            assert np.array_equal(forward, want[0]) and np.array_equal(inverse, want[1]), (width, height, angle)
            mine = FF.rotation_matrices(width, height, angle)
            assert np.array_equal(forward, mine[0]) and np.array_equal(inverse, mine[1])


def test_identity_and_integer_translations(lib):
    bgr = D.as_bgr(D.uniform_frames((1, 37, 53, 3), 5))[0]
    assert np.array_equal(D.host_warp(lib, bgr, [1, 0, 0, 0, 1, 0]), bgr)
    assert np.array_equal(D.warp_linear(bgr, [1, 0, 0, 0, 1, 0]), bgr)
    pad = np.pad(bgr, ((40, 40), (60, 60), (0, 0)), mode="edge")
    for tx, ty in ((3, 0), (0, -5), (-7, 11), (60, -40), (-59, 39)):
        want = pad[40 + ty:40 + ty + 37, 60 + tx:60 + tx + 53]                       # result(x, y) = source(x + tx, y + ty)
        assert np.array_equal(D.host_warp(lib, bgr, [1, 0, tx, 0, 1, ty]), want), (tx, ty)


def test_resize_truths(lib):
    bgr = D.as_bgr(D.uniform_frames((1, 600, 600, 3), 6))[0]
    assert np.array_equal(D.host_resize(lib, bgr[:300, :300]), bgr[:300, :300])
    S = bgr.astype(np.int64)
    mean = np.floor((S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2]) / 4.0 + 0.5).astype(np.uint8)
    assert np.array_equal(D.host_resize(lib, bgr), mean)
    for value in (0, 1, 127, 128, 254, 255):
        flat = np.full((61, 97, 3), value, dtype=np.uint8)
        assert (D.host_resize(lib, flat) == value).all()
        assert (D.host_warp(lib, flat, D.rotation(97, 61, 15)[1]) == value).all()
        got, ok = D.host_blob(lib, flat[None], D.rotation(97, 61, -30)[1], (0, 0, 0, 0, 97, 61))
        assert ok and all((got[c] == np.float32(value) - np.float32(D.MEAN[c])).all() for c in range(3))


@pytest.mark.parametrize("key", sorted(D.CASES))
def test_warp_against_the_float64_filter(lib, FF, BF, key):
    """the weights are exact, so the fixed-point sum equals the float64 filter at the same 1/32-pixel coordinates after round-half-up"""
    plan = plan_of(FF, BF, key)
    bgr = D.as_bgr(D.case_frames(key))[0]
    for a, angle in enumerate(plan.angles):
        if angle:
            assert np.array_equal(D.host_warp(lib, bgr, plan.inverse[a]), D.warp_yardstick64(bgr, plan.inverse[a])), (key, angle)


def test_resize_against_float64_bilinear(lib):
    assert abs(D.measure_resize_share() - D.RESIZE_WORST_SHARE) < 1e-12              # the constant is what the restatement shows
    worst_share = 0.0
    for key in sorted(D.CASES):
        bgr = D.as_bgr(D.case_frames(key))[0]
        for h, w in D.case_regions(key):
            levels, share = D.differences(D.host_resize(lib, bgr[:h, :w]), D.resize_yardstick64(bgr[:h, :w]))
            print(f"{key} {w} x {h}: largest difference {levels} levels, {share:.4%} of the bytes differ")
            assert levels <= D.RESIZE_MAX_LEVELS
            worst_share = max(worst_share, share)
    assert worst_share <= 1.5 * D.RESIZE_WORST_SHARE


def test_detect_equals_cv2(lib):
    """wherever cv2 can be imported, or tests/golden/detect_cv2.npz (frame, angle, warped, region, resized) was recorded with it"""
    try:
        import cv2
    except Exception:
        cv2 = None
    if cv2 is None and not os.path.exists(D.cv2_fixture_path()):
        pytest.skip("no cv2 and no tests/golden/detect_cv2.npz: equality with cv2 itself is unpinned here")
    if cv2 is not None:
        bgr = D.as_bgr(D.case_frames("light_640x420"))[0]
        M = cv2.getRotationMatrix2D((320.0, 210.0), 15.0, 1.0)
        assert np.array_equal(M, D.rotation(640, 420, 15)[0])
        warped = cv2.warpAffine(bgr, M, (640, 420), flags=cv2.INTER_LINEAR, borderMode=cv2.BORDER_REPLICATE)
        assert np.array_equal(D.host_warp(lib, bgr, D.rotation(640, 420, 15)[1]), warped)
        assert np.array_equal(D.host_resize(lib, bgr[:294, :384]), cv2.resize(bgr[:294, :384], (300, 300)))
    else:
        data = np.load(D.cv2_fixture_path())
        assert np.array_equal(D.host_warp(lib, data["frame"], D.rotation(data["frame"].shape[1], data["frame"].shape[0], float(data["angle"]))[1]), data["warped"])
        left, top, right, bottom = (int(v) for v in data["region"])
        assert np.array_equal(D.host_resize(lib, data["frame"][top:bottom, left:right]), data["resized"])


def test_abi_and_refusals_without_a_device(hip):
    lib = hip.load_library()
    assert lib.vrg_abi_version() == 8 == hip.ABI_VERSION
    names = {"vrg_linear_taps", "vrg_detect_check", "vrg_detect_blobs_f32", "vrg_detect_blobs_u8", "vrg_warp_linear_u8"}
    assert names <= set(hip.EXPORTED_SYMBOLS)
    header = open(os.path.join(os.path.dirname(hip.PKG_DIR), "include", "vrgdg_hip.h")).read()
    for name in names:
        assert f"int {name}(" in header and getattr(lib._cdll, name).restype is C.c_int
    assert C.sizeof(hip.DetectDesc) == 24 and C.sizeof(hip.DetectFrameDesc) == 8
    null, one, two = C.c_void_p(0), C.c_void_p(64), C.c_void_p(128)      # never dereferenced: validation fails or counts are zero
    assert lib.vrg_detect_blobs_f32(null, 1, 64, 64, 3, null, 0, one, 1, two, null) == 1
    assert lib.vrg_detect_blobs_f32(one, 1, 64, 64, 3, null, 0, null, 1, two, null) == 1
    assert lib.vrg_detect_blobs_f32(one, 1, 64, 64, 3, null, 0, one, 1, null, null) == 1
    assert lib.vrg_detect_blobs_f32(one, 1, 64, 64, 3, null, 2, one, 1, two, null) == 1          # transforms announced, none given
    assert lib.vrg_detect_blobs_f32(one, 1, 64, 64, 2, null, 0, one, 1, two, null) == 1          # C < 3
    assert lib.vrg_detect_blobs_f32(one, 1, 32768, 64, 3, null, 0, one, 1, two, null) == 1
    assert lib.vrg_detect_blobs_f32(one, 1, 64, 32768, 3, null, 0, one, 1, two, null) == 1
    assert lib.vrg_detect_blobs_f32(one, 1, 64, 64, 3, null, 0, one, -1, two, null) == 1
    assert lib.vrg_detect_blobs_f32(one, 1, 64, 64, 3, null, 0, one, 0, two, null) == 0          # zero blobs: no launch
    assert lib.vrg_detect_blobs_f32(null, 0, 64, 64, 3, null, 0, null, 0, null, null) == 0
    assert lib.vrg_detect_blobs_u8(null, 1, 64, 64, null, 0, one, 1, two, null) == 1
    assert lib.vrg_detect_blobs_u8(one, 1, 64, 64, null, 0, one, 0, two, null) == 0
    assert lib.vrg_warp_linear_u8(null, 3, 1, 64, 64, null, 0, one, 1, two, null) == 1
    assert lib.vrg_warp_linear_u8(one, 2, 1, 64, 64, null, 0, one, 1, two, null) == 1            # fp32 frames with fewer than 3 channels
    assert lib.vrg_warp_linear_u8(one, 0, 1, 64, 40000, null, 0, one, 1, two, null) == 1
    assert lib.vrg_warp_linear_u8(one, 0, 1, 64, 64, null, 0, one, 0, two, null) == 0
    assert lib.vrg_linear_taps(0, 300, one, one) == 1 and lib.vrg_linear_taps(300, 300, null, one) == 1

    def check(rows, frames=2, height=400, width=600, transforms=2):
        d = np.array(rows, dtype=np.int32).reshape(-1, 6)
        return lib.vrg_detect_check(C.c_void_p(d.ctypes.data), len(d), frames, height, width, transforms)

    assert check([(0, -1, 0, 0, 600, 400), (1, 1, 592, 392, 600, 400)]) == 0
    for bad in ((2, -1, 0, 0, 600, 400), (-1, -1, 0, 0, 600, 400), (0, 2, 0, 0, 600, 400), (0, -2, 0, 0, 600, 400), (0, 0, -1, 0, 600, 400),
                (0, 0, 0, 0, 601, 400), (0, 0, 0, 0, 600, 401), (0, 0, 10, 10, 10, 50), (0, 0, 10, 10, 17, 50), (0, 0, 10, 10, 50, 17),
                (0, 0, 50, 10, 10, 50)):
        assert check([(0, -1, 0, 0, 600, 400), bad]) == 1, bad
    assert check([], 0, 400, 600, 0) == 0 and check([(0, -1, 0, 0, 600, 400)], 1, 40000, 600, 0) == 1


def test_ops_refuse_before_any_upload(pkg, hip):
    import torch
    from comfyui_vrgamedevgirl_amd import ops
    x = torch.zeros(1, 64, 64, 3)
    for bad in ((0, -1, 0, 0, 65, 64), (1, -1, 0, 0, 64, 64), (0, 0, 0, 0, 64, 64), (0, -1, 0, 0, 7, 64)):
        with pytest.raises(ValueError):
            ops.detect_blobs(x, [bad], None)
    with pytest.raises(ValueError):
        ops.detect_blobs(torch.zeros(1, 64, 64, 2), [(0, -1, 0, 0, 64, 64)], None)
    with pytest.raises(ValueError):
        ops.detect_blobs(torch.zeros(1, 64, 64, 4, dtype=torch.uint8), [(0, -1, 0, 0, 64, 64)], None)
    with pytest.raises(ValueError):
        ops.warp_linear_bytes(x, [(0, 0)], None)
    with pytest.raises(ValueError):
        ops.detect_blobs(x, [(0, 0, 0, 0, 64, 64)], [[1, 0, 0, 0, float("nan"), 0]])


def _outputs(case, slots):
    width = 7 if case["kind"] == "caffe" else 15
    return [[np.array(o, dtype=np.float32).reshape(-1, width) for o in per] + [np.zeros((0, width), np.float32)] * (slots - len(per))
            for per in case["outputs"]]


def test_plan_and_candidates_equal_the_reference_route(FF, BF, golden):
    assert len(golden["cases"]) >= 8
    for case in golden["cases"]:
        if case["module"] == "builder":
            plan = BF.detection_plan(case["width"], case["height"], case["rotation_assist"], case["regions"])
            got = BF.candidates_from_outputs(plan, _outputs(case, plan.slots), case["confidence"], kind=case["kind"])
        else:
            plan = FF.detection_plan(case["width"], case["height"], case["rotation_assist"])
            got = FF.candidates_from_outputs(plan, _outputs(case, plan.slots), case["confidence"], case["minimum_pixels"], kind=case["kind"])
        assert plan.angles == case["angles"], case["key"]
        assert [[list(r) for r in per] for per in plan.regions] == case["region_lists"], case["key"]
        assert [[float(v) for v in item] for item in got] == case["candidates"], case["key"]      # equal as floats
        assert len(plan.transforms) == sum(1 for a in plan.angles if a)
        for a, angle in enumerate(plan.angles):
            assert (plan.inverse[a] is None) == (angle == 0) and plan.transform_index[a] == (-1 if angle == 0 else sum(1 for b in plan.angles[:a] if b))


def test_no_detector_means_no_candidates(FF, BF):
    import torch
    x = torch.zeros(3, 64, 96, 3)
    assert FF.detect_with_rotation(None, x, 0.7, 20, "Light: ±15°") == [[], [], []]
    assert BF.detect_with_rotation(None, x.to(torch.uint8), 0.5) == [[], [], []]
    with pytest.raises(ValueError):
        FF.detection_plan(40000, 64, "Off (fastest)")
    with pytest.raises(ValueError):
        BF.detection_plan(600, 400, "off", [(0, 0, 601, 400)])

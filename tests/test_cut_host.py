"""The shot-aware cut score without a GPU: csrc/vrg_area_math.hpp compiled for the host (tests/host_math/cut_check.cpp) against the
independent numpy restatement and the float64 yardstick of tests/cut_support.py; the host half of the score (cut_scores_from_sums,
boundaries_from_scores) against the reference's own `_cut_score` as recorded in tests/golden/cut_score.json; cv2 itself where a fixture or
the package is at hand; the C ABI of the new entry points and the refusals.  No test here reads the reference checkout."""
import ctypes as C
import inspect
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import cut_support as CS
from conftest import ROOT

# (height, width, channels), frames of each kind: the sizes of the issue
EXACT_CASES = [(size, kind) for size in CS.SIZES for kind in ("uniform", "smooth")] + [((65, 67, 3), "special"), ((480, 854, 3), "special"),
                                                                                      ((512, 512, 3), "special"), ((128, 128, 3), "special"),
                                                                                      ((64, 64, 3), "special"), ((96, 130, 4), "special")]
YARDSTICK_CASES = [(size, kind) for size in ((2160, 3840, 3), (1080, 1920, 3), (720, 1280, 3), (480, 854, 3), (65, 67, 3), (512, 512, 3), (64, 4096, 3),
                                             (64, 64, 3), (96, 130, 4)) for kind in ("uniform", "smooth")]


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return CS.build_host_lib(tmp_path_factory.mktemp("cut_check"))


@pytest.fixture(scope="module")
def FF(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes
    return VRGDG_StandaloneFaceFixNodes


@pytest.fixture(scope="module")
def golden():
    with open(CS.golden_path()) as fh:
        return json.load(fh)


def frames_of(size, kind, seed):
    h, w, c = size
    n = 3 if kind == "special" else (1 if h * w > 1500 * 2500 else 2)
    return CS.FRAME_KINDS[kind]((n, h, w, c), seed)


@pytest.mark.parametrize("size,kind", EXACT_CASES)
def test_host_header_equals_the_restatement(hm, size, kind):
    x = frames_of(size, kind, 300 + size[0] + size[1])
    keep = x.copy()
    want = CS.restated_sums(x)
    got = CS.host_sums(hm, x)
    worst, share = CS.differences(got[0], want[0])
    print(f"{size} {kind}: thumbnails: largest difference {worst} levels, {share:.4%} of the bytes differ; "
          f"histograms differ in {int((got[1] != want[1]).sum())} bins, sums in {int((got[2] != want[2]).sum())} values")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[2].dtype == np.int64 and got[1].dtype == np.int32 and (got[1].sum(axis=1) == 4096).all()
    assert np.array_equal(x, keep)


def test_table_of_the_library_equals_the_header_and_the_restatement(hm, pkg):
    from comfyui_vrgamedevgirl_amd import ops
    for h, w in ((2160, 3840), (1080, 1920), (720, 1280), (480, 854), (512, 512), (128, 128), (64, 64), (65, 67), (64, 4096), (77, 1000)):
        table = ops.area_taps(h, w)
        assert table.shape == (128,) and table.dtype.itemsize == 20
        cells = CS.cells_of(hm, h, w)
        assert np.array_equal(table.view(np.uint8), cells.view(np.uint8))
        for cells_of_axis, n_in in ((table[:64], w), (table[64:], h)):
            taps = CS.axis_taps(n_in)
            assert CS.expand_cells(cells_of_axis) == taps
            assert min(s for _, s, _ in taps) == 0 and max(s for _, s, _ in taps) == n_in - 1       # every tap lies inside the axis
            for d in range(64):                                                                       # the weights of a cell sum to 1
                assert abs(sum(float(a) for dd, _, a in taps if dd == d) - 1.0) < 1e-5
        assert hm.hm_area_mode(h, w) == (0 if h % 64 or w % 64 else (2 if (h, w) == (128, 128) else 1))


@pytest.mark.parametrize("size,kind", YARDSTICK_CASES)
def test_float64_yardstick(hm, size, kind):
    """the thumbnail is at most 1 level from the exact area average in float64 rounded once, on at most 1 % of the bytes"""
    x = frames_of(size, kind, 7)
    got = CS.host_sums(hm, x)[0]
    worst, share = CS.differences(got, CS.yardstick64(x))
    print(f"{size} {kind}: largest difference {worst} levels, {share:.4%} of the bytes differ")
    assert worst <= CS.YARDSTICK_MAX_LEVELS and share <= CS.YARDSTICK_MAX_SHARE


@pytest.mark.parametrize("kind", ("uniform", "smooth"))
def test_two_by_two_rule_is_the_exact_average_rounded_half_up(hm, kind):
    """128 x 128 sources: (a + b + c + d + 2) >> 2 meets the quarters exactly and rounds the halves up, where rint rounds them to even --
    against the yardstick with that tie rule no byte may differ (with ties to even one byte in eight does, by the rule itself)"""
    x = frames_of((128, 128, 3), kind, 7)
    got = CS.host_sums(hm, x)[0]
    worst, share = CS.differences(got, CS.yardstick64(x, ties="up"))
    even = CS.differences(got, CS.yardstick64(x))
    print(f"128 x 128 {kind}: half up: {worst} levels, {share:.4%}; half to even: {even[0]} levels, {even[1]:.4%}")
    assert worst == 0 and share == 0.0 and even[0] <= 1


def test_small_tables_the_issue_relies_on(hm):
    # the reference requantises the thumbnail as ((thumb / 255) * 255).astype(uint8): in fp32 the identity on all 256 values
    t = np.arange(256, dtype=np.float32)
    assert np.array_equal(((t / np.float32(255.0)) * 255).astype(np.uint8), np.arange(256, dtype=np.uint8))
    # calcHist's hue bin floor(h * (32 / 180.0)) in double = (8 h) / 45 in integers, h = 0 .. 179; saturation floor(s * 32 / 256) = s >> 3
    assert [math.floor(h * (32 / 180.0)) for h in range(180)] == [(8 * h) // 45 for h in range(180)]
    assert [math.floor(s * (32 / 256.0)) for s in range(256)] == [s >> 3 for s in range(256)]
    # HSV of the header = HSV of the restatement on a grid of colours and on random ones
    rng = np.random.Generator(np.random.PCG64(11))
    colours = np.concatenate([np.array([[r, g, b] for r in (0, 1, 127, 128, 254, 255) for g in (0, 1, 127, 128, 254, 255) for b in (0, 1, 127, 128, 254, 255)]),
                              rng.integers(0, 256, (4000, 3))]).astype(np.uint8)
    h, s = CS.hsv(colours)
    hh, ss = C.c_int32(), C.c_int32()
    for (r, g, b), wh, ws in zip(colours.tolist(), h.tolist(), s.tolist()):
        hm.hm_cut_hsv(r, g, b, C.byref(hh), C.byref(ss))
        assert (hh.value, ss.value) == (wh, ws) and 0 <= wh < 180 and 0 <= ws < 256


def test_host_scores_lie_within_the_bound_of_the_reference(FF, golden):
    """cut_scores_from_sums on the restatement's thumbnails against the reference's own `_cut_score` (float32 thumbnails, float32 mean,
    normalised float histograms): within 4 x the worst gap the generator measured, which must stay below 1e-5"""
    bound = golden["bound"]
    assert 0.0 < bound < 1e-5 and bound == 4.0 * golden["gap"] and len(golden["cases"]) >= 12
    assert {"hard_cuts", "fade", "flash", "identical", "single_colour"} <= {c["kind"] for c in golden["cases"]}
    for case in golden["cases"]:
        x = CS.make_video(case["kind"], case["shape"], case["seed"])
        _, _, sums = CS.restated_sums(x)
        assert [[int(v) for v in row] for row in sums] == case["sums"], case["key"]
        got = FF.cut_scores_from_sums(sums)
        want = np.asarray(case["scores"], dtype=np.float64)
        worst = float(np.abs(got - want).max())
        print(f"{case['key']}: |score - reference| <= {worst:.3e} (bound {bound:.3e})")
        assert got.dtype == np.float64 and got.shape == want.shape and got[0] == 0.0 and worst <= bound, case["key"]


def test_boundaries_reproduce_the_reference_s_flags(FF, golden):
    margin = 100.0 * golden["bound"]
    cuts = 0
    for case in golden["cases"]:
        scores = FF.cut_scores_from_sums(np.asarray(case["sums"], dtype=np.int64).reshape(-1, 4))
        assert case["thresholds"]
        for t in case["thresholds"]:
            assert all(abs(s - t["cut_sensitivity"]) >= margin for s in case["scores"][1:]), case["key"]
            hard_cut, shot_id = FF.boundaries_from_scores(scores, t["cut_sensitivity"])
            assert hard_cut == t["hard_cut"] and shot_id == t["shot_id"], (case["key"], t["cut_sensitivity"])
            assert all(isinstance(v, bool) for v in hard_cut) and all(isinstance(v, int) for v in shot_id) and not hard_cut[0]
            cuts += sum(hard_cut)
    assert cuts > 10
    assert FF.boundaries_from_scores([0.0, 0.28, 0.27, 0.9], 0.28) == ([False, True, False, True], [0, 1, 1, 2])     # >=, as the reference


def test_score_edge_cases(FF):
    uniform, one_bin = 1024 * 16, 4096 * 4096
    # identical single-colour frames: correlation 1, nothing moved
    assert FF.cut_scores_from_sums([[0, one_bin, one_bin, one_bin]]).tolist() == [0.0, 0.0]
    # two different single colours: disjoint histograms
    s = FF.cut_scores_from_sums([[0, one_bin, one_bin, 0]])[1]
    assert abs(s - 0.5 * (1.0 + 1.0 / 1023.0)) < 1e-15
    # a flat histogram has no variance: cv2's denominator test fails and the correlation is 1
    assert FF.cut_scores_from_sums([[255 * 12288, uniform, one_bin, 4096 * 4]])[1] == 1.0 and FF.cut_scores_from_sums([[0, uniform, uniform, uniform]])[1] == 0.0
    assert FF.cut_scores_from_sums(np.zeros((0, 4), dtype=np.int64)).tolist() == [0.0]


def test_cut_score_equals_cv2(hm):
    """the pin: cv2's own thumbnails and histograms, from the fixture if it was made, else from an importable cv2; neither is at hand
    everywhere"""
    if os.path.exists(CS.cv2_fixture_path()):
        data = np.load(CS.cv2_fixture_path())
        keys = json.loads(str(data["provenance"]))["cases"]
        cases = [(data[k + ".in"], data[k + ".thumbs"], data[k + ".hist"]) for k in keys]
    else:
        cv2 = pytest.importorskip("cv2", reason="neither tests/golden/cut_score_cv2.npz nor the cv2 package (opencv-python) is available")
        cases = []
        for size in CS.SIZES:
            x = frames_of(size, "uniform", 31)
            rgb = CS.quantise(x)
            thumbs = np.stack([cv2.resize(f, (64, 64), interpolation=cv2.INTER_AREA) for f in rgb])
            hist = np.stack([cv2.calcHist([cv2.cvtColor(t, cv2.COLOR_RGB2HSV)], [0, 1], None, [32, 32], [0, 180, 0, 256]).reshape(-1) for t in thumbs])
            cases.append((x, thumbs, hist))
    for x, thumbs, hist in cases:
        got_t, got_h, _ = CS.host_sums(hm, x)
        worst, share = CS.differences(got_t, thumbs)
        print(f"{x.shape}: largest difference {worst} levels, {share:.4%} of the bytes differ")
        assert np.array_equal(got_t, thumbs) and np.array_equal(got_h, np.asarray(hist).astype(np.int32))
        assert np.array_equal(CS.thumbnails(x), thumbs)


def test_refusals(FF, pkg):
    from comfyui_vrgamedevgirl_amd import ops
    for call in (FF.shot_cut_scores, lambda v: FF.shot_boundaries(v, 0.28)):
        with pytest.raises(ValueError, match="below 64 px"):
            call(torch.zeros(2, 63, 80, 3))
        with pytest.raises(ValueError, match="below 64 px"):
            call(torch.zeros(2, 80, 63, 3))
        with pytest.raises(ValueError, match="non-empty video batch"):
            call(torch.zeros(64, 64, 3))
        with pytest.raises(ValueError, match="non-empty video batch"):
            call(torch.zeros(0, 64, 64, 3))
        with pytest.raises(ValueError, match="at least 3 channels"):
            call(torch.zeros(2, 64, 64, 2))
        with pytest.raises(ValueError):
            call(np.zeros((2, 64, 64, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        ops.area_taps(63, 64)
    with pytest.raises(ValueError, match="below 64 px"):
        ops.cut_thumbnails_host(torch.zeros(1, 10, 100, 3))


def _prototype(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vrgdg_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_library_exports_the_symbols_and_the_abi_is_8(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    lib = _hip.load_library()
    assert lib.vrg_abi_version() == 8 == _hip.ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read(), flags=re.S)
    assert "#define VRG_ABI_VERSION 8" in header
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    for name in ("vrg_area_taps", "vrg_cut_thumbs_f32", "vrg_cut_hist_u8", "vrg_cut_pair_sums"):
        assert name in _hip.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        proto = _prototype(header, name)
        res, args = _hip._SIGNATURES[name]
        assert res is C.c_int and len(proto) == len(args), name
        for text, ctype in zip(proto, args):
            assert ctype is (C.c_void_p if "*" in text else kinds[text.split()[0]]), (name, text)
    assert "vrg_area_math.hpp" in build_ext.HEADERS and "vrg_cut.hip" in build_ext.SOURCES


def test_entry_point_refusals_without_device(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    lib = _hip.load_library()
    null, a, b, t = C.c_void_p(0), C.c_void_p(64), C.c_void_p(4096), C.c_void_p(256)

    def thumbs(i=a, o=b, frames=1, h=64, w=64, c=3, taps=t):
        return lib.vrg_cut_thumbs_f32(i, o, frames, h, w, c, taps, null)

    assert thumbs(frames=0) == _hip.VRG_OK                                             # zero frames: no launch
    assert thumbs(i=null) == thumbs(o=null) == thumbs(taps=null) == thumbs(o=a) == _hip.VRG_ERR_BAD_ARG
    assert thumbs(frames=-1) == thumbs(h=63) == thumbs(w=63) == thumbs(c=2) == thumbs(c=5) == _hip.VRG_ERR_BAD_ARG
    assert thumbs(i=C.c_void_p(66)) == thumbs(taps=C.c_void_p(258)) == _hip.VRG_ERR_BAD_ARG      # not on the 4-byte grid
    assert thumbs(h=65536, w=65536, frames=1) == _hip.VRG_ERR_UNSUPPORTED              # a frame of more than 2^31 floats
    assert lib.vrg_cut_hist_u8(a, b, 0, null) == _hip.VRG_OK and lib.vrg_cut_hist_u8(null, b, 1, null) == _hip.VRG_ERR_BAD_ARG
    assert lib.vrg_cut_hist_u8(a, null, 1, null) == lib.vrg_cut_hist_u8(a, b, -1, null) == _hip.VRG_ERR_BAD_ARG
    assert lib.vrg_cut_pair_sums(a, b, t, 1, null) == lib.vrg_cut_pair_sums(a, b, t, 0, null) == _hip.VRG_OK      # no pair: no launch
    assert lib.vrg_cut_pair_sums(null, b, t, 2, null) == lib.vrg_cut_pair_sums(a, null, t, 2, null) == _hip.VRG_ERR_BAD_ARG
    assert lib.vrg_cut_pair_sums(a, b, null, 2, null) == lib.vrg_cut_pair_sums(a, b, C.c_void_p(260), 2, null) == _hip.VRG_ERR_BAD_ARG
    assert lib.vrg_area_taps(64, 64, null) == lib.vrg_area_taps(63, 64, a) == lib.vrg_area_taps(64, 0, a) == _hip.VRG_ERR_BAD_ARG


def test_python_surface(pkg, FF):
    from comfyui_vrgamedevgirl_amd import _devices, ops
    assert list(inspect.signature(FF.shot_cut_scores).parameters) == ["video_frames"]
    assert list(inspect.signature(FF.shot_boundaries).parameters) == ["video_frames", "cut_sensitivity"]
    assert list(inspect.signature(ops.cut_thumbnails).parameters)[0] == "frames"
    assert list(inspect.signature(ops.cut_thumbnails_host).parameters) == ["frames_cpu"]
    assert list(inspect.signature(ops.cut_pair_sums).parameters)[0] == "thumbs"
    assert callable(_devices.upload_frames)
    assert set(FF.NODE_CLASS_MAPPINGS) == {"VRGDGFaceFixComposite", "VRGDGFaceFixCompositeOpaque"}
    assert not [k for k in pkg.NODE_CLASS_MAPPINGS if "cut" in k.lower() or "shot" in k.lower()]
    assert "cut scoring" not in FF.__doc__

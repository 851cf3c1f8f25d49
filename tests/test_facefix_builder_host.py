"""The AI Video Builder's Face Fix without a GPU: csrc/vrg_facefix_math.hpp compiled for the host (tests/host_math/facefix_check.cpp) against
the independent numpy restatement and the float64 yardstick of tests/facefix_builder_support.py; the span table against the analytic
ellipse; cv2 itself where a fixture or the package is at hand (neither is everywhere: the ellipse rasteriser and the Gaussian arithmetic of
cv2 are NOT pinned without them); the host functions against values recorded from the reference; the C ABI of the new entry points and
their refusals.  No test here reads the reference checkout."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import facefix_builder_support as FS
import lanczos_support as LS
from conftest import ROOT

MASK_SIZES = ((37, 41), (20, 23), (64, 64), (5, 5), (1, 7), (7, 1), (2, 2), (90, 90), (33, 64), (101, 57), (12, 30), (28, 29), (640, 360))
FEATHERS = (0, 1, 18)
NEW_SYMBOLS = ("vrg_ff_ellipse_spans", "vrg_ff_gauss_coeffs", "vrg_lanczos4_boxes_u8", "vrg_ff_masks_f32", "vrg_ff_resize_stats_u8",
               "vrg_ff_composite_u8")


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return FS.build_host_lib(tmp_path_factory.mktemp("facefix_check"))


@pytest.fixture(scope="module")
def fixture():
    with open(FS.FIXTURE_JSON) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def ff(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix, _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return VRGDG_FaceFix


@pytest.mark.parametrize("w,h", MASK_SIZES)
def test_spans_of_the_header_equal_the_restatement(hm, ff, w, h):
    want = FS.ellipse_spans(w, h, *FS.mask_geometry(w, h))
    assert np.array_equal(FS.host_spans(hm, w, h), want)
    assert np.array_equal(ff.ellipse_spans(w, h), want)                   # the library's host function is the header


@pytest.mark.parametrize("feather", (0, 1, 2, 18, 77, 256))
def test_coefficients_equal_the_restatement(hm, ff, feather):
    n = FS.gauss_taps(feather)
    want = FS.gauss_coeffs(n, max(0.1, feather))
    got = np.zeros(n, dtype=np.float32)
    hm.hm_ff_coeffs(feather, got)
    assert n == ff.gauss_taps(feather) == max(3, 4 * feather + 1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(ff.gauss_coeffs(feather).view(np.uint32), want.view(np.uint32))
    assert abs(float(want.astype(np.float64).sum()) - 1.0) < 1e-5


@pytest.mark.parametrize("w,h", [s for s in MASK_SIZES if s[0] * s[1] <= 10000])
@pytest.mark.parametrize("feather", FEATHERS)
def test_mask_of_the_header_equals_the_restatement_bit_for_bit(hm, fixture, w, h, feather):
    want = FS.soft_ellipse_mask(w, h, feather)
    got = FS.host_mask(hm, w, h, feather)
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    gap = float(np.abs(got.astype(np.float64) - FS.yardstick_mask(w, h, feather)).max())
    print(f"{w} x {h}, feather {feather}: {gap:.3e} from the float64 yardstick (recorded gap_mask {fixture['gap_mask']:.3e})")
    assert gap <= FS.MASK_BOUND_FACTOR * fixture["gap_mask"]
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0


def test_mask_with_more_taps_than_pixels(hm, fixture):
    """feather 256 on 64 x 64 (1025 taps: every index is reflected many times) and feather 18 on 20 x 23 (73 taps)"""
    for w, h, feather in ((64, 64, 256), (20, 23, 18), (1, 7, 18)):
        want = FS.soft_ellipse_mask(w, h, feather)
        got = FS.host_mask(hm, w, h, feather)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert float(np.abs(got.astype(np.float64) - FS.yardstick_mask(w, h, feather)).max()) <= FS.MASK_BOUND_FACTOR * fixture["gap_mask"]


def test_reflect101_repeats(pkg):
    assert list(FS.reflect101(np.arange(-9, 10), 4)) == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3]
    assert list(FS.reflect101(np.arange(-3, 4), 1)) == [0] * 7 and list(FS.reflect101(np.arange(-3, 5), 2)) == [1, 0, 1, 0, 1, 0, 1, 0]


def _inside(hm, w, h):
    spans = FS.host_spans(hm, w, h)
    (cx, cy), (ax, ay) = FS.mask_geometry(w, h)
    return FS.spans_to_plane(spans, w, np.uint8).astype(bool), cx, cy, ax, ay


@pytest.mark.parametrize("w,h", MASK_SIZES + ((1920, 1080), (511, 512)))
def test_spans_against_the_analytic_ellipse(hm, w, h):
    """with m = 1.5 / min(ax, ay): every pixel of normalised radius <= 1 - m is inside, none of radius > 1 + m is"""
    inside, cx, cy, ax, ay = _inside(hm, w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    radius = np.sqrt(((xx - cx) / ax) ** 2 + ((yy - cy) / ay) ** 2)
    m = 1.5 / min(ax, ay)
    assert not (~inside & (radius <= 1.0 - m)).any()
    assert not (inside & (radius > 1.0 + m)).any()


@pytest.mark.parametrize("w,h", MASK_SIZES + ((1920, 1080), (511, 512)))
def test_spans_are_symmetric_about_the_centre(hm, w, h):
    """The spans are symmetric under the reflections the centre allows: about the centre column and the centre row, over the pixels whose
    mirror image lies inside the plane.  (FillConvexPoly's outline as restated is not: Line2 walks every edge from its left or upper end,
    so an edge and its mirror image can land one pixel apart at the end of a row; ff_ellipse_spans closes the spans under both
    reflections.)"""
    inside, cx, cy, _, _ = _inside(hm, w, h)
    xlo, xhi, ylo, yhi = max(0, 2 * cx - (w - 1)), min(w - 1, 2 * cx), max(0, 2 * cy - (h - 1)), min(h - 1, 2 * cy)
    sub = inside[ylo:yhi + 1, xlo:xhi + 1]
    print(f"{w} x {h}: {int((sub != sub[:, ::-1]).sum())} / {int((sub != sub[::-1, :]).sum())} pixels differ from their mirror image about the "
          f"centre column / row, of {int(sub.sum())} filled")
    assert np.array_equal(sub, sub[:, ::-1]) and np.array_equal(sub, sub[::-1, :])


@pytest.mark.parametrize("key", sorted(FS.COMPOSITE_CASES))
def test_bytes_of_the_header_equal_the_restatement(hm, key):
    originals, enhanced, boxes, strengths, feather, cm = FS.case_inputs(key)
    k = 0
    for f, box in enumerate(boxes):
        if box is None:
            continue
        e, k = enhanced[k], k + 1
        left, top, right, bottom = box
        w, h = right - left, bottom - top
        mask = FS.soft_ellipse_mask(w, h, feather)
        resized = np.asarray(LS.restated(e[None], w, h))[0]
        target = np.ascontiguousarray(originals[f, top:bottom, left:right])
        face, sums = FS.color_match(resized, target, mask, cm)
        want = FS.blend(target, face, mask, strengths[f])
        got, got_sums = FS.host_composite(hm, target, resized, mask, cm, strengths[f])
        assert got_sums == sums, (key, f)
        assert np.array_equal(got, want), (key, f, LS.differences(got, want))


def test_mean_shift_needs_sixteen_pixels_and_clips(hm):
    rng = np.random.Generator(np.random.PCG64(77))
    target = rng.integers(0, 256, size=(6, 6, 3), dtype=np.uint8)
    face = rng.integers(0, 60, size=(6, 6, 3), dtype=np.uint8)
    for selected in (15, 16):
        mask = np.zeros(36, dtype=np.float32)
        mask[:selected] = 0.36
        mask[selected:] = 0.35                                               # 0.35 itself is not selected
        mask = mask.reshape(6, 6)
        got, sums = FS.host_composite(hm, target, face, mask, 1.0, 1.0)
        want_face, want_sums = FS.color_match(face, target, mask, 1.0)
        assert sums == want_sums and sums[0] == selected
        assert np.array_equal(got, FS.blend(target, want_face, mask, 1.0))
        assert (want_face is face) == (selected < 16)


def test_ellipse_spans_equal_cv2(hm):
    """the pin of the rasteriser: cv2's own fill, from the fixture if it was made, else from an importable cv2"""
    if os.path.exists(FS.CV2_FIXTURE):
        data = np.load(FS.CV2_FIXTURE)
        cases = [((int(w), int(h)), data[f"plane.{w}x{h}"]) for w, h in data["sizes"]]
    else:
        cv2 = pytest.importorskip("cv2", reason="neither tests/golden/facefix_builder_cv2.npz nor the cv2 package (opencv-python) is available")
        cases = []
        for w, h in MASK_SIZES:
            plane = np.zeros((h, w), dtype=np.float32)
            centre, axes = FS.mask_geometry(w, h)
            cv2.ellipse(plane, centre, axes, 0, 0, 360, 1.0, -1)
            cases.append(((w, h), plane))
    for (w, h), plane in cases:
        assert np.array_equal(FS.spans_to_plane(FS.host_spans(hm, w, h), w), plane), (w, h)


def test_mask_close_to_cv2(hm, fixture):
    """cv2's GaussianBlur may order its sums differently: the mask must lie within the recorded bound of cv2's, not equal it"""
    if os.path.exists(FS.CV2_FIXTURE):
        data = np.load(FS.CV2_FIXTURE)
        cases = [((int(w), int(h), int(f)), data[f"mask.{w}x{h}.{f}"]) for w, h in data["sizes"] for f in data["feathers"]]
    else:
        cv2 = pytest.importorskip("cv2", reason="neither tests/golden/facefix_builder_cv2.npz nor the cv2 package (opencv-python) is available")
        cases = []
        for w, h in MASK_SIZES[:8]:
            for feather in FEATHERS:
                plane = np.zeros((h, w), dtype=np.float32)
                centre, axes = FS.mask_geometry(w, h)
                cv2.ellipse(plane, centre, axes, 0, 0, 360, 1.0, -1)
                if feather:
                    plane = cv2.GaussianBlur(plane, (4 * feather + 1, 4 * feather + 1), max(0.1, feather))
                cases.append(((w, h, feather), plane.clip(0.0, 1.0)))
    for (w, h, feather), want in cases:
        got = FS.host_mask(hm, w, h, feather)
        assert float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) <= 2 * FS.MASK_BOUND_FACTOR * fixture["gap_mask"], (w, h, feather)


def test_composite_equals_cv2(hm):
    """the whole route with cv2's own resize, ellipse and blur under the reference's numpy lines"""
    if os.path.exists(FS.CV2_FIXTURE):
        data = np.load(FS.CV2_FIXTURE)
        wants = {key: data["composite." + key] for key in FS.COMPOSITE_CASES if "composite." + key in data}
    else:
        cv2 = pytest.importorskip("cv2", reason="neither tests/golden/facefix_builder_cv2.npz nor the cv2 package (opencv-python) is available")
        wants = {}
        for key in FS.COMPOSITE_CASES:
            originals, enhanced, boxes, strengths, feather, cm = FS.case_inputs(key)
            out, k = originals.copy(), 0
            for f, box in enumerate(boxes):
                if box is None:
                    continue
                e, k = enhanced[k], k + 1
                if strengths[f] <= 0:
                    continue
                left, top, right, bottom = box
                w, h = right - left, bottom - top
                alpha = np.zeros((h, w), dtype=np.float32)
                cv2.ellipse(alpha, *FS.mask_geometry(w, h), 0, 0, 360, 1.0, -1)
                if feather:
                    alpha = cv2.GaussianBlur(alpha, (4 * feather + 1, 4 * feather + 1), max(0.1, feather))
                alpha = alpha.clip(0.0, 1.0)
                target = originals[f, top:bottom, left:right]
                face, _ = FS.color_match(cv2.resize(e, (w, h), interpolation=cv2.INTER_LANCZOS4), target, alpha, cm)
                out[f, top:bottom, left:right] = FS.blend(target, face, alpha, strengths[f])
            wants[key] = out
    assert wants
    for key, want in wants.items():
        assert np.array_equal(FS.composite(*FS.case_inputs(key)), want), key


def test_square_crop_box_and_settings_give_the_reference_s_answers(ff, fixture):
    rows = fixture["square_crop_box"]
    assert len(rows) >= 40
    for row in rows:
        got = ff._square_crop_box(tuple(row["face_box"]), row["width"], row["height"], row["padding"])
        assert isinstance(got, tuple) and list(got) == row["result"], row
    settings = fixture["settings"]
    assert any(r["payload"].get("feather") == 0 for r in settings) and any(r["payload"].get("color_match") == 0 for r in settings)
    for row in settings:
        assert ff.settings_from_payload(row["payload"]) == row["result"], row
    assert ff.settings_from_payload({"feather": 0, "color_match": 0}) == {"feather": 18, "color_match": 0.65}
    assert ff.settings_from_payload({}) == {"feather": 18, "color_match": 0.65}
    assert ff.NODE_CLASS_MAPPINGS == {}


def test_fixture_is_small_and_complete(fixture):
    assert os.path.getsize(FS.FIXTURE_NPZ) + os.path.getsize(FS.FIXTURE_JSON) <= 300 * 1024
    data = np.load(FS.FIXTURE_NPZ)
    assert {c["key"] for c in fixture["composites"]} == set(FS.COMPOSITE_CASES)
    for case in fixture["composites"]:
        assert case["selected_max"] <= 65793
        for f, box in enumerate(case["boxes"]):
            if box is not None:
                assert data[f"composite.{case['key']}.{f}"].shape == (box[3] - box[1], box[2] - box[0], 3)
    assert 0.0 < fixture["gap_mask"] < 1e-5
    big = fixture["large_box_measurement"]
    assert big["selected"] > 65793 and big["largest_difference_levels"] <= 1


def _prototype(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vrgdg_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_library_exports_the_symbols_and_the_abi_is_8(ff):
    from comfyui_vrgamedevgirl_amd import _hip
    lib = _hip.load_library()
    assert lib.vrg_abi_version() == 8 == _hip.ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read(), flags=re.S)
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    for name in NEW_SYMBOLS:
        assert name in _hip.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        proto = _prototype(header, name)
        res, args = _hip._SIGNATURES[name]
        assert res is C.c_int and len(proto) == len(args), name
        for text, ctype in zip(proto, args):
            assert ctype is (C.c_void_p if "*" in text else kinds[text.split()[0]]), (name, text)
    # the records as the header lays them out
    assert C.sizeof(_hip.FaceFixBoxDesc) == 32 and _hip.FaceFixBoxDesc.taps_offset.offset == 24
    assert C.sizeof(_hip.FaceFixMaskDesc) == 24 and _hip.FaceFixMaskDesc.span_offset.offset == 8
    assert C.sizeof(_hip.FaceFixDesc) == 48 and _hip.FaceFixDesc.strength.offset == 20 and _hip.FaceFixDesc.mask_offset.offset == 24
    for struct, fields in ((_hip.FaceFixBoxDesc, "vrg_ff_box_desc"), (_hip.FaceFixMaskDesc, "vrg_ff_mask_desc"), (_hip.FaceFixDesc, "vrg_ff_desc")):
        body = re.search(r"typedef struct " + fields + r" \{(.*?)\} " + fields + ";", header, flags=re.S).group(1)
        names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f[0] for f in struct._fields_], fields


def test_refusals_without_device(ff):
    from comfyui_vrgamedevgirl_amd import _hip
    lib = _hip.load_library()
    null, a, b, c, d, e, t, s = (C.c_void_p(v) for v in (0, 64, 128, 192, 256, 320, 384, 448))
    ok, bad, unsupported = _hip.VRG_OK, _hip.VRG_ERR_BAD_ARG, _hip.VRG_ERR_UNSUPPORTED

    def boxes(i=a, frames=1, h=8, w=8, o=b, desc=c, n=1, oh=4, ow=4, taps=t, n_taps=8):
        return lib.vrg_lanczos4_boxes_u8(i, frames, h, w, o, desc, n, oh, ow, taps, n_taps, null)

    assert boxes(n=0) == ok                                                  # zero frames: no launch
    assert boxes(i=null) == boxes(o=null) == boxes(desc=null) == boxes(taps=null) == bad
    assert boxes(o=a) == bad                                                 # in == out
    assert boxes(taps=C.c_void_p(386)) == bad                                # the table is read as dwords
    assert boxes(n=-1) == boxes(frames=-1) == boxes(n_taps=-1) == bad
    for key in ("h", "w", "oh", "ow"):
        assert boxes(**{key: 0}) == bad
    assert boxes(oh=40000, ow=40000) == unsupported

    def masks(spans=a, n_spans=8, coeffs=b, n=5, desc=c, n_masks=1, largest=16, scratch=d, out=e, floats=16):
        return lib.vrg_ff_masks_f32(spans, n_spans, coeffs, n, desc, n_masks, largest, scratch, out, floats, null)

    assert masks(n_masks=0) == ok and masks(largest=0) == ok
    assert masks(spans=null) == masks(desc=null) == masks(out=null) == bad
    assert masks(coeffs=null) == masks(scratch=null) == bad and masks(scratch=e) == bad
    assert masks(n=4) == bad and masks(n=1027) == bad and masks(n=-1) == bad         # an even count, more than feather 256 gives
    assert masks(n_masks=-1) == masks(floats=-1) == masks(n_spans=-1) == bad

    def stats(orig=a, enh=b, mk=c, desc=d, taps=t, face=e, st=s, frames=1, n_enh=1, h=8, w=8, eh=4, ew=4, largest=16, cm=0.5):
        return lib.vrg_ff_resize_stats_u8(orig, enh, mk, 16, desc, taps, 8, face, 48, st, frames, n_enh, h, w, eh, ew, largest, cm, null)

    assert stats(frames=0) == ok
    assert stats(orig=null) == stats(enh=null) == stats(mk=null) == stats(desc=null) == stats(taps=null) == stats(face=null) == stats(st=null) == bad
    assert stats(face=a) == stats(face=b) == bad                             # the packed bytes alias an input
    assert stats(st=C.c_void_p(452)) == bad                                  # the sums are 64-bit
    assert stats(frames=-1) == stats(n_enh=-1) == stats(largest=-1) == bad
    for key in ("h", "w", "eh", "ew"):
        assert stats(**{key: 0}) == bad

    def comp(orig=a, mk=c, desc=d, face=e, st=s, o=b, frames=1, h=8, w=8):
        return lib.vrg_ff_composite_u8(orig, mk, 16, desc, face, 48, st, o, frames, h, w, null)

    assert comp(frames=0) == ok
    assert comp(orig=null) == comp(mk=null) == comp(desc=null) == comp(face=null) == comp(st=null) == comp(o=null) == bad
    assert comp(o=a) == bad and comp(o=e) == bad                             # in == out
    assert comp(frames=-1) == comp(h=0) == comp(w=0) == bad
    assert comp(h=30000, w=30000) == unsupported
    assert lib.vrg_ff_ellipse_spans(4, 4, null) == bad and lib.vrg_ff_ellipse_spans(0, 4, a) == bad
    assert lib.vrg_ff_gauss_coeffs(3, null) == bad and lib.vrg_ff_gauss_coeffs(-1, a) == bad and lib.vrg_ff_gauss_coeffs(257, a) == bad


def test_python_surface(ff):
    import inspect
    import torch
    assert list(inspect.signature(ff.crop_frames).parameters) == ["frames_u8", "crop_boxes", "enhance_size"]
    assert list(inspect.signature(ff.composite_frames).parameters) == ["originals_u8", "enhanced_u8", "crop_boxes", "strengths", "feather",
                                                                       "color_match"]
    assert list(inspect.signature(ff._soft_ellipse_mask).parameters) == ["width", "height", "feather"]
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="Invalid crop box for frame 1"):
        ff.composite_frames(frames, frames, [None, (3, 3, 3, 6)], 1.0, 18, 0.65)
    with pytest.raises(ValueError, match="Invalid crop box for frame 0"):
        ff.crop_frames(frames, [(5, 2, 4, 6), None], 16)
    with pytest.raises(ValueError):
        ff.crop_frames(frames, [(0, 0, 9, 9), None], 16)                    # outside the frame
    with pytest.raises(ValueError):
        ff.crop_frames(frames, [None], 16)                                  # one entry per frame
    with pytest.raises(ValueError):
        ff.crop_frames(frames.float(), [None, None], 16)
    with pytest.raises(ValueError):
        ff.ellipse_spans(0, 5)

"""The far-face repair composite without a GPU: the numpy restatement of tests/far_face_support.py and csrc/vrg_pil_math.hpp compiled for the
host (tests/host_math/farface_check.cpp) equal INSTALLED PILLOW ITSELF byte for byte -- Image.resize(LANCZOS) on RGB and L, the
soft-ellipse mask through GaussianBlur, Image.paste under an L mask -- and numpy's own fp32 means bit for bit, in the plain form and in the
parallel form the kernel uses; both equal what the reference's own functions recorded in tests/golden/far_face.{json,npz}; the steered
case tells numpy's means from exact means; the C ABI of the new entry points and their refusals.  No test here reads the reference checkout."""
import ctypes as C
import hashlib
import inspect
import json
import os
import re

import numpy as np
import pytest

import far_face_support as S
from conftest import ROOT

NEW_SYMBOLS = ("vrg_pil_lanczos_ksize", "vrg_pil_lanczos_table", "vrg_pil_box_parameters", "vrg_pil_resize_u8", "vrg_pil_mask_u8",
               "vrg_np_masked_means_f32", "vrg_pil_paste_u8")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return S.build_host_lib(tmp_path_factory.mktemp("farface_check"))


@pytest.fixture(scope="module")
def golden():
    with open(S.FIXTURE_JSON) as fh:
        return json.load(fh), np.load(S.FIXTURE_NPZ)


@pytest.fixture(scope="module")
def ffr(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext, far_face_repair
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return far_face_repair


@pytest.mark.parametrize("case", S.RESIZE_CASES)
@pytest.mark.parametrize("channels", (3, 0))
def test_resize_equals_pillow(hm, golden, case, channels):
    Image = pytest.importorskip("PIL.Image")
    (iw, ih), (ow, oh) = case
    img = S.random_image(3000 + S.RESIZE_CASES.index(case), ih, iw, channels)
    want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.Resampling.LANCZOS))
    assert np.array_equal(S.resize(img, (ow, oh)), want)
    assert np.array_equal(S.host_resize(hm, img, (ow, oh)), want)
    assert np.array_equal(golden[1][f"resize.{iw}x{ih}.{ow}x{oh}.{'RGB' if channels else 'L'}"], want)
    for n_in, n_out in ((iw, ow), (ih, oh)):
        for got, ref in zip(S.host_table(hm, n_in, n_out), S.lanczos_table(n_in, n_out)):
            assert np.array_equal(got, ref)


def test_library_tables_are_the_header(hm, ffr):
    for n_in, n_out in ((33, 90), (128, 37), (300, 7), (1, 5)):
        ksize, table = ffr.lanczos_table(n_in, n_out)
        bounds, weights = S.host_table(hm, n_in, n_out)
        assert ksize == weights.shape[1] == S.lanczos_ksize(n_in, n_out)
        assert np.array_equal(table[:2 * n_out].reshape(-1, 2), bounds) and np.array_equal(table[2 * n_out:].reshape(n_out, ksize), weights)
    for feather in (1, 2, 18, 40, 300):
        assert ffr.box_parameters(feather) == S.host_box(hm, float(feather)) == S.box_parameters(feather)
    assert S.box_parameters(1) == (0, 11184811, 2796202)                    # the quotient is rounded to float first: not ...810


@pytest.mark.parametrize("size", S.MASK_SIZES)
@pytest.mark.parametrize("feather", S.FEATHERS)
def test_mask_equals_pillow(hm, golden, ffr, size, feather):
    pytest.importorskip("PIL")
    from PIL import Image, ImageDraw, ImageFilter
    w, h = size
    inset_x, inset_y = int(round(w * 0.12)), int(round(h * 0.12))
    want = Image.new("L", size, 0)
    ImageDraw.Draw(want).ellipse((inset_x, inset_y, w - inset_x, h - inset_y), fill=255)
    if feather > 0:
        want = want.filter(ImageFilter.GaussianBlur(radius=float(feather)))
    want = np.asarray(want)
    assert np.array_equal(S.soft_face_mask(size, feather), want)
    assert np.array_equal(S.host_mask(hm, size, feather), want)
    assert np.array_equal(golden[1][f"mask.{w}x{h}.{feather}"], want)       # the reference's own soft_face_mask
    assert np.array_equal(ffr.ellipse_spans(w, h), S.ellipse_spans(w, h))
    if feather in (1, 18) and w * h <= 4000:                                # the running accumulator gives the bytes of the prefix sums
        assert np.array_equal(S.gaussian_blur(S.spans_to_mask(S.ellipse_spans(w, h), w), float(feather), S._box_lines), want)


def test_blur_of_random_bytes_equals_pillow(hm):
    pytest.importorskip("PIL")
    from PIL import Image, ImageFilter
    for (w, h), sigma in (((90, 71), 1), ((37, 41), 2), ((12, 9), 18), ((33, 33), 5)):
        img = S.random_image(77, h, w, 0)
        want = np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius=float(sigma))))
        assert np.array_equal(S.gaussian_blur(img, float(sigma)), want)


def test_paste_equals_pillow(hm):
    Image = pytest.importorskip("PIL.Image")
    o, r, m = S.random_image(5, 40, 50), S.random_image(6, 40, 50), S.random_image(7, 40, 50, 0)
    m[0], m[1] = 0, 255
    want = Image.fromarray(o)
    want.paste(Image.fromarray(r), (0, 0), Image.fromarray(m))
    want = np.asarray(want)
    assert np.array_equal(S.paste(o, r, m), want) and np.array_equal(S.host_paste(hm, o, r, m), want)
    assert np.array_equal(want[0], o[0]) and np.array_equal(want[1], r[1])
    two = ((o.astype(np.int64) * (255 - m[:, :, None]) + 127) // 255 + (r.astype(np.int64) * m[:, :, None] + 127) // 255)
    assert not np.array_equal(two, want)                                    # two separately rounded products are not the paste


@pytest.mark.parametrize("key", S.MEANS_CASES)
def test_means_equal_numpy(hm, golden, key):
    o, r, m = S.means_inputs(key)
    rec = {c["key"]: c for c in golden[0]["means"]}[key]
    selected = (m.astype(np.float32) / 255.0) > 0.25
    count = int(selected.sum())
    om, rm = o.astype(np.float32)[selected].mean(axis=0), r.astype(np.float32)[selected].mean(axis=0)     # numpy itself
    shift = (om - rm) * 0.65
    assert shift.dtype == np.float32
    adjusted, c2, om2, rm2, shift2 = S.color_match(o, r, m)
    want = [count] + S.bits(om) + S.bits(rm) + S.bits(shift) + [int(count >= 16), 0]
    assert [c2] + S.bits(om2) + S.bits(rm2) + S.bits(shift2) == want[:10]
    for parallel in (0, 1):
        assert [int(v) for v in S.host_means(hm, o, r, m, parallel)] == want, parallel
    assert [rec["count"]] + rec["original_mean_bits"] + rec["repaired_mean_bits"] + rec["shift_bits"] == want[:10]
    assert sha(adjusted) == rec["sha256"]
    assert np.array_equal(S.host_paste(hm, o, r, np.full_like(m, 255), S.host_means(hm, o, r, m, 1)), adjusted)
    assert (adjusted is r) == (count < 16)
    if key in ("400_ge200", "560_random", "560_ge128"):
        assert rec["sequential_differs_from_exact"] and S.bits(S.exact_means(o, m)[1]) != S.bits(om)
        assert count * 200 > (1 << 24) or key != "400_ge200"


def test_maps_compose_associatively(hm):
    """the claim the parallel form rests on: maps of runs, reduced pairwise, give the sequential fp32 sum -- over four binade crossings"""
    big = S.random_image(11, 700, 700, 3, 250, 256)                         # crosses 2^24, 2^25, 2^26 and 2^27
    mask = np.full((700, 700), 255, np.uint8)
    assert [int(v) for v in S.host_means(hm, big, big, mask, 1)] == [int(v) for v in S.host_means(hm, big, big, mask, 0)]
    assert S.bits(S.sequential_means(big, mask)[1]) == [int(v) for v in S.host_means(hm, big, big, mask, 1)[1:4]]


def test_composites_equal_the_reference(hm, golden):
    originals, repaired, masks = S.composite_inputs()
    for i, (feather, cm) in enumerate(S.COMPOSITE_VARIANTS):
        rec = golden[0]["composites"][i]
        assert (rec["feather"], rec["color_match"]) == (feather, cm)
        got = S.composite(originals, repaired, S.COMPOSITE_BOXES, feather, cm, masks)
        assert [sha(f) for f in got] == rec["frame_sha256"]
        for f in rec["stored_boxes"]:
            left, top, right, bottom = S.COMPOSITE_BOXES[f]
            assert np.array_equal(got[f, top:bottom, left:right], golden[1][f"composite.{i}.{f}"])


def test_steered_case_tells_numpy_means_from_exact_means(golden):
    rec = golden[0]["steered"]
    frames, rep, masks = S.steered_inputs(rec["k"])
    assert np.floor(rec["shift_sequential"]) != np.floor(rec["shift_exact"]) and rec["differing_bytes"] > 0
    got = S.composite(frames, rep, [S.STEERED_BOX], -1, True, masks)
    other = S.composite(frames, rep, [S.STEERED_BOX], -1, True, masks, means=S.exact_means)
    assert sha(got) == rec["sha256"] and sha(other) == rec["exact_route_sha256"] != rec["sha256"]
    assert int((got != other).sum()) == rec["differing_bytes"]


def test_fixture_is_small_and_complete(golden):
    assert os.path.getsize(S.FIXTURE_NPZ) + os.path.getsize(S.FIXTURE_JSON) <= \
        os.path.getsize(os.path.join(os.path.dirname(S.FIXTURE_NPZ), "facefix_builder.npz")) + \
        os.path.getsize(os.path.join(os.path.dirname(S.FIXTURE_NPZ), "facefix_builder.json"))
    meta = golden[0]
    assert meta["pillow"] and meta["numpy"]
    assert {m["key"] for m in meta["means"]} == set(S.MEANS_CASES) and len(meta["masks"]) == len(S.MASK_SIZES) * len(S.FEATHERS)
    assert {m["key"]: m for m in meta["means"]}["560_random"]["sequential_differs_from_exact"]
    assert meta["large"]["count"] > 65793 and meta["large"]["sequential_differs_from_exact"]


def _prototype(header, name):
    m = re.search(r"\b(int|int32_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vrgdg_hip.h"
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


def test_library_exports_the_symbols_and_the_abi_is_8(ffr):
    from comfyui_vrgamedevgirl_amd import _hip
    lib = _hip.load_library()
    assert lib.vrg_abi_version() == 8 == _hip.ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read(), flags=re.S)
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    for name in NEW_SYMBOLS:
        assert name in _hip.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        kind, proto = _prototype(header, name)
        res, args = _hip._SIGNATURES[name]
        assert res is (C.c_int32 if kind == "int32_t" else C.c_int) and len(proto) == len(args), name
        for text, ctype in zip(proto, args):
            assert ctype is (C.c_void_p if "*" in text else kinds[text.split()[0]]), (name, text)
    assert C.sizeof(_hip.PilResizeDesc) == 64 and _hip.PilResizeDesc.in_w.offset == 40
    assert C.sizeof(_hip.PilMaskDesc) == 40 and _hip.PilMaskDesc.span_offset.offset == 24
    assert C.sizeof(_hip.PilBoxDesc) == 40 and _hip.PilBoxDesc.mask_offset.offset == 24
    for struct, fields in ((_hip.PilResizeDesc, "vrg_pil_resize_desc"), (_hip.PilMaskDesc, "vrg_pil_mask_desc"), (_hip.PilBoxDesc, "vrg_pil_box_desc")):
        body = re.search(r"typedef struct " + fields + r" \{(.*?)\} " + fields + ";", header, flags=re.S).group(1)
        names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f[0] for f in struct._fields_], fields


def test_refusals_without_device(ffr):
    import torch
    from comfyui_vrgamedevgirl_amd import _hip
    lib = _hip.load_library()
    null, a, b, c, d, e, t, s = (C.c_void_p(v) for v in (0, 64, 128, 192, 256, 320, 384, 448))
    ok, bad, unsupported = _hip.VRG_OK, _hip.VRG_ERR_BAD_ARG, _hip.VRG_ERR_UNSUPPORTED

    def resize(src=a, desc=b, n=1, ch=3, tables=t, tmp=c, dst=d, largest=16):
        return lib.vrg_pil_resize_u8(src, 64, desc, n, ch, tables, 64, tmp, 64, dst, 64, largest, null)

    assert resize(n=0) == ok and resize(largest=0) == ok
    assert resize(ch=2) == resize(ch=4) == resize(ch=0) == bad              # C must be 1 or 3
    assert resize(src=null) == resize(desc=null) == resize(dst=null) == resize(tables=null) == resize(tmp=null) == bad
    assert resize(dst=a) == resize(tmp=a) == resize(tmp=d) == bad and resize(n=-1) == bad
    assert resize(largest=1 << 31) == unsupported

    def masks(spans=a, desc=b, n=1, mw=8, mh=8, scratch=c, out=d):
        return lib.vrg_pil_mask_u8(spans, 8, desc, n, mw, mh, scratch, out, 64, null)

    assert masks(n=0) == ok and masks(mw=0) == ok
    assert masks(spans=null) == masks(desc=null) == masks(scratch=null) == masks(out=null) == masks(scratch=d) == bad
    assert masks(n=-1) == masks(mw=-1) == bad and masks(mw=8193) == masks(mh=8193) == unsupported

    def means(o=a, r=b, m=c, desc=d, st=s, frames=1, h=8, w=8):
        return lib.vrg_np_masked_means_f32(o, r, 48, m, 16, desc, st, frames, h, w, 0.65, null)

    assert means(frames=0) == ok
    assert means(o=null) == means(r=null) == means(m=null) == means(desc=null) == means(st=null) == bad
    assert means(st=C.c_void_p(450)) == bad and means(frames=-1) == means(h=0) == means(w=0) == bad

    def paste(o=a, r=b, m=c, desc=d, st=s, out=e, frames=1, h=8, w=8):
        return lib.vrg_pil_paste_u8(o, r, 48, m, 16, desc, st, out, frames, h, w, null)

    assert paste(frames=0) == ok
    assert paste(o=null) == paste(r=null) == paste(m=null) == paste(desc=null) == paste(st=null) == paste(out=null) == bad
    assert paste(out=a) == paste(out=b) == bad and paste(frames=-1) == paste(h=0) == bad and paste(h=30000, w=30000) == unsupported
    assert lib.vrg_pil_lanczos_ksize(0, 4) == 0 and lib.vrg_pil_lanczos_ksize(300, 7) == 2 * 129 + 1
    assert lib.vrg_pil_lanczos_table(4, 4, null, a) == bad and lib.vrg_pil_lanczos_table(0, 4, a, b) == bad
    assert lib.vrg_pil_box_parameters(1.0, null) == bad and lib.vrg_pil_box_parameters(0.0, a) == bad

    # the Python surface refuses before anything is uploaded
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    crop = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="Invalid crop box for frame 1"):
        ffr.composite_frames(frames, [crop], [None, (3, 3, 3, 6)])         # an empty box
    with pytest.raises(ValueError):
        ffr.composite_frames(frames, [crop], [(0, 0, 9, 9), None])         # a box outside the frame
    with pytest.raises(ValueError):
        ffr.composite_frames(frames, [np.zeros((4, 4, 2), np.uint8)], [(0, 0, 4, 4), None])      # C = 2
    with pytest.raises(ValueError):
        ffr.composite_frames(frames, [np.zeros((4, 4), np.uint8)], [(0, 0, 4, 4), None])         # an L image as the repaired crop
    with pytest.raises(ValueError):
        ffr.composite_frames(frames, [crop], [(0, 0, 4, 4), None], feather=-1)                   # no masks
    with pytest.raises(ValueError):
        ffr.composite_frames(frames, [crop], [(0, 0, 4, 4), None], feather=-1, masks=[np.zeros((4, 4, 3), np.uint8)])    # not an L mask
    with pytest.raises(ValueError):
        ffr.composite_frames(frames, [crop], [(0, 0, 4, 4), None], feather=-1, masks=[np.zeros((0, 4), np.uint8)])       # an empty mask
    with pytest.raises(ValueError):
        ffr.composite_frames(frames, [crop], [(0, 0, 4, 4), None], feather=-1, masks=[])                                 # one mask per box
    with pytest.raises(ValueError):
        ffr.composite_frames(frames, [crop, crop, crop], [(0, 0, 4, 4), None])
    with pytest.raises(ValueError):
        ffr.pil_lanczos_resize([np.zeros((4, 4, 2), np.uint8)], (8, 8))
    with pytest.raises(ValueError):
        ffr.pil_lanczos_resize([crop], (0, 8))


def test_host_arithmetic_and_surface(ffr):
    assert list(inspect.signature(ffr.composite_frames).parameters) == ["originals_u8", "repaired", "crop_boxes", "feather", "color_match", "masks"]
    assert inspect.signature(ffr.composite_frames).parameters["feather"].default == 18
    assert list(inspect.signature(ffr.soft_face_mask).parameters) == ["size", "feather", "shrink"]
    assert ffr.NODE_CLASS_MAPPINGS == {}
    F = ffr.FaceBox
    # values worked out by hand from the reference's lines (:172-199): padding, the 32 px floor, the push back inside
    assert ffr.expanded_square_crop(F(100, 80, 20, 30, 1.0), 640, 360, 2.35) == (75, 60, 145, 130)
    assert ffr.expanded_square_crop(F(0, 0, 10, 10, 1.0), 640, 360, 2.0) == (0, 0, 32, 32)
    assert ffr.expanded_square_crop(F(630, 350, 10, 10, 1.0), 640, 360, 2.0) == (608, 328, 640, 360)
    assert ffr.expanded_square_crop(F(10, 10, 300, 300, 1.0), 200, 100, 2.0) == (0, 0, 200, 100)
    faces = [F(10, 10, 50, 50, 0.9), F(300, 160, 40, 40, 0.8)]
    assert ffr.choose_face(faces, 640, 360, "largest") is faces[0] and ffr.choose_face(faces, 640, 360, "center") is faces[1]
    assert ffr.choose_face([], 640, 360, "largest") is None

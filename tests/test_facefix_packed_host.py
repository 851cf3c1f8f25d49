"""The packed Builder Face Fix (frames on the host, only the boxes cross the bus) without a GPU: the plan's integers, the tile search of
csrc/vrg_facefix_packed_math.hpp compiled for the host (tests/host_math/facefix_packed_check.cpp), the body shared with the whole-frame
kernels under both addressings (csrc/vrg_facefix_body.hpp, tests/host_math/facefix_body_check.cpp), the refusals of vrg_ff_packed_check
and of the three launches, header <-> _hip._SIGNATURES <-> library, the public signatures, and packing / pasting with the device step
replaced by the numpy restatement of tests/facefix_builder_support.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import facefix_builder_support as FS
from conftest import PKG_DIR, ROOT

TILE = 256
NEW_SYMBOLS = ("vrg_ff_packed_check", "vrg_lanczos4_packed_u8", "vrg_ff_packed_resize_stats_u8", "vrg_ff_packed_composite_u8")
F, H, W, _ = FS.FRAMES_SHAPE
I64P = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def ff(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix, _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return VRGDG_FaceFix


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("facefix_packed_check")), "libfacefix_packed_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "facefix_packed_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out],
                   check=True)
    lib = C.CDLL(out)
    lib.hm_ffp_find.argtypes, lib.hm_ffp_find.restype = [I64P, C.c_int64, C.c_int64], C.c_int64
    lib.hm_ffp_tiles.argtypes, lib.hm_ffp_tiles.restype = [C.c_int32, C.c_int32], C.c_int64
    lib.hm_ffp_place.argtypes, lib.hm_ffp_place.restype = [C.c_int32, C.c_int32, C.c_int64, C.c_int64, I64P], C.c_int32
    return lib


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def _plans(ff):
    yield "interior_edges", FS.CROP_BOXES["interior_edges"], None
    for size, boxes in FS.CROP_BOXES["copy_and_down"].items():
        yield f"copy_and_down.{size}", boxes, None
    for key, (_, _, boxes, strengths, _, _) in FS.COMPOSITE_CASES.items():
        yield key, boxes, strengths


def test_plan_offsets_prefix_and_byte_counts(ff):
    seen_inactive = False
    for key, boxes, strengths in _plans(ff):
        plan = ff.packed_plan(F, H, W, boxes, strengths)
        active = [f for f, b in enumerate(boxes) if b is not None and (strengths is None or strengths[f] > 0)]
        assert plan.frames == active, key                                   # frames without a box or with strength <= 0 are absent
        seen_inactive |= any(b is not None for f, b in enumerate(boxes) if f not in active)
        with_box = [f for f, b in enumerate(boxes) if b is not None]
        assert plan.box_index == [with_box.index(f) for f in active] and plan.n_boxes == len(with_box), key
        sizes = []
        for f, (left, top, w, h) in zip(plan.frames, plan.boxes):
            assert (left, top, left + w, top + h) == tuple(boxes[f]), key
            sizes.append(w * h * 3)
        spans = sorted(zip(plan.offsets, sizes))                            # blocks do not overlap and leave no holes
        assert spans[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:])), key
        want = np.concatenate([[0], np.cumsum([-(-(w * h) // TILE) for _, _, w, h in plan.boxes])])
        assert plan.tile_prefix.dtype == np.int64 and np.array_equal(plan.tile_prefix, want) and plan.tiles == int(want[-1]), key
        assert plan.bytes_up == plan.bytes_down == sum(sizes) and plan.bytes_up < F * H * W * 3 == plan.frame_bytes, key
        assert plan.strengths == [1.0 if strengths is None else strengths[f] for f in active], key
    assert seen_inactive                                                    # the cases hold a strength-0 frame that has a box
    empty = ff.packed_plan(2, 8, 8, [None, None])
    assert empty.frames == [] and empty.bytes_up == 0 and list(empty.tile_prefix) == [0] and empty.tiles == 0
    assert ff.packed_plan(2, 8, 8, [(0, 0, 8, 8), None], [2.0, 1.0]).strengths == [1.0]      # clamped as composite_frames clamps


def test_plan_raises_what_boxes_raises(ff):
    with pytest.raises(ValueError, match="Invalid crop box for frame 1"):
        ff.packed_plan(2, 8, 8, [None, (3, 3, 3, 6)])
    with pytest.raises(ValueError, match="does not lie inside"):
        ff.packed_plan(2, 8, 8, [(0, 0, 9, 9), None])
    with pytest.raises(ValueError, match="one box"):
        ff.packed_plan(2, 8, 8, [None])
    with pytest.raises(ValueError, match="one value per frame"):
        ff.packed_plan(2, 8, 8, [None, None], [1.0])


# ---- the header on the host ---------------------------------------------------------------------------------------------------------------
def _table(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


# tile counts per record; tests/test_refbatch_host.py runs the same lists through the records' first_tile
SEARCH_COUNTS = ([1], [47], [1, 1, 1], [3, 1, 47, 2], [0, 0, 3, 1], [2, 0, 0, 5, 0, 1], [4, 2, 0, 0], [0, 5, 0], [0, 0, 1, 0, 0], [1] * 700, [1, 2] * 350)


@pytest.mark.parametrize("counts", SEARCH_COUNTS)
def test_search_finds_first_and_last_tile_of_every_record(hm, counts):
    """tile counts of 0 repeat a prefix value: in front, in the middle, at the end of the table"""
    prefix, n = _table(counts), len(counts)
    for rec, count in enumerate(counts):
        if count == 0:
            continue
        first = int(prefix[rec])
        for tile in {first, first + count - 1}:
            assert hm.hm_ffp_find(prefix, n, tile) == rec, (counts[:8], rec, tile)
    for tile in range(min(int(prefix[-1]), 64)):                             # every tile has the owner a linear walk finds
        assert hm.hm_ffp_find(prefix, n, tile) == max(i for i in range(n) if prefix[i] <= tile and counts[i] > 0)
    assert 0 <= hm.hm_ffp_find(prefix, n, int(prefix[-1]) + 5) < n           # a tile past the grid still names a record of the table


@pytest.mark.parametrize("w,h", ((1, 1), (1, 7), (7, 1), (16, 16), (17, 16), (257, 1), (300, 40), (3, 3), (2, 2)))
def test_tiles_cover_the_box_once(hm, w, h):
    tiles = hm.hm_ffp_tiles(w, h)
    assert tiles == -(-(w * h) // TILE)
    out, covered, first = np.zeros(2, dtype=np.int64), [], 11
    for tile in range(first, first + tiles):
        assert hm.hm_ffp_place(w, h, first, tile, out) == 1
        assert 1 <= out[1] <= TILE
        covered.extend(range(int(out[0]), int(out[0] + out[1])))
    assert covered == list(range(w * h))
    assert hm.hm_ffp_place(w, h, first, first - 1, out) == 0 and hm.hm_ffp_place(w, h, first, first + tiles, out) == 0
    for bad in ((0, 5), (5, 0), (-1, 5), (46341, 46341)):                    # no box, or 2^31 bytes and more: no tiles
        assert hm.hm_ffp_tiles(*bad) == 0 and hm.hm_ffp_place(*bad, 0, 0, out) == 0


# ---- the shared body under both addressings --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def body(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("facefix_body_check")), "libfacefix_body_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "facefix_body_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out],
                   check=True)
    lib = C.CDLL(out)
    lib.hm_ffb_box.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_float,
                               C.c_int32, C.c_void_p, C.c_void_p, I64P, C.c_void_p]
    lib.hm_ffb_box.restype = None
    return lib


BODY_FRAME = (48, 64, 3)
BODY_ENHANCED = (20, 24, 3)
BODY_CROP = 12
BODY_BOXES = {"17x16_two_tiles": (5, 7, 17, 16), "1x1": (30, 20, 1, 1), "16x16_corner": (48, 32, 16, 16), "23x19": (11, 3, 23, 19)}      # left, top, w, h


def _body_run(lib, base, offset, pitch, w, h, enhanced, mask, cm, strength):
    """the box whose first byte is base[offset:], rows `pitch` pixels apart -> (crop, resized, sums, out)"""
    crop = np.zeros((BODY_CROP, BODY_CROP, 3), dtype=np.uint8)
    resized, out, sums = np.zeros((h, w, 3), dtype=np.uint8), np.zeros((h, w, 3), dtype=np.uint8), np.zeros(7, dtype=np.int64)
    lib.hm_ffb_box(base.ctypes.data + offset, pitch, w, h, enhanced.ctypes.data, enhanced.shape[0], enhanced.shape[1], mask.ctypes.data, cm, strength,
                   BODY_CROP, crop.ctypes.data, resized.ctypes.data, sums, out.ctypes.data)
    return crop, resized, sums, out


@pytest.mark.parametrize("cm", (0.0, 0.65))
@pytest.mark.parametrize("feather", (0, 3))
@pytest.mark.parametrize("name", sorted(BODY_BOXES))
def test_shared_body_agrees_under_both_addressings(body, name, feather, cm):
    """csrc/vrg_facefix_body.hpp on the same pixels as k_lanczos4_boxes / k_ff_resize_stats / FfMover address them (a box inside a frame,
    pitch = the frame's width) and as the packed kernels do (a dense block, pitch = box_w)"""
    left, top, w, h = BODY_BOXES[name]
    H, W, _ = BODY_FRAME
    assert left + w <= W and top + h <= H
    rng = np.random.Generator(np.random.PCG64(77))
    frame = rng.integers(0, 256, size=BODY_FRAME, dtype=np.uint8)
    enhanced = rng.integers(0, 256, size=BODY_ENHANCED, dtype=np.uint8)
    dense = np.ascontiguousarray(frame[top:top + h, left:left + w])
    mask = np.ascontiguousarray(FS.soft_ellipse_mask(w, h, feather), dtype=np.float32)
    strength = 0.75
    in_frame = _body_run(body, frame, (top * W + left) * 3, W, w, h, enhanced, mask, cm, strength)
    packed = _body_run(body, dense, 0, w, w, h, enhanced, mask, cm, strength)
    for what, a, b in zip(("crop", "resized", "sums", "composite"), in_frame, packed):
        assert np.array_equal(a, b), (name, feather, cm, what)
    crop, resized, sums, out = packed
    selected = mask > np.float32(0.35)
    want = [int(selected.sum())] + [int(img[..., c][selected].astype(np.int64).sum()) for img in (resized, dense) for c in range(3)]
    assert sums.tolist() == (want if cm > 0 else [0] * 7), (name, feather, cm)         # colour match off: nothing is measured
    assert want[0] > 0
    # ... and the bytes are those of the numpy restatement of the route
    assert np.array_equal(crop, FS.crops(frame[None], [(left, top, left + w, top + h)], BODY_CROP)[0])
    assert np.array_equal(resized, np.asarray(FS.LS.restated(enhanced[None], w, h))[0])
    face, _ = FS.color_match(resized, dense, mask, cm)
    assert np.array_equal(out, FS.blend(dense, face, mask, strength))
    assert not np.array_equal(out, dense)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def _records(ff, rows):
    desc = np.zeros(len(rows), dtype=ff._PACKED_DESC)
    for i, row in enumerate(rows):
        desc[i] = row
    return desc


def test_packed_check_refusals(ff):
    from comfyui_vrgamedevgirl_amd import _hip
    lib = _hip.load_library()
    ok, bad = _hip.VRG_OK, _hip.VRG_ERR_BAD_ARG
    # two boxes: 5 x 4 at 0 and 17 x 16 (two tiles) behind it; masks 20 + 272 floats, taps 9 + 33 records, one repaired frame each
    good = [(0, 0, 5, 4, 0, 1.0, 0, 0, 0), (60, 60, 17, 16, 1, 0.5, 20, 9, 60)]
    total = 60 + 17 * 16 * 3
    prefix = np.array([0, 1, 3], dtype=np.int64)

    def check(rows=good, table=prefix, n=None, src=total, out=total, enh=2, floats=292, taps=42, cap=total, oh=0, ow=0):
        desc = _records(ff, rows)
        return lib.vrg_ff_packed_check(C.c_void_p(desc.ctypes.data), len(rows) if n is None else n,
                                       None if table is None else C.c_void_p(table.ctypes.data), src, out, enh, floats, taps, cap, oh, ow)

    def with_field(index, name, value):
        desc = _records(ff, good)
        desc[index][name] = value
        return [tuple(r) for r in desc.tolist()]

    assert check() == ok and check(n=0) == ok and check(rows=[], n=0, table=None) == ok
    assert check(src=total - 1) == bad and check(out=total - 1) == bad and check(cap=total - 1) == bad      # a block ends past its buffer
    assert check(floats=291) == bad and check(taps=41) == bad and check(enh=1) == bad
    for name in ("src_offset", "dst_offset", "mask_offset", "taps_offset", "bytes_offset"):
        assert check(rows=with_field(0, name, -1)) == bad, name
        assert check(rows=with_field(1, name, 1 << 40)) == bad, name
    assert check(rows=with_field(0, "box_w", 0)) == bad and check(rows=with_field(0, "box_h", -3)) == bad
    huge, room = [(0, 0, 46341, 46341, 0, 1.0, 0, 0, 0)], 1 << 40            # 2^31 bytes and more, although every buffer would hold it
    table = np.array([0, -(-(46341 * 46341) // TILE)], dtype=np.int64)
    assert check(rows=huge, table=table, src=room, out=room, floats=room, taps=room, cap=room) == bad
    assert check(rows=[(0, 0, 20000, 20000, 0, 1.0, 0, 0, 0)], table=np.array([0, 1562500], dtype=np.int64), src=room, out=room, floats=room,
                 taps=room, cap=room) == ok
    assert check(rows=with_field(1, "enhanced_index", -1)) == check(rows=with_field(1, "enhanced_index", 2)) == bad
    assert check(rows=with_field(0, "strength", 0.0)) == check(rows=with_field(0, "strength", float("nan"))) == bad
    for table in ([0, 1, 2], [0, 2, 3], [1, 2, 4], [0, 1, 4], [0, 0, 3]):    # not the running sum of the records' tiles
        assert check(table=np.array(table, dtype=np.int64)) == bad, table
    assert check(table=None) == bad                                          # the composite's records come with their table
    assert check(n=-1) == check(src=-1) == check(out=-1) == check(enh=-1) == check(floats=-1) == check(taps=-1) == check(cap=-1) == bad
    assert check(oh=-1) == check(oh=8, ow=0) == check(oh=0, ow=8) == bad
    null = lib.vrg_ff_packed_check(None, 1, C.c_void_p(prefix.ctypes.data), 8, 8, 1, 8, 8, 8, 0, 0)
    assert null == bad
    # a crop's records: src and out_w + out_h taps; no table, and the composite's fields are not read
    crop = [(0, -7, 5, 4, -1, 0.0, -1, 0, -1), (60, -7, 17, 16, -1, 0.0, -1, 16, -1)]
    assert check(rows=crop, table=None, out=0, enh=0, floats=0, cap=0, taps=32, oh=8, ow=8) == ok
    assert check(rows=crop, table=None, out=0, enh=0, floats=0, cap=0, taps=31, oh=8, ow=8) == bad
    assert check(rows=crop, table=None, src=total - 1, taps=32, oh=8, ow=8) == bad
    assert check(rows=crop, table=np.array([0, 1, 2], dtype=np.int64), taps=32, oh=8, ow=8) == bad      # a table that is given is checked


def test_launch_refusals_without_device(ff):
    from comfyui_vrgamedevgirl_amd import _hip
    lib = _hip.load_library()
    null, a, b, c, d, e, t, s, p = (C.c_void_p(v) for v in (0, 64, 128, 192, 256, 320, 384, 448, 512))
    ok, bad, unsupported = _hip.VRG_OK, _hip.VRG_ERR_BAD_ARG, _hip.VRG_ERR_UNSUPPORTED

    def crop(src=a, src_bytes=48, desc=c, n=1, out=b, oh=4, ow=4, taps=t, n_taps=8):
        return lib.vrg_lanczos4_packed_u8(src, src_bytes, desc, n, out, oh, ow, taps, n_taps, null)

    assert crop(n=0) == ok                                                   # no records: no launch
    assert crop(src=null) == crop(out=null) == crop(desc=null) == crop(taps=null) == bad
    assert crop(out=a) == bad and crop(taps=C.c_void_p(386)) == bad
    assert crop(n=-1) == crop(src_bytes=-1) == crop(n_taps=-1) == crop(oh=0) == crop(ow=0) == bad
    assert crop(oh=40000, ow=40000) == unsupported and crop(n=1 << 40) == unsupported

    def stats(src=a, enh=b, mk=c, desc=d, pre=p, taps=t, face=e, st=s, n=1, tiles=1, n_enh=1, eh=4, ew=4, cm=0.5):
        return lib.vrg_ff_packed_resize_stats_u8(src, 48, enh, n_enh, eh, ew, mk, 16, desc, pre, n, tiles, taps, 8, face, 48, st, cm, null)

    assert stats(n=0) == ok
    assert stats(src=null) == stats(enh=null) == stats(mk=null) == stats(desc=null) == stats(pre=null) == stats(taps=null) == bad
    assert stats(face=null) == stats(st=null) == bad
    assert stats(face=a) == stats(face=b) == bad                             # the packed bytes alias an input
    assert stats(st=C.c_void_p(452)) == bad and stats(pre=C.c_void_p(516)) == bad         # 64-bit words
    assert stats(n=-1) == stats(tiles=-1) == stats(n_enh=-1) == stats(eh=0) == stats(ew=0) == bad
    assert stats(tiles=1 << 31) == unsupported and stats(eh=30000, ew=30000) == unsupported

    def comp(src=a, mk=c, desc=d, pre=p, face=e, st=s, o=b, n=1, tiles=1, out_bytes=48):
        return lib.vrg_ff_packed_composite_u8(src, 48, mk, 16, desc, pre, n, tiles, face, 48, st, o, out_bytes, null)

    assert comp(n=0) == ok
    assert comp(src=null) == comp(mk=null) == comp(desc=null) == comp(pre=null) == comp(face=null) == comp(st=null) == comp(o=null) == bad
    assert comp(o=a) == bad and comp(o=e) == bad                             # out aliases an input
    assert comp(n=-1) == comp(tiles=-1) == comp(out_bytes=-1) == bad
    assert comp(tiles=1 << 31) == unsupported
    assert comp(tiles=0) == ok                                               # records without tiles: nothing to launch


def _prototype(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vrgdg_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_signatures_and_library_agree(ff):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    lib = _hip.load_library()
    assert lib.vrg_abi_version() == 8 == _hip.ABI_VERSION                    # additive: the version stays
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read(), flags=re.S)
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    for name in NEW_SYMBOLS:
        assert name in _hip.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        proto = _prototype(header, name)
        res, args = _hip._SIGNATURES[name]
        assert res is C.c_int and len(proto) == len(args), name
        for text, ctype in zip(proto, args):
            assert ctype is (C.c_void_p if "*" in text else kinds[text.split()[0]]), (name, text)
    rec = _hip.FaceFixPackedDesc
    assert C.sizeof(rec) == 56 and C.sizeof(rec) % 8 == 0                    # the int64 table rides behind the records
    assert rec.src_offset.offset == 0 and rec.dst_offset.offset == 8 and rec.strength.offset == 28 and rec.mask_offset.offset == 32
    assert issubclass(rec, _hip.Record) and rec.c_name == "vrg_ff_packed_desc"
    assert int(re.search(r"#define\s+VRG_FF_PACKED_TILE\s+(\d+)", header).group(1)) == _hip.FACEFIX_PACKED_TILE == TILE
    assert "vrg_facefix_packed.hip" in build_ext.SOURCES and "vrg_facefix_packed_math.hpp" in build_ext.HEADERS
    source = open(os.path.join(PKG_DIR, "csrc", "vrg_facefix_packed.hip")).read()
    assert "blockIdx.y" not in source and "blockIdx.z" not in source and "launch_chunks" not in source


# ---- the Python surface -------------------------------------------------------------------------------------------------------------------
def test_public_signatures(ff):
    def names(fn):
        return [(n, p.kind) for n, p in inspect.signature(fn).parameters.items()]

    POS, KW = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    assert names(ff.packed_plan) == [(n, POS) for n in ("frames", "height", "width", "crop_boxes", "strengths")]
    assert inspect.signature(ff.packed_plan).parameters["strengths"].default is None
    assert names(ff.crop_frames_packed) == [(n, POS) for n in ("frames_u8", "crop_boxes", "enhance_size")]
    composite = [(n, POS) for n in ("originals_u8", "enhanced_u8", "crop_boxes", "strengths", "feather", "color_match")]
    assert names(ff.composite_boxes_packed) == composite
    assert names(ff.composite_frames_packed) == composite + [("inplace", KW)]
    assert inspect.signature(ff.composite_frames_packed).parameters["inplace"].default is False
    assert names(ff.last_transfer) == [] and set(ff.last_transfer()) == {"bytes_up", "bytes_down", "enhanced_up", "tables_up"}
    # the functions the routes had before are untouched
    assert list(inspect.signature(ff.crop_frames).parameters) == ["frames_u8", "crop_boxes", "enhance_size"]
    assert list(inspect.signature(ff.composite_frames).parameters) == ["originals_u8", "enhanced_u8", "crop_boxes", "strengths", "feather",
                                                                       "color_match"]
    assert ff.NODE_CLASS_MAPPINGS == {}


def test_gpu_resident_frames_are_refused_by_name(ff):
    class Decoded:                                                           # what DecodedFrames looks like: a batch behind .u8
        u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)

    frames = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(TypeError, match="crop_frames"):
        ff.crop_frames_packed(Decoded(), [(0, 0, 4, 4)], 8)
    with pytest.raises(TypeError, match="composite_frames"):
        ff.composite_boxes_packed(Decoded(), frames, [(0, 0, 4, 4)], 1.0)
    with pytest.raises(TypeError, match="composite_frames"):
        ff.composite_frames_packed(Decoded(), frames, [(0, 0, 4, 4)], 1.0)
    with pytest.raises(ValueError, match="Invalid crop box for frame 0"):
        ff.crop_frames_packed(frames, [(5, 2, 4, 6)], 16)
    with pytest.raises(ValueError, match="Invalid crop box for frame 0"):
        ff.composite_frames_packed(frames, frames, [(5, 2, 4, 6)], 1.0)
    with pytest.raises(ValueError):
        ff.crop_frames_packed(frames.float(), [None], 16)
    with pytest.raises(ValueError):
        ff.crop_frames_packed(frames, [(0, 0, 4, 4)], 0)


# ---- packing and pasting, the device step replaced by the restatement ----------------------------------------------------------------------
def test_pack_gathers_every_active_box(ff):
    frames = FS.make_frames("random", FS.FRAMES_SHAPE, FS.FRAMES_SEED)
    _, _, boxes, strengths, _, _ = FS.COMPOSITE_CASES["f0_cm0_48x40"]
    plan = ff.packed_plan(F, H, W, boxes, strengths)
    stage = np.full(plan.bytes_up + 9, 0xA5, dtype=np.uint8)
    ff._pack_boxes(list(frames), plan, stage)
    for f, (left, top, w, h), offset in zip(plan.frames, plan.boxes, plan.offsets):
        assert np.array_equal(stage[offset:offset + w * h * 3].reshape(h, w, 3), frames[f, top:top + h, left:left + w])
    assert (stage[plan.bytes_up:] == 0xA5).all()
    assert any(offset % 16 for offset in plan.offsets)                       # blocks start off the 16-byte grid


@pytest.fixture
def restated_device_step(ff, monkeypatch):
    """composite_boxes_packed computed by the numpy restatement: what the device step must return, with no device"""
    def boxes_from_restatement(originals_u8, enhanced_u8, crop_boxes, strengths, feather=18, color_match=0.65):
        originals = np.stack([np.asarray(f) for f in (originals_u8.numpy() if isinstance(originals_u8, torch.Tensor) else originals_u8)])
        enhanced = np.stack([np.asarray(e) for e in (enhanced_u8.numpy() if isinstance(enhanced_u8, torch.Tensor) else enhanced_u8)])
        whole = FS.composite(originals, enhanced, crop_boxes, strengths, feather, color_match)
        plan = ff.packed_plan(*originals.shape[:3], crop_boxes, strengths)
        return [whole[f, top:top + h, left:left + w].copy() for f, (left, top, w, h) in zip(plan.frames, plan.boxes)]

    monkeypatch.setattr(ff, "composite_boxes_packed", boxes_from_restatement)


@pytest.mark.parametrize("form", ("list", "tensor"))
def test_paste_into_a_copy_or_in_place(ff, restated_device_step, form):
    key = "f1_cm1_dark_64"
    originals, enhanced, boxes, strengths, feather, cm = FS.case_inputs(key)
    want = FS.composite(originals, enhanced, boxes, strengths, feather, cm)
    assert not np.array_equal(want, originals)

    def given():
        return [f.copy() for f in originals] if form == "list" else torch.from_numpy(originals.copy())

    def as_array(x):
        return np.stack(x) if isinstance(x, list) else x.numpy()

    mine = given()
    got = ff.composite_frames_packed(mine, list(enhanced), boxes, strengths, feather, cm)
    assert type(got) is type(mine) and got is not mine
    assert np.array_equal(as_array(got), want)
    assert np.array_equal(as_array(mine), originals)                        # inplace=False: the originals' bytes are untouched
    if form == "list":
        assert all(not np.shares_memory(g, m) for g, m in zip(got, mine))
    mine = given()
    got = ff.composite_frames_packed(mine, list(enhanced), boxes, strengths, feather, cm, inplace=True)
    assert got is mine and np.array_equal(as_array(mine), want)
    outside = np.ones(originals.shape[:3], dtype=bool)                      # inplace=True: only bytes inside active boxes may change
    for f, box in enumerate(boxes):
        if box is not None and strengths[f] > 0:
            outside[f, box[1]:box[3], box[0]:box[2]] = False
    assert np.array_equal(as_array(mine)[outside], originals[outside])


def test_paste_into_strided_frames(ff, restated_device_step):
    """frames that are views (a decoder's padded rows): copied by value, pasted in place through the view"""
    originals, enhanced, boxes, strengths, feather, cm = FS.case_inputs("f0_cm0_48x40")
    want = FS.composite(originals, enhanced, boxes, strengths, feather, cm)
    padded = np.zeros((F, H, W + 6, 3), dtype=np.uint8)
    padded[:, :, :W] = originals
    views = [padded[f, :, :W] for f in range(F)]
    assert not views[0].flags.c_contiguous
    got = ff.composite_frames_packed(views, list(enhanced), boxes, strengths, feather, cm)
    assert np.array_equal(np.stack(got), want) and np.array_equal(padded[:, :, :W], originals)
    ff.composite_frames_packed(views, list(enhanced), boxes, strengths, feather, cm, inplace=True)
    assert np.array_equal(padded[:, :, :W], want) and not padded[:, :, W:].any()

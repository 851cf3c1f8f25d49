"""The packed far-face repair composite (frames on the host, only the boxes cross the bus) without a GPU: the plan's integers, the
verdicts of vrg_pil_packed_check, the refusals of the two launches, header <-> _hip, the calls that move nothing, and the body shared
with the whole-frame kernels (csrc/vrg_farface_body.hpp) compiled with g++ (tests/host_math/farface_packed_check.cpp) against the numpy
restatement of tests/far_face_support.py, byte for byte and bit for bit."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import far_face_support as FS
from conftest import PKG_DIR, ROOT

U8P, U32P, I64P = FS.U8P, FS.U32P, FS.I64P
F, H, W = len(FS.COMPOSITE_BOXES), FS.FRAME_H, FS.FRAME_W


@pytest.fixture(scope="module")
def fr(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext, far_face_repair
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return far_face_repair


@pytest.fixture(scope="module")
def hip(fr):
    from comfyui_vrgamedevgirl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("farface_packed_check")), "libfarface_packed_check.so")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host_math", "farface_packed_check.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_pilp_means.argtypes = [U8P, U8P, U8P, C.c_int64, U32P]
    lib.hm_pil_means_framed.argtypes = [C.c_void_p, C.c_int32, C.c_int32, U8P, U8P, C.c_int64, U32P]
    lib.hm_pilp_paste.argtypes = [U8P, U8P, U8P, C.c_int64, C.c_int32, U32P, U8P]
    lib.hm_pilp_tiles.argtypes, lib.hm_pilp_tiles.restype = [C.c_int32, C.c_int32], C.c_int64
    lib.hm_pilp_place.argtypes, lib.hm_pilp_place.restype = [C.c_int32, C.c_int32, C.c_int64, C.c_int64, I64P], C.c_int32
    return lib


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def test_plan_offsets_prefix_and_byte_counts(fr, hip):
    tile = hip.PIL_PACKED_TILE
    plan = fr.packed_plan(F, H, W, FS.COMPOSITE_BOXES)
    assert plan.frames == [0, 1, 2, 3]
    sizes = []
    for f, (left, top, w, h) in zip(plan.frames, plan.boxes):
        assert (left, top, left + w, top + h) == tuple(FS.COMPOSITE_BOXES[f])
        sizes.append(w * h * 3)
    assert plan.offsets == [int(v) for v in np.cumsum([0] + sizes[:-1])]        # back to back, no holes
    want = np.concatenate([[0], np.cumsum([-(-(w * h) // tile) for _, _, w, h in plan.boxes])])
    assert plan.tile_prefix.dtype == np.int64 and np.array_equal(plan.tile_prefix, want) and plan.tiles == int(want[-1])
    assert plan.bytes_up == plan.bytes_down == sum(sizes) and plan.frame_bytes == F * H * W * 3
    small = fr.packed_plan(3, 1080, 1920, [(100, 100, 228, 228), None, (0, 0, 32, 32)])
    assert small.frames == [0, 2] and small.bytes_up == (128 * 128 + 32 * 32) * 3 < small.frame_bytes // 300
    empty = fr.packed_plan(2, 8, 8, [None, None])
    assert empty.frames == [] and empty.boxes == [] and empty.offsets == [] and empty.bytes_up == 0
    assert list(empty.tile_prefix) == [0] and empty.tiles == 0 and empty.frame_bytes == 2 * 8 * 8 * 3


def test_plan_raises_what_composite_frames_raises(fr):
    with pytest.raises(ValueError, match="Invalid crop box for frame 1"):
        fr.packed_plan(2, 8, 8, [None, (3, 3, 3, 6)])
    with pytest.raises(ValueError, match="does not lie inside"):
        fr.packed_plan(2, 8, 8, [(0, 0, 9, 9), None])
    with pytest.raises(ValueError, match="one box"):
        fr.packed_plan(2, 8, 8, [None])


def test_header_record_and_tile(hip):
    header = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    assert int(re.search(r"#define\s+VRG_PIL_PACKED_TILE\s+(\d+)", header).group(1)) == hip.PIL_PACKED_TILE
    assert C.sizeof(hip.PilPackedDesc) == 48                               # an int64 prefix may trail the records in one upload
    assert [n for n, _ in hip.PilPackedDesc._fields_] == ["src_offset", "dst_offset", "box_w", "box_h", "color_match", "reserved", "mask_offset",
                                                           "rep_offset"]
    for name in ("vrg_pil_packed_check", "vrg_np_packed_masked_means_f32", "vrg_pil_packed_paste_u8"):
        assert name in hip.EXPORTED_SYMBOLS
    assert hip.host_library().vrg_abi_version() == 8


# ---- vrg_pil_packed_check ------------------------------------------------------------------------------------------------------------------
BOXES = [(5, 7), (16, 16), (1, 1), (300, 2)]                               # (w, h): 35, 256, 1 and 600 pixels


def _table(hip):
    desc = np.zeros(len(BOXES), dtype=hip.record_dtype(hip.PilPackedDesc))
    at = at_mask = 0
    for i, (w, h) in enumerate(BOXES):
        desc[i] = (at, at, w, h, 1, 0, at_mask, at)
        at, at_mask = at + w * h * 3, at_mask + w * h
    prefix = np.concatenate([[0], np.cumsum([-(-(w * h) // hip.PIL_PACKED_TILE) for w, h in BOXES])]).astype(np.int64)
    return desc, prefix, at, at_mask


def _verdict(hip, desc, prefix, total, mask_total, n=None):
    return hip.host_library().vrg_pil_packed_check(C.c_void_p(desc.ctypes.data), len(desc) if n is None else n, C.c_void_p(prefix.ctypes.data),
                                                   total, total, mask_total, total)


def test_check_verdicts(hip):
    desc, prefix, total, mask_total = _table(hip)
    assert list(prefix) == [0, 1, 2, 3, 6]
    assert _verdict(hip, desc, prefix, total, mask_total) == 0
    assert _verdict(hip, desc, prefix, total, mask_total, n=0) == 0
    assert hip.host_library().vrg_pil_packed_check(None, 0, None, 0, 0, 0, 0) == 0
    assert hip.host_library().vrg_pil_packed_check(None, 1, None, 8, 8, 8, 8) == 1
    assert hip.host_library().vrg_pil_packed_check(C.c_void_p(desc.ctypes.data), 1, C.c_void_p(prefix.ctypes.data), -1, 8, 8, 8) == 1
    spoilers = [("src_offset", total), ("src_offset", -1), ("src_offset", total - 5), ("rep_offset", total + 1), ("rep_offset", total - 5),
                ("mask_offset", -1), ("mask_offset", mask_total), ("dst_offset", total - 5), ("box_w", 0), ("box_h", -3)]
    everything = desc.copy()
    for k, (field, value) in enumerate(spoilers):
        bad = desc.copy()
        bad[k % 2][field] = value
        assert _verdict(hip, bad, prefix, total, mask_total) == 1, (field, value)
        if field in ("src_offset", "rep_offset", "mask_offset", "box_w"):
            everything[k % 2][field] = value
    for i in range(len(prefix)):                                            # a wrong prefix entry, anywhere
        wrong = prefix.copy()
        wrong[i] += 1
        assert _verdict(hip, desc, wrong, total, mask_total) == 1, i
    wrong = prefix.copy()
    wrong[2] += 1
    assert _verdict(hip, everything, wrong, total, mask_total) == 1         # all together
    assert _verdict(hip, desc, prefix, total - 1, mask_total) == 1          # the last block leaves a buffer one byte short
    assert _verdict(hip, desc, prefix, total, mask_total - 1) == 1
    huge = desc[:1].copy()
    huge[0]["box_w"], huge[0]["box_h"] = 40000, 40000                       # 2^31 bytes and more: no box
    assert _verdict(hip, huge, np.array([0, 0], np.int64), 1 << 40, 1 << 40) == 1


def test_launch_refusals_without_a_device(hip):
    lib = hip.host_library()
    a, b, c, d, e, f, g = (C.c_void_p(4096 * k) for k in range(1, 8))      # never dereferenced: the call is refused or has nothing to do
    paste = lib.vrg_pil_packed_paste_u8
    assert paste(a, 8, b, 8, c, 8, d, e, 0, 0, f, g, 8, None) == 0         # no record
    assert paste(a, 8, b, 8, c, 8, d, e, 1, 0, f, g, 8, None) == 0         # no tile
    assert paste(a, 8, b, 8, c, 8, d, e, 1, (1 << 31) - 1 + 1, f, g, 8, None) == 2
    assert paste(a, 8, b, 8, c, 8, d, e, 1, 1, f, a, 8, None) == 1         # out == src
    assert paste(a, 8, b, 8, c, 8, d, e, 1, 1, f, b, 8, None) == 1         # out == repaired
    assert paste(None, 8, b, 8, c, 8, d, e, 1, 1, f, g, 8, None) == 1
    assert paste(a, 8, b, 8, c, 8, d, C.c_void_p(4097), 1, 1, f, g, 8, None) == 1      # the prefix is int64
    assert paste(a, 8, b, 8, c, 8, d, e, 1, 1, C.c_void_p(4098), g, 8, None) == 1      # the stats are uint32
    assert paste(a, 8, b, 8, c, 8, d, e, 1, -1, f, g, 8, None) == 1
    assert paste(a, -8, b, 8, c, 8, d, e, 1, 1, f, g, 8, None) == 1
    means = lib.vrg_np_packed_masked_means_f32
    assert means(a, 8, b, 8, c, 8, d, f, 0, 0.65, None) == 0
    assert means(a, 8, b, 8, c, 8, d, None, 1, 0.65, None) == 1
    assert means(a, 8, b, 8, c, 8, d, C.c_void_p(4098), 1, 0.65, None) == 1
    assert means(a, 8, b, 8, c, -1, d, f, 1, 0.65, None) == 1
    assert means(a, 8, b, 8, c, 8, d, f, 1 << 31, 0.65, None) == 2


# ---- the shared body on the host ---------------------------------------------------------------------------------------------------------------
def _body_cases():
    """(name, original [h, w, 3], repaired [h, w, 3], mask [h, w]): the 15 / 16 boundary, one chunk of the means, a chunk plus one pixel"""
    for key in ("sel15", "sel16"):
        yield (key,) + FS.means_inputs(key)
    for name, (w, h) in (("2048", (64, 32)), ("2049", (683, 3))):
        yield name, FS.random_image(9101, h, w), FS.random_image(9102, h, w, 3, 0, 120), FS.random_image(9103, h, w, 0, 40, 256)
        yield name + "_all", FS.random_image(9104, h, w), FS.random_image(9105, h, w), np.full((h, w), 255, np.uint8)


def _want_stats(original, repaired, mask):
    _, count, om, rm, shift = FS.color_match(original, repaired, mask)
    return np.array([count] + FS.bits(om) + FS.bits(rm) + FS.bits(shift) + [int(count >= 16), 0], dtype=np.uint32)


def test_shared_body_equals_the_restatement_on_dense_blocks_and_inside_a_frame(hm):
    seen = set()
    for name, original, repaired, mask in _body_cases():
        h, w = mask.shape
        want = _want_stats(original, repaired, mask)
        seen.add((int(want[0]), h * w))
        got = np.zeros(12, np.uint32)
        hm.hm_pilp_means(np.ascontiguousarray(original), np.ascontiguousarray(repaired), np.ascontiguousarray(mask), h * w, got)
        assert np.array_equal(got, want), name
        frame = FS.random_image(9200, h + 5, w + 9)                         # the same box at (left 4, top 3) of a wider frame
        frame[3:3 + h, 4:4 + w] = original
        framed = np.zeros(12, np.uint32)
        hm.hm_pil_means_framed(frame.ctypes.data + (3 * (w + 9) + 4) * 3, w, w + 9, np.ascontiguousarray(repaired), np.ascontiguousarray(mask),
                               h * w, framed)
        assert np.array_equal(framed, want), name
        for color_match in (0, 1):
            out = np.zeros_like(original)
            hm.hm_pilp_paste(np.ascontiguousarray(original), np.ascontiguousarray(repaired), np.ascontiguousarray(mask), h * w, color_match, got,
                             out)
            face = FS.color_match(original, repaired, mask)[0] if color_match else repaired
            assert np.array_equal(out, FS.paste(original, face, mask)), (name, color_match)
    assert {(15, 36), (16, 36), (2048, 2048), (2049, 2049)} <= seen         # the cases are what their names say


def test_tile_placement(hm, hip):
    tile = hip.PIL_PACKED_TILE
    out = np.zeros(2, np.int64)
    for w, h in ((1, 1), (tile, 1), (tile + 1, 1), (64, 32), (683, 3), (700, 40)):
        px = w * h
        tiles = -(-px // tile)
        assert hm.hm_pilp_tiles(w, h) == tiles
        for first in (0, 7):
            for k in range(tiles):
                assert hm.hm_pilp_place(w, h, first, first + k, out) == 1 and list(out) == [k * tile, min(tile, px - k * tile)], (w, h, k)
            assert hm.hm_pilp_place(w, h, first, first + tiles, out) == 0 and hm.hm_pilp_place(w, h, first, first - 1, out) == 0
    assert hm.hm_pilp_tiles(0, 5) == 0 and hm.hm_pilp_tiles(5, -1) == 0 and hm.hm_pilp_tiles(40000, 40000) == 0
    assert hm.hm_pilp_place(0, 5, 0, 0, out) == 0


# ---- calls that move nothing ------------------------------------------------------------------------------------------------------------------
def test_no_box_moves_nothing_and_opens_no_device(fr, monkeypatch):
    monkeypatch.setattr(fr, "compute_device", lambda: pytest.fail("a call without a box asked for a device"))
    frames = torch.from_numpy(FS.random_image(9300, 12, 10)[None].repeat(3, axis=0).copy())
    kept = frames.clone()
    assert fr.composite_boxes_packed(frames, [], [None] * 3) == []
    assert fr.last_transfer() == {"bytes_up": 0, "bytes_down": 0, "repaired_up": 0, "tables_up": 0}
    out = fr.composite_frames_packed(frames, [None] * 3, [None] * 3, 18, True)
    assert isinstance(out, torch.Tensor) and out.data_ptr() != frames.data_ptr() and torch.equal(out, kept) and torch.equal(frames, kept)
    listed = [f.numpy() for f in frames]
    back = fr.composite_frames_packed(listed, [], [None] * 3, inplace=True)
    assert back is listed and all(np.array_equal(a, b.numpy()) for a, b in zip(back, kept))
    copies = fr.composite_frames_packed(listed, [], [None] * 3)
    assert isinstance(copies, list) and all(c is not a and np.array_equal(c, a) for c, a in zip(copies, listed))
    assert fr.last_transfer() == {"bytes_up": 0, "bytes_down": 0, "repaired_up": 0, "tables_up": 0}


def test_the_packed_route_refuses_decoded_frames_by_name(fr):
    decoded = types.SimpleNamespace(u8=torch.zeros((1, 8, 8, 3), dtype=torch.uint8))       # what DecodedFrames shows: its batch as .u8
    for call in (fr.composite_boxes_packed, fr.composite_frames_packed):
        with pytest.raises(TypeError, match="use composite_frames"):
            call(decoded, [], [None])

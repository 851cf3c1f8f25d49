"""The packed Builder Face Fix on the GPU (VRGDG_FaceFix.crop_frames_packed / composite_boxes_packed / composite_frames_packed,
csrc/vrg_facefix_packed.hip): frames on the host, only the boxes cross the bus.  Every result equals, byte for byte, the numpy restatement
of tests/facefix_builder_support.py and the recorded bytes of tests/golden/facefix_builder.npz, and the unchanged whole-frame functions
(crop_frames / composite_frames) on the same inputs.  There is no tolerance anywhere."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import facefix_builder_support as FS

pytestmark = pytest.mark.gpu

GUARD, PAD = 0x5A, 64
SWEEP_H, SWEEP_W = 40, 300
SWEEP_ENHANCED = (9, 7)                   # (h, w) of every repaired frame of the sweep
#: one entry per frame: (left, top, right, bottom) or None
SWEEP_BOXES = [
    None,                                 # the first frame has no box
    (0, 0, 1, 1), (299, 0, 300, 1), (0, 39, 1, 40), (299, 39, 300, 40),      # 1 x 1 in every corner
    (5, 3, 6, 10), (5, 3, 12, 4),         # 1 x 7 and 7 x 1
    (10, 10, 26, 26),                     # 16 x 16: exactly one tile
    (10, 10, 27, 26),                     # 17 x 16: a second tile of 16 pixels
    (20, 5, 40, 25),                      # strength 0: the frame stays out of the launch
    (3, 7, 260, 8),                       # 257 x 1
    (0, 0, 300, 40),                      # the whole frame: 47 tiles
    (100, 20, 103, 23),                   # 3 x 3: fewer than 16 selected pixels, never matched
    (200, 10, 216, 26),                   # 16 x 16 beside it: matched
    (50, 20, 57, 29),                     # 7 x 9: the repaired frame already has the box's size
    None,                                 # the last frame has no box
]
SWEEP_STRENGTHS = [1.0, 1.0, 0.65, 1.0, 0.3, 1.0, 0.65, 1.0, 0.65, 0.0, 1.0, 0.65, 1.0, 1.0, 0.65, 1.0]
SWEEP_SETTINGS = [(feather, cm) for cm in (0.0, 0.65) for feather in (0, 1, 18)]


@pytest.fixture(scope="module")
def ff(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix
    return VRGDG_FaceFix


@pytest.fixture(scope="module")
def golden():
    with open(FS.FIXTURE_JSON) as fh:
        meta = json.load(fh)
    return meta, np.load(FS.FIXTURE_NPZ)


@pytest.fixture(scope="module")
def sweep():
    """(originals, enhanced: one per box) of the geometry sweep, made once"""
    originals = FS.make_frames("smooth", (len(SWEEP_BOXES), SWEEP_H, SWEEP_W, 3), 6100)
    n = sum(b is not None for b in SWEEP_BOXES)
    return originals, FS.make_frames("random", (n,) + SWEEP_ENHANCED + (3,), 6101)


def _boxes(case):
    return [tuple(b) if b is not None else None for b in case["boxes"]]


def _blocks(whole, plan):
    return [whole[f, top:top + h, left:left + w] for f, (left, top, w, h) in zip(plan.frames, plan.boxes)]


def _pasted(originals, boxes, blocks, plan):
    out = originals.copy()
    for f, (left, top, w, h), block in zip(plan.frames, plan.boxes, blocks):
        out[f, top:top + h, left:left + w] = block
    return out


# ---- the fixtures of the whole-frame route ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(4))
def test_crops_equal_the_recorded_bytes_the_restatement_and_crop_frames(ff, golden, index):
    case = golden[0]["crops"][index]
    size, boxes = case["enhance_size"], _boxes(case)
    assert size in FS.CROP_SIZES
    frames = FS.make_frames(case["frames"]["kind"], case["frames"]["shape"], case["frames"]["seed"])
    want = golden[1]["crop." + case["key"]]
    assert np.array_equal(FS.crops(frames, boxes, size), want)
    given = torch.from_numpy(frames.copy())
    got = ff.crop_frames_packed(given, boxes, size)
    assert isinstance(got, torch.Tensor) and not got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
    assert np.array_equal(given.numpy(), frames)                            # the frames are never written
    plan = ff.packed_plan(*frames.shape[:3], boxes)
    moved = ff.last_transfer()
    assert moved["bytes_up"] == plan.bytes_up < frames.nbytes and moved["bytes_down"] == want.nbytes and moved["enhanced_up"] == 0
    listed = ff.crop_frames_packed([f for f in frames], boxes, size)
    assert isinstance(listed, list) and np.array_equal(np.stack(listed), want)
    assert np.array_equal(ff.crop_frames(torch.from_numpy(frames), boxes, size).numpy(), want)       # the whole-frame route, unchanged


@pytest.mark.parametrize("key", sorted(FS.COMPOSITE_CASES))
def test_composites_equal_the_recorded_bytes_the_restatement_and_composite_frames(ff, golden, key):
    case = next(c for c in golden[0]["composites"] if c["key"] == key)
    originals, enhanced, boxes, strengths, feather, cm = FS.case_inputs(key)
    want = originals.copy()
    for f, box in enumerate(case["boxes"]):
        if box is not None:
            want[f, box[1]:box[3], box[0]:box[2]] = golden[1][f"composite.{key}.{f}"]
    assert np.array_equal(FS.composite(originals, enhanced, boxes, strengths, feather, cm), want)
    plan = ff.packed_plan(*originals.shape[:3], boxes, strengths)
    blocks = ff.composite_boxes_packed(torch.from_numpy(originals), torch.from_numpy(enhanced), boxes, strengths, feather, cm)
    assert len(blocks) == len(plan.frames)
    for got, block in zip(blocks, _blocks(want, plan)):
        assert got.dtype == np.uint8 and np.array_equal(got, block)
    moved = ff.last_transfer()
    assert moved["bytes_up"] == plan.bytes_up and moved["bytes_down"] == plan.bytes_down and plan.bytes_up < originals.nbytes
    assert moved["enhanced_up"] == len(plan.frames) * enhanced[0].nbytes
    given = torch.from_numpy(originals.copy())
    got = ff.composite_frames_packed(given, torch.from_numpy(enhanced), boxes, strengths, feather, cm)
    assert isinstance(got, torch.Tensor) and not got.is_cuda and np.array_equal(got.numpy(), want)
    assert np.array_equal(given.numpy(), originals)                         # originals_u8 is never written
    listed = [f.copy() for f in originals]
    same = ff.composite_frames_packed(listed, [e for e in enhanced], boxes, strengths, feather, cm, inplace=True)
    assert same is listed and np.array_equal(np.stack(listed), want)
    # one repaired frame per ORIGINAL frame instead of one per box
    per_frame = np.zeros((len(boxes),) + enhanced.shape[1:], dtype=np.uint8)
    per_frame[[f for f, b in enumerate(boxes) if b is not None]] = enhanced
    assert np.array_equal(np.stack(ff.composite_frames_packed([f for f in originals], [e for e in per_frame], boxes, strengths, feather, cm)), want)
    whole = ff.composite_frames(torch.from_numpy(originals), torch.from_numpy(enhanced), boxes, strengths, feather, cm)
    assert np.array_equal(whole.numpy(), want)                              # the whole-frame route, unchanged


def test_gpu_resident_frames_are_refused_and_nothing_to_do_moves_nothing(ff, pkg):
    from comfyui_vrgamedevgirl_amd.VRGDG_StandaloneVideoEnhancerNodes import DecodedFrames
    frames = FS.make_frames("random", (2, 12, 12, 3), 1)
    dev = torch.from_numpy(frames).cuda()
    with pytest.raises(TypeError, match="crop_frames"):
        ff.crop_frames_packed(dev, [(0, 0, 4, 4), None], 8)
    with pytest.raises(TypeError, match="crop_frames"):
        ff.crop_frames_packed(DecodedFrames(dev), [(0, 0, 4, 4), None], 8)
    with pytest.raises(TypeError, match="composite_frames"):
        ff.composite_frames_packed(dev, torch.from_numpy(frames), [(0, 0, 4, 4), None], 1.0)
    with pytest.raises(TypeError, match="composite_frames"):
        ff.composite_frames_packed(torch.from_numpy(frames), dev, [(0, 0, 4, 4), None], 1.0)
    assert tuple(ff.crop_frames_packed(torch.from_numpy(frames), [None, None], 16).shape) == (0, 16, 16, 3)
    assert ff.crop_frames_packed([f for f in frames], [None, None], 16) == []
    assert ff.composite_boxes_packed([f for f in frames], None, [None, (0, 0, 4, 4)], [1.0, 0.0]) == []
    assert ff.last_transfer() == {"bytes_up": 0, "bytes_down": 0, "enhanced_up": 0, "tables_up": 0}
    got = ff.composite_frames_packed([f for f in frames], None, [None, None], 1.0)
    assert np.array_equal(np.stack(got), frames)


# ---- the geometry sweep -------------------------------------------------------------------------------------------------------------------
def test_sweep_is_what_it_says(ff):
    plan = ff.packed_plan(len(SWEEP_BOXES), SWEEP_H, SWEEP_W, SWEEP_BOXES, SWEEP_STRENGTHS)
    assert SWEEP_BOXES[0] is None and SWEEP_BOXES[-1] is None and 9 not in plan.frames and plan.n_boxes == len(plan.frames) + 1
    tiles = dict(zip(plan.frames, np.diff(plan.tile_prefix)))
    assert tiles[7] == 1 and tiles[8] == 2 and tiles[10] == 2 and tiles[11] == 47 and tiles[1] == 1
    assert any(offset % 16 for offset in plan.offsets) and any(offset % 4 for offset in plan.offsets)
    assert int((FS.soft_ellipse_mask(3, 3, 0) > np.float32(0.35)).sum()) < 16 <= int((FS.soft_ellipse_mask(16, 16, 0) > np.float32(0.35)).sum())
    assert (SWEEP_BOXES[14][3] - SWEEP_BOXES[14][1], SWEEP_BOXES[14][2] - SWEEP_BOXES[14][0]) == SWEEP_ENHANCED


@pytest.mark.parametrize("size", (8, 17))
def test_sweep_crops(ff, sweep, size):
    """8 x 8 is less than a workgroup per record, 17 x 17 a second workgroup of 33 pixels; boxes from 1 x 1 to the whole frame"""
    originals, _ = sweep
    want = FS.crops(originals, SWEEP_BOXES, size)
    got = ff.crop_frames_packed([f for f in originals], SWEEP_BOXES, size)
    assert np.array_equal(np.stack(got), want)
    assert np.array_equal(ff.crop_frames(torch.from_numpy(originals), SWEEP_BOXES, size).numpy(), want)


@pytest.mark.parametrize("feather,cm", SWEEP_SETTINGS)
def test_sweep_composites(ff, sweep, feather, cm):
    originals, enhanced = sweep
    want = FS.composite(originals, enhanced, SWEEP_BOXES, SWEEP_STRENGTHS, feather, cm)
    got = ff.composite_frames_packed([f for f in originals], [e for e in enhanced], SWEEP_BOXES, SWEEP_STRENGTHS, feather, cm)
    diff = np.abs(np.stack(got).astype(np.int16) - want.astype(np.int16))
    print(f"feather {feather}, color_match {cm}: {int((diff != 0).sum())} bytes differ, largest difference {int(diff.max())} levels")
    assert np.array_equal(np.stack(got), want)
    for f in (0, 9, 15):                                                    # no box, strength 0: the frame comes back unchanged
        assert np.array_equal(got[f], originals[f])
    whole = ff.composite_frames(torch.from_numpy(originals), torch.from_numpy(enhanced), SWEEP_BOXES, SWEEP_STRENGTHS, feather, cm)
    assert np.array_equal(whole.numpy(), want)


# ---- the tile map's seams in one call ------------------------------------------------------------------------------------------------------
#: boxes at which the shared tile map (csrc/vrg_packed_tiles.hpp) can go wrong, one per frame of 32 x 300: a single pixel, 255 pixels (one
#: short of a tile), 256 (exactly one), 257 x 1 (a tile plus one pixel), and a frame without a box -- five frames, since a frame has one box
SEAM_H, SEAM_W = 32, 300
SEAM_BOXES = [(7, 5, 8, 6), (20, 3, 35, 20), None, (100, 10, 116, 26), (30, 31, 287, 32)]


@pytest.mark.parametrize("cm", (0.0, 0.65))
def test_tile_seams_equal_the_whole_frame_route(ff, cm):
    plan = ff.packed_plan(len(SEAM_BOXES), SEAM_H, SEAM_W, SEAM_BOXES, [1.0] * len(SEAM_BOXES))
    assert [w * h for _, _, w, h in plan.boxes] == [1, 255, 256, 257] and list(plan.tile_prefix) == [0, 1, 2, 3, 5] and plan.frames == [0, 1, 3, 4]
    originals = FS.make_frames("random", (len(SEAM_BOXES), SEAM_H, SEAM_W, 3), 6400)
    enhanced = FS.make_frames("random", (4, 9, 7, 3), 6401)
    got = ff.composite_frames_packed(torch.from_numpy(originals), torch.from_numpy(enhanced), SEAM_BOXES, [1.0] * len(SEAM_BOXES), 1, cm)
    whole = ff.composite_frames(torch.from_numpy(originals).cuda(), torch.from_numpy(enhanced).cuda(), SEAM_BOXES, [1.0] * len(SEAM_BOXES), 1, cm)
    assert np.array_equal(got.numpy(), whole.cpu().numpy())
    assert np.array_equal(got[2].numpy(), originals[2]) and not np.array_equal(got.numpy(), originals)
    for f, (left, top, w, h) in zip(plan.frames, plan.boxes):                # nothing outside a box was written
        outside = np.ones((SEAM_H, SEAM_W), dtype=bool)
        outside[top:top + h, left:left + w] = False
        assert np.array_equal(got[f].numpy()[outside], originals[f][outside]), f


def test_seven_hundred_small_boxes(ff):
    """700 frames of 6 x 6 with boxes of 2 x 2 and 3 x 3 in turn: one tile each, so the search runs over 700 equal steps"""
    n = 700
    originals = FS.make_frames("random", (n, 6, 6, 3), 6200)
    enhanced = FS.make_frames("random", (n, 4, 5, 3), 6201)
    boxes = [((f % 4), (f % 3), (f % 4) + 2 + (f & 1), (f % 3) + 2 + (f & 1)) for f in range(n)]
    strengths = [(1.0, 0.65, 0.3)[f % 3] for f in range(n)]
    plan = ff.packed_plan(n, 6, 6, boxes, strengths)
    assert len(plan.frames) == n and plan.tiles == n and {(b[2], b[3]) for b in plan.boxes} == {(2, 2), (3, 3)}
    want = FS.composite(originals, enhanced, boxes, strengths, 1, 0.65)
    got = ff.composite_frames_packed(torch.from_numpy(originals), torch.from_numpy(enhanced), boxes, strengths, 1, 0.65)
    assert np.array_equal(got.numpy(), want)
    crops = ff.crop_frames_packed(torch.from_numpy(originals), boxes, 4)
    assert np.array_equal(crops.numpy(), FS.crops(originals, boxes, 4))


# ---- through the C ABI: guard bytes, records made bad in the table ------------------------------------------------------------------------
def _guarded(nbytes):
    raw = torch.full((nbytes + 2 * PAD,), GUARD, dtype=torch.uint8, device="cuda")
    return raw, raw[PAD:PAD + nbytes]


def _intact(raw, view):
    return bool((raw[:PAD] == GUARD).all()) and bool((raw[PAD + view.numel():] == GUARD).all())


def _abi_composite(ff, originals, enhanced, boxes, strengths, feather, cm, edit=None, extra_tiles=0):
    """composite_boxes_packed by hand, every buffer a kernel writes between guard bytes; `edit(desc)` spoils records before the upload"""
    from comfyui_vrgamedevgirl_amd import _hip
    plan = ff.packed_plan(*originals.shape[:3], boxes, strengths)
    n, total, (EH, EW) = len(plan.frames), plan.bytes_up, enhanced.shape[1:3]
    stage = np.zeros(total, dtype=np.uint8)
    ff._pack_boxes(list(originals), plan, stage)
    spans, records, mask_offsets, mask_floats, largest = ff._mask_tables([(b[2], b[3]) for b in plan.boxes], feather)
    table, tap_offsets = ff._tap_tables([(b[3], b[2]) for b in plan.boxes], lambda s: (EH, EW), lambda s: s)
    desc = np.zeros(n, dtype=ff._PACKED_DESC)
    for i, ((_, _, w, h), offset, s) in enumerate(zip(plan.boxes, plan.offsets, plan.strengths)):
        desc[i] = (offset, offset, w, h, i, s, mask_offsets[(w, h)], tap_offsets[(h, w)], offset)
    if edit is not None:
        edit(desc)
    verdict = _hip.host_library().vrg_ff_packed_check(C.c_void_p(desc.ctypes.data), n, C.c_void_p(plan.tile_prefix.ctypes.data), total, total, n,
                                                      mask_floats, len(table), total, 0, 0)
    src = torch.from_numpy(stage).cuda()
    enh = torch.from_numpy(np.ascontiguousarray(enhanced[plan.box_index])).cuda()
    dev_desc = ff._upload(desc, src.device, trailing=(plan.tile_prefix,))
    prefix = C.c_void_p(dev_desc.data_ptr() + desc.nbytes)
    taps = ff._upload(table, src.device)
    masks = ff._run_masks(spans, records, mask_floats, largest, feather, src.device)
    (raw_face, face), (raw_stats, stats), (raw_out, out) = _guarded(total), _guarded(n * 96), _guarded(total)
    lib, stream = _hip.lib(), _hip.current_stream()
    tiles = plan.tiles + extra_tiles
    assert lib.vrg_ff_packed_resize_stats_u8(_hip.ptr(src), total, _hip.ptr(enh), n, EH, EW, _hip.ptr(masks), mask_floats, _hip.ptr(dev_desc),
                                             prefix, n, tiles, _hip.ptr(taps), len(table), _hip.ptr(face), total, _hip.ptr(stats), cm,
                                             stream) == _hip.VRG_OK
    assert lib.vrg_ff_packed_composite_u8(_hip.ptr(src), total, _hip.ptr(masks), mask_floats, _hip.ptr(dev_desc), prefix, n, tiles,
                                          _hip.ptr(face), total, _hip.ptr(stats), _hip.ptr(out), total, stream) == _hip.VRG_OK
    torch.cuda.synchronize()
    assert _intact(raw_face, face) and _intact(raw_stats, stats) and _intact(raw_out, out)
    assert np.array_equal(src.cpu().numpy(), stage)                         # the packed originals are never written
    words = stats.cpu().numpy().view(np.int64).reshape(n, 12)
    return plan, desc, verdict, out.cpu().numpy(), words


def test_guards_statistics_and_a_grid_longer_than_the_table(ff, sweep):
    from comfyui_vrgamedevgirl_amd import _hip
    import lanczos_support as LS
    originals, enhanced = sweep
    want = FS.composite(originals, enhanced, SWEEP_BOXES, SWEEP_STRENGTHS, 1, 0.65)
    for extra in (0, 3):                                                    # workgroups past the last tile find no tile of theirs
        plan, desc, verdict, out, words = _abi_composite(ff, originals, enhanced, SWEEP_BOXES, SWEEP_STRENGTHS, 1, 0.65, extra_tiles=extra)
        assert verdict == _hip.VRG_OK
        for block, offset in zip(_blocks(want, plan), plan.offsets):
            assert np.array_equal(out[offset:offset + block.size].reshape(block.shape), block)
    for i, (f, (left, top, w, h), index) in enumerate(zip(plan.frames, plan.boxes, plan.box_index)):
        resized = np.asarray(LS.restated(enhanced[index:index + 1], w, h))[0]
        _, sums = FS.color_match(resized, originals[f, top:top + h, left:left + w], FS.soft_ellipse_mask(w, h, 1), 0.65)
        assert [int(v) for v in words[i, :7]] == sums and int(words[i, 7]) == (1 if sums[0] >= 16 else 0), (i, f)
        assert list(words[i, 10:]) == [0, 0]
    matched = {f: int(words[i, 7]) for i, f in enumerate(plan.frames)}
    assert matched[12] == 0 and matched[13] == 1 and matched[11] == 1       # 3 x 3 unmatched beside 16 x 16 matched


def test_crop_guards_and_records_made_bad_in_the_table(ff, sweep):
    """a record whose block or taps lie outside the stated sizes is refused by vrg_ff_packed_check, and on the device writes zeros"""
    from comfyui_vrgamedevgirl_amd import _hip
    originals, _ = sweep
    size = 8
    plan = ff.packed_plan(len(SWEEP_BOXES), SWEEP_H, SWEEP_W, SWEEP_BOXES)
    n, total = len(plan.frames), plan.bytes_up
    stage = np.zeros(total, dtype=np.uint8)
    ff._pack_boxes(list(originals), plan, stage)
    table, offsets = ff._tap_tables([(b[3], b[2]) for b in plan.boxes], lambda s: s, lambda s: (size, size))
    desc = np.zeros(n, dtype=ff._PACKED_DESC)
    for i, ((_, _, w, h), offset) in enumerate(zip(plan.boxes, plan.offsets)):
        desc[i] = (offset, 0, w, h, 0, 0.0, 0, offsets[(h, w)], 0)

    def check(records):
        return _hip.host_library().vrg_ff_packed_check(C.c_void_p(records.ctypes.data), n, None, total, 0, 0, 0, len(table), 0, size, size)

    assert check(desc) == _hip.VRG_OK
    bad = {2: ("src_offset", total), 5: ("src_offset", -1), 7: ("taps_offset", len(table)), 9: ("box_w", 0), 10: ("src_offset", total - 5)}
    spoiled = desc.copy()
    for i, (name, value) in bad.items():
        spoiled[i][name] = value
        single = desc.copy()
        single[i][name] = value
        assert check(single) == _hip.VRG_ERR_BAD_ARG, (i, name)
    assert check(spoiled) == _hip.VRG_ERR_BAD_ARG
    src, taps = torch.from_numpy(stage).cuda(), ff._upload(table, "cuda")
    want = FS.crops(originals, SWEEP_BOXES, size)
    for records, zeros in ((desc, ()), (spoiled, tuple(bad))):
        raw, out = _guarded(n * size * size * 3)
        dev_desc = ff._upload(records, "cuda")
        assert _hip.lib().vrg_lanczos4_packed_u8(_hip.ptr(src), total, _hip.ptr(dev_desc), n, _hip.ptr(out), size, size, _hip.ptr(taps), len(table),
                                                 _hip.current_stream()) == _hip.VRG_OK
        torch.cuda.synchronize()
        assert _intact(raw, out)
        got = out.cpu().numpy().reshape(n, size, size, 3)
        for i in range(n):
            assert np.array_equal(got[i], np.zeros_like(want[i]) if i in zeros else want[i]), i


def test_composite_records_made_bad_in_the_table(ff, sweep):
    """vrg_ff_packed_check refuses them first; on the device a record that may not be blended comes out as a copy of its original bytes, one
    without a place to read or write leaves the output alone, and one the statistics launch does not follow has zero statistics"""
    from comfyui_vrgamedevgirl_amd import _hip
    originals, enhanced = sweep
    want = FS.composite(originals, enhanced, SWEEP_BOXES, SWEEP_STRENGTHS, 1, 0.65)
    good = _abi_composite(ff, originals, enhanced, SWEEP_BOXES, SWEEP_STRENGTHS, 1, 0.65)
    plan, total = good[0], good[0].bytes_up
    copies = {1: ("mask_offset", 1 << 40), 6: ("bytes_offset", total - 2), 10: ("strength", 0.0), 11: ("mask_offset", -1)}
    skipped = {3: ("dst_offset", total), 8: ("src_offset", 1 << 40)}
    unread = {4: ("enhanced_index", len(plan.frames)), 12: ("taps_offset", 1 << 40)}      # refused as well; only their verdict is asked here
    for i, (name, value) in {**copies, **skipped, **unread}.items():
        def one(desc, i=i, name=name, value=value):
            desc[i][name] = value
        assert _abi_composite(ff, originals, enhanced, SWEEP_BOXES, SWEEP_STRENGTHS, 1, 0.65, edit=one)[2] == _hip.VRG_ERR_BAD_ARG, (i, name)

    def spoil(desc):
        for i, (name, value) in {**copies, **skipped}.items():
            desc[i][name] = value

    _, desc, verdict, out, words = _abi_composite(ff, originals, enhanced, SWEEP_BOXES, SWEEP_STRENGTHS, 1, 0.65, edit=spoil)
    assert verdict == _hip.VRG_ERR_BAD_ARG
    for i, (f, (left, top, w, h), offset) in enumerate(zip(plan.frames, plan.boxes, plan.offsets)):
        block = out[offset:offset + w * h * 3].reshape(h, w, 3)
        if i in copies:
            assert np.array_equal(block, originals[f, top:top + h, left:left + w]), i
        elif i in skipped:
            assert (block == GUARD).all(), i
        else:
            assert np.array_equal(block, want[f, top:top + h, left:left + w]), i
        if i in copies or skipped.get(i, ("",))[0] == "src_offset":           # not followed by the statistics launch either
            assert not words[i].any(), i
        else:
            assert np.array_equal(words[i], good[4][i]), i

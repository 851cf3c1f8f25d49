"""The AI Video Builder's Face Fix on the GPU (comfyui-vrgamedevgirl_amd/VRGDG_FaceFix.py, csrc/vrg_facefix.hip): every case equals the
bytes the reference's own route gave (tests/golden/facefix_builder.npz, made by tools/make_golden_facefix_builder.py), exactly.  All cases
keep the selected count at or below 65,793, where the reference's fp32 means are the exact means."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import facefix_builder_support as FS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ff(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix
    return VRGDG_FaceFix


@pytest.fixture(scope="module")
def golden():
    with open(FS.FIXTURE_JSON) as fh:
        meta = json.load(fh)
    return meta, np.load(FS.FIXTURE_NPZ)


def _want(golden, case, originals):
    want = originals.copy()
    for f, box in enumerate(case["boxes"]):
        if box is not None:
            want[f, box[1]:box[3], box[0]:box[2]] = golden[1][f"composite.{case['key']}.{f}"]
    return want


def _boxes(case):
    return [tuple(b) if b is not None else None for b in case["boxes"]]


@pytest.mark.parametrize("index", range(4))
def test_crops_equal_the_reference_route(ff, golden, index):
    case = golden[0]["crops"][index]
    want = golden[1]["crop." + case["key"]]
    frames = FS.make_frames(case["frames"]["kind"], case["frames"]["shape"], case["frames"]["seed"])
    dev = torch.from_numpy(frames).cuda()
    got = ff.crop_frames(dev, _boxes(case), case["enhance_size"])
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(dev.cpu().numpy(), frames)                        # the frames are never written
    # the same bytes from CPU frames, in the form they came in
    cpu = ff.crop_frames(torch.from_numpy(frames), _boxes(case), case["enhance_size"])
    assert not cpu.is_cuda and np.array_equal(cpu.numpy(), want)
    listed = ff.crop_frames([f for f in frames], _boxes(case), case["enhance_size"])
    assert isinstance(listed, list) and np.array_equal(np.stack(listed), want)


def test_crop_of_the_output_size_is_a_byte_copy(ff):
    frames = FS.make_frames("random", FS.FRAMES_SHAPE, FS.FRAMES_SEED + 1)
    for size, boxes in FS.CROP_BOXES["copy_and_down"].items():
        left, top, right, bottom = boxes[0]
        assert (right - left, bottom - top) == (size, size)
        got = ff.crop_frames(torch.from_numpy(frames).cuda(), boxes, size).cpu().numpy()
        assert np.array_equal(got[0], frames[0, top:bottom, left:right])
    assert tuple(ff.crop_frames(torch.from_numpy(frames).cuda(), [None] * 5, 16).shape) == (0, 16, 16, 3)


@pytest.mark.parametrize("index", range(6))
def test_composites_equal_the_reference_route(ff, golden, index):
    case = golden[0]["composites"][index]
    originals, enhanced, boxes, strengths, feather, cm = FS.case_inputs(case["key"])
    assert [list(b) if b else None for b in boxes] == case["boxes"] and strengths == case["strengths"]
    want = _want(golden, case, originals)
    dev, enh = torch.from_numpy(originals).cuda(), torch.from_numpy(enhanced).cuda()
    got = ff.composite_frames(dev, enh, boxes, strengths, feather, cm)
    assert got.is_cuda and got.shape == dev.shape and got.data_ptr() != dev.data_ptr()
    diff = np.abs(got.cpu().numpy().astype(np.int16) - want.astype(np.int16))
    print(f"{case['key']}: {int((diff != 0).sum())} bytes differ, largest difference {int(diff.max())} levels")
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(dev.cpu().numpy(), originals)                     # originals_u8 is never written
    for f, box in enumerate(boxes):                                         # no box, or strength 0: the frame comes back unchanged
        if box is None or strengths[f] <= 0:
            assert np.array_equal(got[f].cpu().numpy(), originals[f])
    # CPU inputs give the identical bytes, in the form they came in
    cpu = ff.composite_frames(torch.from_numpy(originals), torch.from_numpy(enhanced), boxes, strengths, feather, cm)
    assert not cpu.is_cuda and np.array_equal(cpu.numpy(), want)


def test_lists_decoded_frames_and_one_enhanced_frame_per_original(ff, golden, pkg):
    from comfyui_vrgamedevgirl_amd.VRGDG_StandaloneVideoEnhancerNodes import DecodedFrames
    case = next(c for c in golden[0]["composites"] if c["key"] == "f18_cm065_64")
    originals, enhanced, boxes, strengths, feather, cm = FS.case_inputs(case["key"])
    want = _want(golden, case, originals)
    listed = ff.composite_frames([f for f in originals], [e for e in enhanced], boxes, strengths, feather, cm)
    assert isinstance(listed, list) and np.array_equal(np.stack(listed), want)
    decoded = ff.composite_frames(DecodedFrames(torch.from_numpy(originals).cuda()), torch.from_numpy(enhanced).cuda(), boxes, strengths, feather, cm)
    assert isinstance(decoded, DecodedFrames) and np.array_equal(decoded.u8.cpu().numpy(), want)
    per_frame = np.zeros((len(boxes),) + enhanced.shape[1:], dtype=np.uint8)
    per_frame[[f for f, b in enumerate(boxes) if b is not None]] = enhanced
    got = ff.composite_frames(torch.from_numpy(originals).cuda(), torch.from_numpy(per_frame).cuda(), boxes, strengths, feather, cm)
    assert np.array_equal(got.cpu().numpy(), want)
    # an unaligned batch (a view one byte into a buffer) takes the byte path: the same bytes
    raw = torch.zeros(originals.size + 1, dtype=torch.uint8, device="cuda")
    raw[1:] = torch.from_numpy(originals).cuda().reshape(-1)
    got = ff.composite_frames(raw[1:].view(originals.shape), torch.from_numpy(enhanced).cuda(), boxes, strengths, feather, cm)
    assert np.array_equal(got.cpu().numpy(), want)
    # nothing to composite: the originals come back as a fresh batch
    none = ff.composite_frames(torch.from_numpy(originals).cuda(), None, [None] * len(boxes), 1.0, feather, cm)
    assert np.array_equal(none.cpu().numpy(), originals)


@pytest.mark.parametrize("w,h,feather", ((37, 41, 0), (37, 41, 1), (37, 41, 18), (20, 23, 18), (64, 64, 256), (1, 7, 18), (5, 5, 1), (301, 287, 18)))
def test_masks_equal_the_restatement_bit_for_bit(ff, w, h, feather):
    got = ff._soft_ellipse_mask(w, h, feather)
    want = FS.soft_ellipse_mask(w, h, feather)
    assert got.dtype == np.float32 and got.shape == (h, w) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_statistics_are_the_exact_sums(ff, golden):
    """the record of vrg_ff_resize_stats_u8 through the C ABI: count and six integer sums, matched, shifts"""
    from comfyui_vrgamedevgirl_amd import _hip
    import lanczos_support as LS
    originals = FS.make_frames("smooth", (2, 90, 160, 3), 1)
    enhanced = FS.make_frames("random", (2, 48, 40, 3), 2)
    boxes = [(30, 20, 67, 61), (100, 50, 105, 55)]
    x, e = torch.from_numpy(originals).cuda(), torch.from_numpy(enhanced).cuda()
    spans, records, offsets, floats, largest = ff._mask_tables([(37, 41), (5, 5)], 1)
    masks = ff._run_masks(spans, records, floats, largest, 1, x.device)
    table, tap_offsets = ff._tap_tables([(41, 37), (5, 5)], lambda s: (48, 40), lambda s: s)
    desc = np.zeros(2, dtype=ff._FF_DESC)
    desc[0] = (0, 30, 20, 37, 41, 1.0, offsets[(37, 41)], tap_offsets[(41, 37)], 0)
    desc[1] = (1, 100, 50, 5, 5, 1.0, offsets[(5, 5)], tap_offsets[(5, 5)], 37 * 41 * 3)
    capacity = 37 * 41 * 3 + 75
    face = torch.zeros(capacity, dtype=torch.uint8, device="cuda")
    stats = torch.full((2 * _hip.FACEFIX_STATS_WORDS,), -1, dtype=torch.int64, device="cuda")
    taps, dev_desc = ff._upload(table, x.device), ff._upload(desc, x.device)
    _hip.check(_hip.lib().vrg_ff_resize_stats_u8(_hip.ptr(x), _hip.ptr(e), _hip.ptr(masks), floats, _hip.ptr(dev_desc), _hip.ptr(taps), len(table),
                                                 _hip.ptr(face), capacity, _hip.ptr(stats), 2, 2, 90, 160, 48, 40, largest, 1.0,
                                                 _hip.current_stream()), "vrg_ff_resize_stats_u8")
    rec = stats.cpu().numpy().reshape(2, -1)
    for f, (left, top, right, bottom) in enumerate(boxes):
        w, h = right - left, bottom - top
        resized = np.asarray(LS.restated(enhanced[f:f + 1], w, h))[0]
        start = int(desc[f]["bytes_offset"])
        assert np.array_equal(face[start:start + w * h * 3].cpu().numpy().reshape(h, w, 3), resized)
        _, sums = FS.color_match(resized, originals[f, top:bottom, left:right], FS.soft_ellipse_mask(w, h, 1), 1.0)
        assert [int(v) for v in rec[f, :7]] == sums and int(rec[f, 7]) == (1 if sums[0] >= 16 else 0)
        assert list(rec[f, 10:]) == [0, 0]
    assert int(rec[1, 0]) < 16 and list(rec[1, 8:10]) == [0, 0]


def test_abi_refusals_and_records_that_name_nothing(ff):
    """through the C ABI on the device: in == out is refused, zero frames launch nothing, a record outside the stated sizes is "no box" """
    from comfyui_vrgamedevgirl_amd import _hip
    lib, stream = _hip.lib(), _hip.current_stream()
    frames = FS.make_frames("random", (2, 24, 32, 3), 3)
    x = torch.from_numpy(frames).cuda()
    out = torch.full((3, 8, 8, 3), 7, dtype=torch.uint8, device="cuda")
    table = ff._lanczos_taps(10, 10, 8, 8)
    desc = np.zeros(3, dtype=ff._BOX_DESC)
    desc[0] = (1, 5, 6, 10, 10, 0, 0)
    desc[1] = (2, 5, 6, 10, 10, 0, 0)                                       # a frame that is not there
    desc[2] = (0, 25, 6, 10, 10, 0, 0)                                      # a box over the right edge
    taps, dev_desc = ff._upload(table, x.device), ff._upload(desc, x.device)
    args = (_hip.ptr(x), 2, 24, 32, _hip.ptr(out), _hip.ptr(dev_desc))
    assert lib.vrg_lanczos4_boxes_u8(*args, 0, 8, 8, _hip.ptr(taps), len(table), stream) == _hip.VRG_OK
    assert int(out.min()) == 7                                              # zero frames: nothing written
    assert lib.vrg_lanczos4_boxes_u8(_hip.ptr(x), 2, 24, 32, _hip.ptr(x), _hip.ptr(dev_desc), 3, 8, 8, _hip.ptr(taps), len(table), stream) == _hip.VRG_ERR_BAD_ARG
    assert lib.vrg_lanczos4_boxes_u8(*args, 3, 8, 8, _hip.ptr(taps), len(table), stream) == _hip.VRG_OK
    got = out.cpu().numpy()
    assert np.array_equal(got[0], FS.crops(frames, [None, (5, 6, 15, 16)], 8)[0]) and not got[1].any() and not got[2].any()
    assert lib.vrg_lanczos4_boxes_u8(*args, 3, 8, 8, _hip.ptr(taps), len(table) - 1, stream) == _hip.VRG_OK      # the records end before the table
    assert not out.cpu().numpy().any()
    # the composite: a record whose mask or bytes lie outside what was stated copies the frame
    masks = torch.ones(100, dtype=torch.float32, device="cuda")
    face = torch.full((300,), 255, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(2 * _hip.FACEFIX_STATS_WORDS, dtype=torch.int64, device="cuda")
    fd = np.zeros(2, dtype=ff._FF_DESC)
    fd[0] = (0, 2, 3, 10, 10, 1.0, 0, 0, 0)
    fd[1] = (0, 2, 3, 10, 10, 1.0, 1, 0, 0)                                 # the mask would end one float past the table
    dev_fd = ff._upload(fd, x.device)
    res = torch.empty_like(x)
    assert lib.vrg_ff_composite_u8(_hip.ptr(x), _hip.ptr(masks), 100, _hip.ptr(dev_fd), _hip.ptr(face), 300, _hip.ptr(stats), _hip.ptr(x), 2, 24, 32,
                                   stream) == _hip.VRG_ERR_BAD_ARG
    assert lib.vrg_ff_composite_u8(_hip.ptr(x), _hip.ptr(masks), 100, _hip.ptr(dev_fd), _hip.ptr(face), 300, _hip.ptr(stats), _hip.ptr(res), 2, 24, 32,
                                   stream) == _hip.VRG_OK
    got = res.cpu().numpy()
    want = frames.copy()
    want[0, 3:13, 2:12] = 255
    assert np.array_equal(got, want)
    assert lib.vrg_ff_composite_u8(_hip.ptr(x), _hip.ptr(masks), 100, _hip.ptr(dev_fd), _hip.ptr(face), 300, _hip.ptr(stats), _hip.ptr(res), 0, 24, 32,
                                   stream) == _hip.VRG_OK

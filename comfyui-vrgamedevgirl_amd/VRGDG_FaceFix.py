"""The pixels of the AI Video Builder's Face Fix (VRGDG_FaceFix.py of the reference: the routes /vrgdg/face_fix/prepare and
/vrgdg/face_fix/finalize) on the GPU, on decoded uint8 B,G,R frames.

``crop_frames``       what ``prepare_face_fix`` does per tracked frame (:473-476): the square box cut out of the frame and
                      ``cv2.resize(crop, (enhance_size, enhance_size), INTER_LANCZOS4)`` -- one launch for a batch of boxes of any sizes.
``composite_frames``  the loop body of ``finalize_face_fix`` (:937-957): the repaired frame resized to its box, ``_soft_ellipse_mask``,
                      ``_color_match``, the fp32 blend under ``alpha * composite_strength`` and the paste into a copy of the original --
                      four launches for a batch, no host round trip in between.

``detection_plan`` / ``detector_blobs`` / ``rotated_frames`` / ``candidates_from_outputs`` / ``detect_with_rotation``
                      the pixel work in front of the face detector and the host arithmetic behind it (``_detect_with_rotation`` /
                      ``_detect``, :67-157) with the Builder's rules: mode names off / light / strong, the caller's regions at angle 0 and
                      ``_initial_regions`` (rounded tiles) at the others, regions with a side below 8 skipped, boxes decoded with
                      round() and kept when x2 > x and y2 > y.  The implementation is shared with VRGDG_StandaloneFaceFixNodes
                      (csrc/vrg_detect.hip); the network is a seam (``forward``), None by default.

``crop_frames_packed`` / ``composite_boxes_packed`` / ``composite_frames_packed`` / ``packed_plan`` / ``last_transfer``
                      the same pixels for frames that stay on the HOST, which is all the two routes ever hold: only the boxes cross
                      the bus, gathered into one page-locked buffer each way (csrc/vrg_facefix_packed.hip).

Device-resident inputs stay on the device; ``crop_frames`` and ``composite_frames`` upload CPU inputs (a uint8 tensor, a list of numpy
frames) whole and download the result whole (the staging helpers of VRGDG_LUTVideoTools); the packed functions take CPU inputs only and
move the boxes.  The detector network, tracking, PNG / video I/O, manifests, ffmpeg and the
aiohttp routes are out of scope.  The arithmetic is csrc/vrg_facefix_math.hpp; the library is reached through ``_hip`` only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _hip, _packed, ops
from ._devices import compute_device
from ._packed import frame_boxes as _boxes, frames_in as _frames_in, pack_boxes as _pack_boxes, peek as _peek

NODE_CLASS_MAPPINGS = {}
NODE_DISPLAY_NAME_MAPPINGS = {}

DEFAULT_FEATHER = 18
DEFAULT_COLOR_MATCH = 0.65
_TAP = _hip.record_dtype(_hip.LzTap)
_BOX_DESC = _hip.record_dtype(_hip.FaceFixBoxDesc)
_MASK_DESC = _hip.record_dtype(_hip.FaceFixMaskDesc)
_FF_DESC = _hip.record_dtype(_hip.FaceFixDesc)

_host = _hip.host_library       # the library for its HOST table functions (no GPU needed)
_lanczos_taps = ops.lanczos4_taps
_upload = _hip.upload_records   # records and the byte / int32 tables that go with them


# ------------------------------------------------------------------------------------------------
# host integers
# ------------------------------------------------------------------------------------------------
def _square_crop_box(face_box, width, height, padding):
    """(left, top, right, bottom) of the square around a tracked face (:207-226): the larger side of the face grown by ``padding`` on both
    sides, no larger than the frame, rounded half to even, pushed back inside the frame."""
    x, y, face_w, face_h = face_box
    side = min(max(face_w, face_h) * (1.0 + 2.0 * max(0.0, padding)), width, height)
    left = int(round(x + face_w / 2.0 - side / 2.0))
    top = int(round(y + face_h / 2.0 - side / 2.0))
    right, bottom = left + int(round(side)), top + int(round(side))
    if left < 0:
        left, right = 0, right - left
    if top < 0:
        top, bottom = 0, bottom - top
    if right > width:
        left, right = left - (right - width), width
    if bottom > height:
        top, bottom = top - (bottom - height), height
    return (max(0, left), max(0, top), min(width, right), min(height, bottom))


def _blend_settings(feather, color_match):
    """(feather, color_match) clamped as finalize_face_fix clamps them (:930-931)"""
    return max(0, min(256, int(feather))), max(0.0, min(1.0, float(color_match)))


def settings_from_payload(payload) -> dict:
    """``feather`` and ``color_match`` as finalize_face_fix reads them (:930-931): a missing or zero value falls back to the default
    (the reference's ``or``), then the clamp."""
    feather, color_match = _blend_settings(payload.get("feather") or DEFAULT_FEATHER, payload.get("color_match") or DEFAULT_COLOR_MATCH)
    return {"feather": feather, "color_match": color_match}


def ellipse_spans(width: int, height: int) -> np.ndarray:
    """[height, 2] int32: the filled pixels x0 .. x1 of every row of the mask's ellipse (x0 > x1: none); host only"""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("ellipse_spans: width and height must be at least 1")
    spans = np.zeros((height, 2), dtype=np.int32)
    _hip.check(_host().vrg_ff_ellipse_spans(width, height, C.c_void_p(spans.ctypes.data)), "vrg_ff_ellipse_spans")
    return spans


def gauss_taps(feather: int) -> int:
    return max(3, 4 * int(feather) + 1)


def gauss_coeffs(feather: int) -> np.ndarray:
    """the fp32 coefficients of the mask's GaussianBlur for 0 <= feather <= 256; host only"""
    feather = int(feather)
    if not 0 <= feather <= 256:
        raise ValueError("gauss_coeffs: feather must lie in 0 .. 256")
    coeffs = np.zeros(gauss_taps(feather), dtype=np.float32)
    _hip.check(_host().vrg_ff_gauss_coeffs(feather, C.c_void_p(coeffs.ctypes.data)), "vrg_ff_gauss_coeffs")
    return coeffs


def _active(boxes, strengths=None):
    """[(frame, box_index, box, strength)] of the ACTIVE frames, in frame order: a box, and strength > 0 where strengths are given (1.0
    without); ``box_index`` = the frame's position among the frames that have a box"""
    with_box = [f for f, box in enumerate(boxes) if box is not None]
    return [(f, k, boxes[f], 1.0 if strengths is None else strengths[f]) for k, f in enumerate(with_box) if strengths is None or strengths[f] > 0.0]


def _tap_tables(sizes, in_size_of, out_size_of):
    """the concatenated Lanczos records of the distinct sizes: -> (table, {size: offset in records})"""
    offsets, parts, total = {}, [], 0
    for size in sizes:
        if size in offsets:
            continue
        (ih, iw), (oh, ow) = in_size_of(size), out_size_of(size)
        offsets[size] = total
        parts.append(_lanczos_taps(ih, iw, oh, ow))
        total += ow + oh
    return (np.concatenate(parts) if parts else np.zeros(1, dtype=_TAP)), offsets


def crop_frames(frames_u8, crop_boxes, enhance_size):
    """``cv2.resize(frame[top:bottom, left:right], (enhance_size, enhance_size), INTER_LANCZOS4)`` for every frame that has a box
    (``crop_boxes``: one (left, top, right, bottom) or None per frame) -> ``[n, S, S, 3]`` uint8 in the order of the frames, in the form
    the frames came in (CUDA tensor, CPU tensor, list of numpy frames, DecodedFrames)."""
    size = int(enhance_size)
    if size < 1:
        raise ValueError("enhance_size must be at least 1")
    boxes = _boxes(crop_boxes, *_peek(frames_u8, "frames"))
    x, back = _frames_in(frames_u8, "frames")
    F, H, W, _ = x.shape
    used = [(f, b) for f, b in enumerate(boxes) if b is not None]
    with torch.cuda.device(x.device):
        out = torch.empty((len(used), size, size, 3), dtype=torch.uint8, device=x.device)
        if used:
            table, offsets = _tap_tables([(b[3], b[2]) for _, b in used], lambda s: s, lambda s: (size, size))
            desc = np.zeros(len(used), dtype=_BOX_DESC)
            for i, (f, (left, top, w, h)) in enumerate(used):
                desc[i] = (f, left, top, w, h, 0, offsets[(h, w)])
            taps, dev_desc = _upload(table, x.device), _upload(desc, x.device)
            _hip.check(_hip.lib().vrg_lanczos4_boxes_u8(_hip.ptr(x), F, H, W, _hip.ptr(out), _hip.ptr(dev_desc), len(used), size, size,
                                                        _hip.ptr(taps), len(table), _hip.current_stream()), "vrg_lanczos4_boxes_u8")
        return back(out)


def _mask_tables(sizes, feather):
    """spans, mask records and the packed offsets of the distinct (w, h): -> (spans, records, {(w, h): offset in floats}, floats, largest)"""
    offsets, spans, records, total, rows, largest = {}, [], [], 0, 0, 0
    for w, h in sizes:
        if (w, h) in offsets:
            continue
        offsets[(w, h)] = total
        spans.append(ellipse_spans(w, h))
        records.append((w, h, rows, total))
        rows += h
        total += w * h
        largest = max(largest, w * h)
    return np.concatenate(spans), np.array(records, dtype=_MASK_DESC), offsets, total, largest


def _composite_tables(boxes, enh_size, feather):
    """active ``boxes`` (left, top, w, h), repaired frames of ``enh_size`` (height, width) -> (spans, mask records, mask offsets, mask_floats,
    largest, tap table, tap offsets)"""
    return (*_mask_tables([(b[2], b[3]) for b in boxes] or [(1, 1)], feather), *_tap_tables([(b[3], b[2]) for b in boxes], lambda s: enh_size, lambda s: s))


def _run_masks(spans, records, total, largest, feather, device):
    """the launches of vrg_ff_masks_f32 -> the packed masks on the device"""
    masks = torch.empty(max(total, 1), dtype=torch.float32, device=device)
    n_coeffs = gauss_taps(feather) if feather > 0 else 0
    coeffs = _upload(gauss_coeffs(feather), device) if n_coeffs else None
    scratch = torch.empty_like(masks) if n_coeffs else None
    dev_spans, dev_records = _upload(spans, device), _upload(records, device)
    _hip.check(_hip.lib().vrg_ff_masks_f32(_hip.ptr(dev_spans), len(spans), _hip.ptr(coeffs) if n_coeffs else None, n_coeffs,
                                           _hip.ptr(dev_records), len(records), largest, _hip.ptr(scratch) if n_coeffs else None,
                                           _hip.ptr(masks), total, _hip.current_stream()), "vrg_ff_masks_f32")
    return masks


def _soft_ellipse_mask(width, height, feather) -> np.ndarray:
    """``_soft_ellipse_mask(width, height, feather)`` of the reference (:880-894) as a float32 ``[height, width]`` array, made on the GPU"""
    width, height, feather = int(width), int(height), max(0, int(feather))
    if width < 1 or height < 1:
        raise ValueError("mask width and height must be at least 1")
    if feather > 256:
        raise ValueError("feather must not exceed 256")
    device = compute_device()
    with torch.cuda.device(device):
        spans, records, _, total, largest = _mask_tables([(width, height)], feather)
        return _run_masks(spans, records, total, largest, feather, device).cpu().numpy().reshape(height, width)


def _strengths(strengths, frames):
    values = [float(strengths)] * frames if isinstance(strengths, (int, float)) else [float(v) for v in strengths]
    if len(values) != frames:
        raise ValueError(f"strengths must hold one value per frame: {len(values)} for {frames} frames")
    return [max(0.0, min(1.0, v)) for v in values]


def composite_frames(originals_u8, enhanced_u8, crop_boxes, strengths, feather=DEFAULT_FEATHER, color_match=DEFAULT_COLOR_MATCH):
    """The loop body of ``finalize_face_fix`` for a batch: ``enhanced_u8`` (one frame per box in the order of the frames, or one per
    original frame) resized to its box, colour matched, blended under the soft ellipse times ``strengths[f]`` and pasted into a copy of
    ``originals_u8``, which is never written.  Frames without a box or with strength <= 0 come back unchanged.  The result has the shape
    and the form of ``originals_u8``."""
    feather, color_match = _blend_settings(feather, color_match)
    boxes = _boxes(crop_boxes, *_peek(originals_u8, "originals"))
    strength = _strengths(strengths, len(boxes))
    x, back = _frames_in(originals_u8, "originals")
    F, H, W, _ = x.shape
    n_boxes = sum(b is not None for b in boxes)
    if n_boxes == 0 and (enhanced_u8 is None or len(enhanced_u8) == 0):
        e = torch.zeros((1, 1, 1, 3), dtype=torch.uint8, device=x.device)
    else:
        e, _ = _frames_in(enhanced_u8, "enhanced")
        if e.device != x.device:
            e = e.to(x.device)
    if e.shape[0] not in (n_boxes, F) and n_boxes:
        raise ValueError(f"enhanced must hold one frame per box ({n_boxes}) or per original frame ({F}), got {e.shape[0]}")
    per_box = e.shape[0] == n_boxes
    with torch.cuda.device(x.device):
        if F == 0:
            return back(torch.empty_like(x))
        plan = CompositePlan(x, e, boxes, strength, per_box, feather, color_match)
        plan.run_masks()
        plan.run_resize_stats()
        return back(plan.run_composite())


class CompositePlan:
    """The tables and buffers of one ``composite_frames`` call on device batches, and its three steps (``composite_frames`` runs them in
    order; tools/bench_facefix_builder.py times each).  ``boxes``: (left, top, w, h) or None per frame; ``strength``: clamped, per frame."""

    def __init__(self, x, e, boxes, strength, per_box, feather, color_match):
        self.x, self.e, self.feather, self.color_match = x, e, feather, color_match
        F, active = int(x.shape[0]), _active(boxes, strength)
        desc = np.zeros(F, dtype=_FF_DESC)
        self.spans, self.records, mask_offsets, self.mask_floats, self.largest, table, tap_offsets = _composite_tables(
            [a[2] for a in active], (int(e.shape[1]), int(e.shape[2])), feather)
        capacity = 0
        for f, index, (left, top, w, h), s in active:
            desc[f] = (index if per_box else f, left, top, w, h, s, mask_offsets[(w, h)], tap_offsets[(h, w)], capacity)
            capacity += w * h * 3
        self.capacity, self.n_taps, self.active = capacity, len(table), len(active)
        self.taps, self.desc = _upload(table, x.device), _upload(desc, x.device)
        self.face = torch.empty(max(capacity, 1), dtype=torch.uint8, device=x.device)
        self.stats = torch.empty(F * _hip.FACEFIX_STATS_WORDS, dtype=torch.int64, device=x.device)
        self.out = torch.empty_like(x)
        self.masks = None

    def run_masks(self):
        self.masks = _run_masks(self.spans, self.records, self.mask_floats, self.largest, self.feather, self.x.device)

    def run_resize_stats(self):
        x, e = self.x, self.e
        _hip.check(_hip.lib().vrg_ff_resize_stats_u8(_hip.ptr(x), _hip.ptr(e), _hip.ptr(self.masks), self.mask_floats, _hip.ptr(self.desc),
                                                     _hip.ptr(self.taps), self.n_taps, _hip.ptr(self.face), self.capacity, _hip.ptr(self.stats),
                                                     int(x.shape[0]), int(e.shape[0]), int(x.shape[1]), int(x.shape[2]), int(e.shape[1]),
                                                     int(e.shape[2]), self.largest if self.active else 0, self.color_match,
                                                     _hip.current_stream()), "vrg_ff_resize_stats_u8")

    def run_composite(self):
        x = self.x
        _hip.check(_hip.lib().vrg_ff_composite_u8(_hip.ptr(x), _hip.ptr(self.masks), self.mask_floats, _hip.ptr(self.desc), _hip.ptr(self.face),
                                                  self.capacity, _hip.ptr(self.stats), _hip.ptr(self.out), int(x.shape[0]), int(x.shape[1]),
                                                  int(x.shape[2]), _hip.current_stream()), "vrg_ff_composite_u8")
        return self.out


# ------------------------------------------------------------------------------------------------
# frames that stay on the host: only the boxes cross the bus (csrc/vrg_facefix_packed.hip)
# ------------------------------------------------------------------------------------------------
_PACKED_DESC = _hip.record_dtype(_hip.FaceFixPackedDesc)


class PackedPlan(_packed.BoxPack):
    """Host integers of one packed call, one entry per ACTIVE frame (a box, and strength > 0 where strengths are given), in frame order:
    ``frames`` the frame indices, ``box_index`` each one's position among the frames that have a box, ``boxes`` (left, top, w, h),
    ``strengths`` (clamped; 1.0 without strengths), ``offsets`` the byte offset of the box's dense [h][w][3] block in the packed buffers,
    ``tile_prefix`` int64 [n + 1]: 0 and the running sum of ceil(w * h / 256), ``tiles`` its last entry; ``n_boxes`` frames with a box.
    ``bytes_up`` = ``bytes_down`` = the bytes of all active boxes: what the composite moves each way for the originals (the repaired
    frames and the small tables go up besides; a crop brings n * S * S * 3 bytes down).  ``frame_bytes`` = frames * H * W * 3."""

    def __init__(self, frames, box_index, boxes, strengths, n_boxes, frame_bytes):
        super().__init__(frames, boxes, frame_bytes)
        self.box_index, self.strengths, self.n_boxes = box_index, strengths, n_boxes


def packed_plan(frames, height, width, crop_boxes, strengths=None) -> PackedPlan:
    """The plan of a packed call on ``frames`` frames of ``height`` x ``width``: ``crop_boxes`` as ``crop_frames`` takes them (the same
    ValueErrors), ``strengths`` as ``composite_frames`` takes them or None (a crop: every box is active).  No pixels, no device."""
    frames, height, width = int(frames), int(height), int(width)
    boxes = _boxes(crop_boxes, frames, height, width)
    used = _active(boxes, None if strengths is None else _strengths(strengths, frames))
    return PackedPlan(*([u[i] for u in used] for i in range(4)), sum(b is not None for b in boxes), frames * height * width * 3)


def last_transfer() -> dict:
    """The bytes the last packed call of this thread moved: ``bytes_up`` / ``bytes_down`` the boxes' pixels (the plan's counts; for a
    crop ``bytes_down`` is n * S * S * 3), ``enhanced_up`` the repaired frames, ``tables_up`` records and tables.  For tests and tools."""
    return _packed.last_transfer("enhanced_up")


def crop_frames_packed(frames_u8, crop_boxes, enhance_size):
    """``crop_frames`` for frames on the host (a CPU uint8 tensor or a list of numpy frames): the boxes are gathered into one page-locked
    buffer, uploaded once, resized in one launch and downloaded once -> ``[n, S, S, 3]`` in the caller's form.  Frames on the GPU
    (a CUDA tensor, DecodedFrames) raise TypeError: ``crop_frames`` keeps them there."""
    size = int(enhance_size)
    if size < 1:
        raise ValueError("enhance_size must be at least 1")
    arrays = _packed.host_arrays(frames_u8, "frames", "crop_frames")
    plan = packed_plan(*_peek(frames_u8, "frames"), crop_boxes)
    n, as_tensor = len(plan.frames), isinstance(frames_u8, torch.Tensor)
    if n == 0:
        _packed.note_transfer("enhanced_up")
        return torch.empty((0, size, size, 3), dtype=torch.uint8) if as_tensor else []
    stage = _packed.staging(plan.bytes_up)
    _pack_boxes(arrays, plan, stage.numpy())
    table, offsets = _tap_tables([(b[3], b[2]) for b in plan.boxes], lambda s: s, lambda s: (size, size))
    desc = np.zeros(n, dtype=_PACKED_DESC)
    for i, ((_, _, w, h), offset) in enumerate(zip(plan.boxes, plan.offsets)):
        desc[i] = (offset, 0, w, h, 0, 0.0, 0, offsets[(h, w)], 0)
    _hip.check(_host().vrg_ff_packed_check(C.c_void_p(desc.ctypes.data), n, None, plan.bytes_up, 0, 0, 0, len(table), 0, size, size),
               "vrg_ff_packed_check")
    device = compute_device()
    with torch.cuda.device(device):
        src = stage[:plan.bytes_up].to(device, non_blocking=True)
        taps, dev_desc = _upload(table, device), _upload(desc, device)
        out = torch.empty((n, size, size, 3), dtype=torch.uint8, device=device)
        _hip.check(_hip.lib().vrg_lanczos4_packed_u8(_hip.ptr(src), plan.bytes_up, _hip.ptr(dev_desc), n, _hip.ptr(out), size, size,
                                                     _hip.ptr(taps), len(table), _hip.current_stream()), "vrg_lanczos4_packed_u8")
        host = _packed.download(out)
    _packed.note_transfer("enhanced_up", bytes_up=plan.bytes_up, bytes_down=out.numel(), tables_up=table.nbytes + desc.nbytes)
    return host.clone() if as_tensor else list(host.numpy())


def composite_boxes_packed(originals_u8, enhanced_u8, crop_boxes, strengths, feather=DEFAULT_FEATHER, color_match=DEFAULT_COLOR_MATCH):
    """The pixels of ``composite_frames`` for frames on the host, boxes only: the active boxes of ``originals_u8`` and their repaired
    frames go up in one page-locked buffer, the composited boxes come down in one -> one ``[h, w, 3]`` array per active frame, in the
    order of ``packed_plan(...).frames`` (views of the download).  Nothing outside a box crosses the bus; no input is written."""
    feather, color_match = _blend_settings(feather, color_match)
    arrays = _packed.host_arrays(originals_u8, "originals", "composite_frames")
    F, H, W = _peek(originals_u8, "originals")
    plan = packed_plan(F, H, W, crop_boxes, strengths)
    n = len(plan.frames)
    if n == 0:
        _packed.note_transfer("enhanced_up")
        return []
    enhanced = _packed.host_arrays(enhanced_u8, "enhanced", "composite_frames")
    EF, EH, EW = _peek(enhanced_u8, "enhanced")
    if EF not in (plan.n_boxes, F):
        raise ValueError(f"enhanced must hold one frame per box ({plan.n_boxes}) or per original frame ({F}), got {EF}")
    picks = plan.box_index if EF == plan.n_boxes else plan.frames
    enh_bytes = EH * EW * 3
    starts = _packed.staged_layout(plan.bytes_up, [enh_bytes] * n)
    stage = _packed.staging(starts[-1])
    staged = stage.numpy()
    _pack_boxes(arrays, plan, staged)
    for pick, start in zip(picks, starts):                                  # the repaired frame of record i is frame i of the upload
        staged[start:start + enh_bytes].reshape(EH, EW, 3)[...] = enhanced[pick]
    spans, records, mask_offsets, mask_floats, largest, table, tap_offsets = _composite_tables(plan.boxes, (EH, EW), feather)
    desc = np.zeros(n, dtype=_PACKED_DESC)
    for i, ((_, _, w, h), offset, s) in enumerate(zip(plan.boxes, plan.offsets, plan.strengths)):
        desc[i] = (offset, offset, w, h, i, s, mask_offsets[(w, h)], tap_offsets[(h, w)], offset)
    total = plan.bytes_up
    _hip.check(_host().vrg_ff_packed_check(C.c_void_p(desc.ctypes.data), n, C.c_void_p(plan.tile_prefix.ctypes.data), total, total, n,
                                           mask_floats, len(table), total, 0, 0), "vrg_ff_packed_check")
    device = compute_device()
    with torch.cuda.device(device):
        dev = stage[:starts[-1]].to(device, non_blocking=True)
        src, enh = C.c_void_p(dev.data_ptr()), C.c_void_p(dev.data_ptr() + starts[0])
        dev_desc, prefix = _packed.upload_with_prefix(desc, plan.tile_prefix, device)
        taps = _upload(table, device)
        masks = _run_masks(spans, records, mask_floats, largest, feather, device)
        face = torch.empty(total, dtype=torch.uint8, device=device)
        stats = torch.empty(n * _hip.FACEFIX_STATS_WORDS, dtype=torch.int64, device=device)
        out = torch.empty(total, dtype=torch.uint8, device=device)
        lib, stream = _hip.lib(), _hip.current_stream()
        _hip.check(lib.vrg_ff_packed_resize_stats_u8(src, total, enh, n, EH, EW, _hip.ptr(masks), mask_floats, _hip.ptr(dev_desc), prefix, n,
                                                     plan.tiles, _hip.ptr(taps), len(table), _hip.ptr(face), total, _hip.ptr(stats), color_match,
                                                     stream), "vrg_ff_packed_resize_stats_u8")
        _hip.check(lib.vrg_ff_packed_composite_u8(src, total, _hip.ptr(masks), mask_floats, _hip.ptr(dev_desc), prefix, n, plan.tiles,
                                                  _hip.ptr(face), total, _hip.ptr(stats), _hip.ptr(out), total, stream),
                   "vrg_ff_packed_composite_u8")
        host = _packed.download(out).numpy()
    tables = desc.nbytes + plan.tile_prefix.nbytes + table.nbytes + spans.nbytes + records.nbytes + (4 * gauss_taps(feather) if feather > 0 else 0)
    _packed.note_transfer("enhanced_up", bytes_up=plan.bytes_up, bytes_down=plan.bytes_down, enhanced_up=n * enh_bytes, tables_up=tables)
    return plan.blocks(host)


def composite_frames_packed(originals_u8, enhanced_u8, crop_boxes, strengths, feather=DEFAULT_FEATHER, color_match=DEFAULT_COLOR_MATCH, *,
                            inplace=False):
    """``composite_frames`` for frames on the host: ``composite_boxes_packed`` pasted into a host copy of ``originals_u8`` (the
    reference's ``original.copy()``; the result has the originals' form), or -- ``inplace=True`` -- into the caller's own frames, which
    are returned.  ``originals_u8`` is never written unless ``inplace=True``."""
    _packed.host_arrays(originals_u8, "originals", "composite_frames")       # frames on the GPU are refused before anything else
    plan = packed_plan(*_peek(originals_u8, "originals"), crop_boxes, strengths)
    results = composite_boxes_packed(originals_u8, enhanced_u8, crop_boxes, strengths, feather, color_match)
    return _packed.paste_into_frames(originals_u8, plan, results, inplace)


# ------------------------------------------------------------------------------------------------
# the detector's input and its candidates, with the Builder's rules
# ------------------------------------------------------------------------------------------------
def _initial_regions(width, height):
    """``_initial_regions`` (:54-64): the whole frame and, from 600 x 400 up, four corner tiles of round(0.60 w) x round(0.70 h)"""
    from .VRGDG_StandaloneFaceFixNodes import scan_regions
    return scan_regions(width, height, builder=True)


def detection_plan(width, height, rotation_assist, regions=None):
    """VRGDG_StandaloneFaceFixNodes.detection_plan with the Builder's rules: angle 0 scans ``regions`` (None: the initial regions), every
    other angle the initial regions; ``rotation_assist`` is off / light / strong (None or unknown: light)."""
    from . import VRGDG_StandaloneFaceFixNodes as nodes
    return nodes.detection_plan(width, height, rotation_assist, regions=regions, builder=True)


def _as_batch(frames_u8):
    if isinstance(frames_u8, torch.Tensor):
        return frames_u8
    from .VRGDG_StandaloneVideoEnhancerNodes import DecodedFrames
    if isinstance(frames_u8, DecodedFrames):
        return frames_u8.u8
    return torch.from_numpy(np.stack([np.asarray(f) for f in frames_u8]))


def detector_blobs(frames_u8, plan, frames=None):
    """fp32 ``[F, A, R, 3, 300, 300]`` blobs of decoded B,G,R frames (a uint8 tensor on the GPU or the CPU, DecodedFrames, or a list of
    numpy frames); see VRGDG_StandaloneFaceFixNodes.detector_blobs."""
    from . import VRGDG_StandaloneFaceFixNodes as nodes
    return nodes.detector_blobs(_as_batch(frames_u8), plan, frames)


def rotated_frames(frames_u8, plan, frames=None):
    """uint8 ``[F, A, H, W, 3]``: the rotated frames the YuNet branch scans"""
    from . import VRGDG_StandaloneFaceFixNodes as nodes
    return nodes.rotated_frames(_as_batch(frames_u8), plan, frames)


def candidates_from_outputs(plan, outputs, confidence, kind="caffe"):
    """The candidates of one frame with the Builder's decode (round(), kept when x2 > x and y2 > y; ``_select_tracked`` applies
    ``minimum_pixels`` later); see VRGDG_StandaloneFaceFixNodes.candidates_from_outputs."""
    from . import VRGDG_StandaloneFaceFixNodes as nodes
    if not plan.builder:
        raise ValueError("candidates_from_outputs: the plan was not made by this module's detection_plan")
    return nodes.candidates_from_outputs(plan, outputs, confidence, 0, kind=kind)


def detect_with_rotation(forward=None, frames_u8=None, confidence=0.5, regions=None, rotation_assist="light", frames=None, chunk_frames=16):
    """``_detect_with_rotation(net, frame, confidence, regions, rotation_assist)`` for the frames of a decoded batch: one candidate list
    per frame.  ``forward(blobs) -> [n, 1, K, 7]`` is the network; None (the default) means no detector: no candidates, nothing computed."""
    from . import VRGDG_StandaloneFaceFixNodes as nodes
    return nodes.detect_with_rotation(forward, _as_batch(frames_u8), confidence, 0, rotation_assist, regions=regions, builder=True, frames=frames,
                                      chunk_frames=chunk_frames)

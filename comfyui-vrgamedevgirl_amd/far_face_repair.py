"""The pixels of the far-face repair backend (scripts/far_face_repair_backend.py of the reference) on the GPU, on decoded uint8 frames,
under the reference's names.

``expanded_square_crop`` / ``choose_face``   the host arithmetic of ``prepare`` (:154-199), unchanged.
``crop_frames``                              ``image.crop(box)`` per marked frame (:287): the crops, of their own sizes.
``soft_face_mask``                           :202-211 -- ``ImageDraw.ellipse`` (the outline is taken from Pillow on the host, two integers
                                             per row, cached per size) and ``ImageFilter.GaussianBlur`` (six byte box passes on the GPU).
``color_match_repaired``                     :214-224 -- the mean shift with numpy's sequential fp32 means over ``mask >= 64``.
``composite_frames``                         the loop body of ``composite`` (:349-366) for a batch: every repaired crop resized to its box
                                             with Pillow's LANCZOS, the mask, the optional colour match and ``Image.paste`` into a copy of
                                             the frame -- a handful of launches for the batch, no host round trip in between.
``pil_lanczos_resize``                       ``Image.resize(size, Image.Resampling.LANCZOS)`` for a batch of RGB or L images of any sizes.
``composite_frames_packed``                  the same for frames that stay on the HOST (a CPU tensor, numpy frames): only the boxes cross the
``composite_boxes_packed``                   bus -- the boxes of the originals and the repaired crops go up in one page-locked buffer, the
                                             composited boxes come down in one (csrc/vrg_farface_packed.hip); ``packed_plan`` gives the
                                             offsets and byte counts without a device, ``last_transfer`` what the last call moved.
``contact_sheet``                            :374-408 -- original and fixed frame side by side, ``Image.thumbnail`` (``Image.reduce`` and a
                                             BICUBIC resize over the fractional box) and the paste into the cells of the sheet: two launches.
``pil_thumbnail`` / ``pil_reduce``           ``Image.thumbnail`` and ``Image.reduce`` for a batch of RGB images of any sizes, on the same kernels.

Every step equals Pillow / numpy byte for byte (csrc/vrg_pil_math.hpp).  The channel order is the caller's: the arithmetic treats the three
channels alike.  Device-resident inputs stay on the device; CPU inputs of ``composite_frames`` are uploaded whole and the result comes back in
the form the frames came in -- ``composite_frames_packed`` moves the boxes alone.  Detection, PNG / video / JPEG I/O, manifests and
``rebuild_video`` are out of scope.  The library is reached through ``_hip`` only; Pillow is needed for the ellipse outline alone.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from . import _hip, _packed, ops
from ._devices import compute_device
from ._packed import frame_boxes as _boxes, frames_in as _frames_in, peek as _peek

NODE_CLASS_MAPPINGS = {}
NODE_DISPLAY_NAME_MAPPINGS = {}

DEFAULT_FEATHER = 18
COLOR_MATCH_STRENGTH = 0.65
MAX_FEATHER = 4096

FaceBox = namedtuple("FaceBox", "x y w h score")

_RESIZE_DESC = _hip.record_dtype(_hip.PilResizeDesc)
_MASK_DESC = _hip.record_dtype(_hip.PilMaskDesc)
_BOX_DESC = _hip.record_dtype(_hip.PilBoxDesc)
_THUMB_ENTRY = _hip.record_dtype(_hip.ThumbEntry)
_PACKED_DESC = _hip.record_dtype(_hip.PilPackedDesc)
_host = _hip.host_library       # the library for its HOST table functions (no GPU needed)
_upload = _hip.upload_records   # records and the byte / int32 tables that go with them

SHEET_CANVAS = (24, 24, 24)
NO_FRAMES = "No frames were available for the contact sheet."
_FILTERS = {"bicubic": _hip.PIL_FILTER_BICUBIC, "lanczos": _hip.PIL_FILTER_LANCZOS}


# ------------------------------------------------------------------------------------------------
# host arithmetic of `prepare`
# ------------------------------------------------------------------------------------------------
def choose_face(faces, width, height, mode):
    """the face ``prepare`` keeps (:154-169): the largest, slightly favouring the centre, or (mode "center") the most central"""
    if not faces:
        return None
    center_x, center_y = width / 2.0, height / 2.0

    def score(face):
        area = face.w * face.h
        dist = math.hypot((face.x + face.w / 2.0 - center_x) / width, (face.y + face.h / 2.0 - center_y) / height)
        return -dist if mode == "center" else area - dist * area * 0.15

    return max(faces, key=score)


def expanded_square_crop(face, image_width, image_height, padding):
    """(left, top, right, bottom) of the padded square around a face (:172-199), at least 32 px, pushed back inside the image"""
    cx, cy = face.x + face.w / 2.0, face.y + face.h / 2.0
    side = max(max(face.w, face.h) * float(padding), 32.0)
    left, top = int(round(cx - side / 2.0)), int(round(cy - side / 2.0))
    right, bottom = int(round(cx + side / 2.0)), int(round(cy + side / 2.0))
    if left < 0:
        left, right = 0, right - left
    if top < 0:
        top, bottom = 0, bottom - top
    if right > image_width:
        left, right = left - (right - image_width), image_width
    if bottom > image_height:
        top, bottom = top - (bottom - image_height), image_height
    left, top = max(0, left), max(0, top)
    return left, top, min(image_width, max(left + 1, right)), min(image_height, max(top + 1, bottom))


# ------------------------------------------------------------------------------------------------
# host tables
# ------------------------------------------------------------------------------------------------
def lanczos_table(n_in: int, n_out: int):
    """(ksize, one axis table as the kernels read it: bounds [n_out, 2] then weights [n_out, ksize], int32); host only"""
    return ops.pil_axis_table(_hip.PIL_FILTER_LANCZOS, n_in, n_out)


def _filter_number(resample):
    key = resample.lower() if isinstance(resample, str) else {v: k for k, v in _FILTERS.items()}.get(int(resample))
    if key not in _FILTERS:
        raise ValueError(f"resample must be one of {sorted(_FILTERS)}, got {resample!r}")
    return _FILTERS[key]


def _host_check(status, what):
    if status == _hip.VRG_OK:
        return
    msg = _host().vrg_error_string(status).decode()
    raise (ValueError if status == 1 else RuntimeError)(f"{what}: {msg}")


def filter_table(resample, n_in: int, in0: float, in1: float, n_out: int):
    """(ksize, one axis table as the kernels read it) of ``Image.resize(.., resample, box)``: ``n_out`` outputs from the source interval
    [in0, in1) of an axis of ``n_in`` pixels; ``resample`` "bicubic" or "lanczos".  The interval is rounded to C float, as Pillow takes it.
    Host only."""
    return ops.pil_axis_table(_filter_number(resample), int(n_in), int(n_out), (float(np.float32(in0)), float(np.float32(in1))))


@functools.lru_cache(maxsize=64)
def box_parameters(feather: int):
    """(radius, ww, fw) of one box pass of ``GaussianBlur(radius=float(feather))``; host only"""
    out = np.zeros(3, dtype=np.int32)
    _hip.check(_host().vrg_pil_box_parameters(float(feather), C.c_void_p(out.ctypes.data)), "vrg_pil_box_parameters")
    return int(out[0]), int(out.view(np.uint32)[1]), int(out.view(np.uint32)[2])


@functools.lru_cache(maxsize=512)
def ellipse_spans(width: int, height: int, shrink: float = 0.12) -> np.ndarray:
    """[height, 2] int32: the first and last column ``ImageDraw.ellipse`` sets in every row of the mask (first > last: none) -- from
    Pillow itself; every row of the outline is one run"""
    from PIL import Image, ImageDraw
    if width < 1 or height < 1:
        raise ValueError("ellipse_spans: width and height must be at least 1")
    inset_x, inset_y = int(round(width * shrink)), int(round(height * shrink))
    mask = Image.new("L", (width, height), 0)
    ImageDraw.Draw(mask).ellipse((inset_x, inset_y, width - inset_x, height - inset_y), fill=255)
    plane = np.asarray(mask) != 0
    any_set = plane.any(axis=1)
    first = plane.argmax(axis=1)
    last = width - 1 - plane[:, ::-1].argmax(axis=1)
    if int(plane.sum()) != int((last - first + 1)[any_set].sum()):
        raise RuntimeError("ellipse_spans: a row of Pillow's ellipse is not one run")
    spans = np.where(any_set[:, None], np.stack([first, last], axis=1), np.array([[1, 0]])).astype(np.int32)
    spans.setflags(write=False)
    return spans


# ------------------------------------------------------------------------------------------------
# images in, images out
# ------------------------------------------------------------------------------------------------
def _image_list(images, name, channels=None):
    """-> (a list of uint8 [h, w, c] / [h, w] tensors or arrays, c) of a batch given as a tensor or a sequence"""
    items = list(images) if not isinstance(images, (torch.Tensor, np.ndarray)) else [images[i] for i in range(images.shape[0])]
    c = channels
    for item in items:
        if item is None:
            continue
        dtype_ok = item.dtype == (torch.uint8 if isinstance(item, torch.Tensor) else np.uint8)
        k = 1 if item.ndim == 2 else int(item.shape[-1]) if item.ndim == 3 else 0
        if not dtype_ok or k not in (1, 3) or (item.ndim == 3 and k == 1 and channels is None):
            raise ValueError(f"{name} must be uint8 images of shape [h, w, 3] or [h, w]")
        if c is None:
            c = k
        if k != c:
            raise ValueError(f"{name} must be uint8 images of {c} channel(s), got {k}")
        if item.shape[0] < 1 or item.shape[1] < 1:
            raise ValueError(f"{name} must not hold an empty image")
    return items, c


def _pack(items, device):
    """the bytes of the images back to back on the device -> (buffer, [offset per image])"""
    offsets, total = [], 0
    for item in items:
        offsets.append(total)
        total += int(np.prod(item.shape))
    if all(isinstance(i, torch.Tensor) and i.is_cuda for i in items) and items:
        buf = torch.cat([i.to(device).contiguous().reshape(-1) for i in items])
    elif items:
        buf = torch.from_numpy(np.concatenate([np.ascontiguousarray(i.cpu().numpy() if isinstance(i, torch.Tensor) else i).reshape(-1)
                                               for i in items])).to(device)
    else:
        buf = torch.zeros(1, dtype=torch.uint8, device=device)
    return buf, offsets


class ResizePlan:
    """``Image.resize(out_size, LANCZOS)`` of a packed batch: sizes[i] = (in_w, in_h, out_w, out_h) -> ``dst`` and ``offsets``"""

    def __init__(self, src, src_offsets, sizes, channels, device):
        self.src, self.channels = src, channels
        desc = np.zeros(len(sizes), dtype=_RESIZE_DESC)
        tables, table_at, n_ints, dst_bytes, tmp_bytes, self.max_pixels = [], {}, 0, 0, 0, 0
        self.offsets = []
        for i, (iw, ih, ow, oh) in enumerate(sizes):
            at, ks = [0, 0], [0, 0]
            for axis, (n_in, n_out) in enumerate(((iw, ow), (ih, oh))):
                if n_in == n_out:
                    continue
                if (n_in, n_out) not in table_at:
                    ksize, table = lanczos_table(n_in, n_out)
                    table_at[(n_in, n_out)] = (n_ints, ksize)
                    tables.append(table)
                    n_ints += len(table)
                at[axis], ks[axis] = table_at[(n_in, n_out)]
            desc[i] = (src_offsets[i], dst_bytes, tmp_bytes, at[0], at[1], iw, ih, ow, oh, ks[0], ks[1])
            self.offsets.append(dst_bytes)
            dst_bytes += ow * oh * channels
            if iw != ow and ih != oh:
                tmp_bytes += ih * ow * channels
            self.max_pixels = max(self.max_pixels, ih * ow, oh * ow)
        self.n, self.n_ints, self.dst_bytes, self.tmp_bytes = len(sizes), n_ints, dst_bytes, tmp_bytes
        self.tables = _upload(np.concatenate(tables) if tables else np.zeros(1, np.int32), device)
        self.desc = _upload(desc, device) if len(sizes) else None
        self.dst = torch.empty(max(dst_bytes, 1), dtype=torch.uint8, device=device)
        self.tmp = torch.empty(max(tmp_bytes, 1), dtype=torch.uint8, device=device)

    def run(self):
        if self.n:
            _hip.check(_hip.lib().vrg_pil_resize_u8(_hip.ptr(self.src), self.src.numel(), _hip.ptr(self.desc), self.n, self.channels,
                                                    _hip.ptr(self.tables), self.n_ints, _hip.ptr(self.tmp), self.tmp_bytes, _hip.ptr(self.dst),
                                                    self.dst_bytes, self.max_pixels, _hip.current_stream()), "vrg_pil_resize_u8")
        return self.dst


def pil_lanczos_resize(images_u8, size):
    """``Image.resize(size, Image.Resampling.LANCZOS)`` (size = (width, height)) of every image of a batch: a uint8 tensor [n, h, w, 3] /
    [n, h, w] or a sequence of [h, w, 3] / [h, w] images of any sizes -> [n, height, width(, 3)] uint8, on the GPU for a CUDA tensor or a
    sequence of them, else on the CPU (a list of arrays for a sequence of arrays)."""
    width, height = int(size[0]), int(size[1])
    if width < 1 or height < 1:
        raise ValueError("size must be at least 1 x 1")
    items, c = _image_list(images_u8, "images")
    flat = bool(items) and items[0].ndim == 2
    shape = (len(items), height, width) + (() if flat else (c or 3,))
    on_device = isinstance(images_u8, torch.Tensor) and images_u8.is_cuda or (bool(items) and all(isinstance(i, torch.Tensor) and i.is_cuda for i in items))
    device = items[0].device if on_device and items else compute_device()
    if not items:
        return torch.empty(shape, dtype=torch.uint8)
    with torch.cuda.device(device):
        src, offsets = _pack(items, device)
        plan = ResizePlan(src, offsets, [(int(i.shape[1]), int(i.shape[0]), width, height) for i in items], c, device)
        out = plan.run()[:plan.dst_bytes].reshape(shape)
        if on_device:
            return out
        out = out.cpu()
        return out if isinstance(images_u8, torch.Tensor) or isinstance(items[0], torch.Tensor) else list(out.numpy())


def crop_frames(frames_u8, crop_boxes):
    """``image.crop((left, top, right, bottom))`` for every frame that has a box (``crop_boxes``: one box or None per frame): the crops in
    the order of the frames, each of its own size -- CUDA tensors for CUDA frames, CPU tensors for a CPU tensor, arrays for arrays."""
    frames, height, width = _peek(frames_u8, "frames")
    boxes = _boxes(crop_boxes, frames, height, width)
    t = getattr(frames_u8, "u8", frames_u8)
    out = []
    for f, box in enumerate(boxes):
        if box is None:
            continue
        left, top, w, h = box
        crop = t[f][top:top + h, left:left + w]
        out.append(crop.clone() if isinstance(crop, torch.Tensor) else np.array(crop, copy=True))
    return out


# ------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------
def _check_feather(feather):
    feather = int(feather)
    if feather > MAX_FEATHER:
        raise ValueError(f"feather must not exceed {MAX_FEATHER}")
    return feather


class MaskPlan:
    """the soft-ellipse masks of the distinct (w, h) of a batch, packed -> ``masks`` and ``offsets[(w, h)]``"""

    def __init__(self, sizes, feather, device, shrink=0.12):
        self.offsets, spans, records, total, rows = {}, [], [], 0, 0
        radius, ww, fw = box_parameters(feather) if feather > 0 else (-1, 0, 0)
        for w, h in sizes:
            if (w, h) in self.offsets:
                continue
            if w > _hip.PIL_MAX_LINE or h > _hip.PIL_MAX_LINE:
                raise ValueError(f"a mask of {w} x {h} exceeds {_hip.PIL_MAX_LINE} pixels a side")
            self.offsets[(w, h)] = total
            spans.append(ellipse_spans(w, h, shrink))
            records.append((w, h, radius, ww, fw, 0, rows, total))
            rows += h
            total += w * h
        self.n, self.total, self.rows = len(records), total, rows
        self.max_w, self.max_h = max([r[0] for r in records] or [0]), max([r[1] for r in records] or [0])
        self.spans = _upload(np.concatenate(spans) if spans else np.zeros((1, 2), np.int32), device)
        self.records = _upload(np.array(records, dtype=_MASK_DESC), device) if records else None
        self.masks = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
        self.scratch = torch.empty(max(total, 1), dtype=torch.uint8, device=device)

    def run(self):
        if self.n:
            _hip.check(_hip.lib().vrg_pil_mask_u8(_hip.ptr(self.spans), self.rows, _hip.ptr(self.records), self.n, self.max_w, self.max_h,
                                                  _hip.ptr(self.scratch), _hip.ptr(self.masks), self.total, _hip.current_stream()),
                       "vrg_pil_mask_u8")
        return self.masks


def soft_face_mask(size, feather, shrink=0.12) -> np.ndarray:
    """``soft_face_mask(size, feather, shrink)`` of the reference (:202-211) as a uint8 ``[height, width]`` array, made on the GPU"""
    width, height = int(size[0]), int(size[1])
    if width < 1 or height < 1:
        raise ValueError("mask width and height must be at least 1")
    feather = _check_feather(feather)
    device = compute_device()
    with torch.cuda.device(device):
        plan = MaskPlan([(width, height)], feather, device, float(shrink))
        return plan.run()[:width * height].cpu().numpy().reshape(height, width)


# ------------------------------------------------------------------------------------------------
# the composite
# ------------------------------------------------------------------------------------------------
def _per_box(values, boxes, name):
    """the entries of `values` that belong to the frames with a box: one per box, or one per frame (None allowed where there is no box)"""
    n_boxes = sum(b is not None for b in boxes)
    items = list(values) if not isinstance(values, (torch.Tensor, np.ndarray)) else [values[i] for i in range(values.shape[0])]
    if len(items) == n_boxes:
        picked = items
    elif len(items) == len(boxes):
        picked = [v for v, b in zip(items, boxes) if b is not None]
    else:
        raise ValueError(f"{name} must hold one image per box ({n_boxes}) or per frame ({len(boxes)}), got {len(items)}")
    if any(v is None for v in picked):
        raise ValueError(f"{name} has no image for a frame that has a box")
    return picked


class CompositePlan:
    """The tables and buffers of one ``composite_frames`` call on a device batch, and its steps (``composite_frames`` runs them in order;
    tools/bench_far_face.py times each).  ``boxes``: (left, top, w, h) or None per frame; ``repaired`` / ``masks``: one image per box."""

    def __init__(self, x, boxes, repaired, feather, color_match, masks=None):
        device = x.device
        self.x, self.color_match = x, bool(color_match)
        used = [(f, b) for f, b in enumerate(boxes) if b is not None]
        src, offsets = _pack(repaired, device)
        msrc, moffsets = _pack(masks, device) if feather < 0 else (None, None)
        mask_offsets = self._plans([b for _, b in used], feather, device, repaired, src, offsets, masks, msrc, moffsets)
        desc = np.zeros(int(x.shape[0]), dtype=_BOX_DESC)
        for k, (f, (left, top, w, h)) in enumerate(used):
            desc[f] = (left, top, w, h, int(self.color_match), 0, mask_offsets[k], self.resize.offsets[k])
        self.desc = _upload(desc, device)
        self.stats = torch.zeros(int(x.shape[0]) * _hip.PIL_STATS_WORDS, dtype=torch.int32, device=device)
        self.out = torch.empty_like(x)
        self.rep = self.masks = None

    def _plans(self, boxes, feather, device, repaired, src, offsets, masks, msrc, moffsets):
        """the resize of the crops (`repaired[k]` at ``offsets[k]`` of the device buffer ``src``) and the masks of ``boxes`` -- fresh, or the
        saved ones (``masks[k]`` at ``moffsets[k]`` of ``msrc``) resized as L -> the mask's offset per box"""
        self.resize = ResizePlan(src, offsets, [(int(r.shape[1]), int(r.shape[0]), b[2], b[3]) for r, b in zip(repaired, boxes)], 3, device)
        if feather >= 0:
            self.mask_plan, self.mask_resize = MaskPlan([(b[2], b[3]) for b in boxes], feather, device), None
            self.mask_bytes = self.mask_plan.total
            return [self.mask_plan.offsets[(b[2], b[3])] for b in boxes]
        self.mask_plan = None
        self.mask_resize = ResizePlan(msrc, moffsets, [(int(m.shape[1]), int(m.shape[0]), b[2], b[3]) for m, b in zip(masks, boxes)], 1, device)
        self.mask_bytes = self.mask_resize.dst_bytes
        return self.mask_resize.offsets

    def run_resize(self):
        self.rep = self.resize.run()

    def run_masks(self):
        self.masks = self.mask_plan.run() if self.mask_plan is not None else self.mask_resize.run()

    def _args(self):
        x = self.x
        return (_hip.ptr(x), _hip.ptr(self.rep), self.resize.dst_bytes, _hip.ptr(self.masks), self.mask_bytes, _hip.ptr(self.desc),
                _hip.ptr(self.stats))

    def run_means(self):
        if self.color_match:
            self._means(_hip.current_stream())

    def run_paste(self):
        return self._paste(_hip.current_stream())

    # what the two steps launch on the stream they are handed: PackedCompositePlan launches the packed kernels instead
    def _means(self, stream):
        x = self.x
        _hip.check(_hip.lib().vrg_np_masked_means_f32(*self._args(), int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), COLOR_MATCH_STRENGTH,
                                                      stream), "vrg_np_masked_means_f32")

    def _paste(self, stream):
        x = self.x
        _hip.check(_hip.lib().vrg_pil_paste_u8(*self._args(), _hip.ptr(self.out), int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), stream),
                   "vrg_pil_paste_u8")
        return self.out


def _prepare(originals_u8, repaired, crop_boxes, feather, masks):
    feather = _check_feather(feather)
    boxes = _boxes(crop_boxes, *_peek(originals_u8, "originals"))
    rep, _ = _image_list(_per_box(repaired, boxes, "repaired"), "repaired", 3)
    if any(r.ndim != 3 for r in rep):
        raise ValueError("repaired must be uint8 images of shape [h, w, 3]")
    mk = None
    if feather < 0:
        if masks is None:
            raise ValueError("feather < 0 keeps the saved masks: masks must be given")
        mk, _ = _image_list(_per_box(masks, boxes, "masks"), "masks", 1)
        mk = [m[:, :, 0] if m.ndim == 3 else m for m in mk]
    return feather, boxes, rep, mk


def composite_frames(originals_u8, repaired, crop_boxes, feather=DEFAULT_FEATHER, color_match=False, masks=None):
    """The loop body of ``composite`` for a batch: ``repaired`` (one RGB crop of any size per box in the order of the frames, or one entry
    per frame) resized to its box with LANCZOS, colour matched if asked, and pasted under the mask into a copy of ``originals_u8``, which is
    never written.  ``feather >= 0`` makes a fresh soft ellipse per box (0: unblurred); ``feather < 0`` keeps ``masks`` (uint8 [h, w] images
    of any sizes, one per box), LANCZOS-resized as L.  Frames without a box come back unchanged.  The result has the shape and the form of
    ``originals_u8`` (CUDA tensor, CPU tensor, list of numpy frames)."""
    feather, boxes, rep, mk = _prepare(originals_u8, repaired, crop_boxes, feather, masks)
    x, back = _frames_in(originals_u8, "originals")
    with torch.cuda.device(x.device):
        if x.shape[0] == 0:
            return back(torch.empty_like(x))
        plan = CompositePlan(x, boxes, rep, feather, color_match, mk)
        plan.run_resize()
        plan.run_masks()
        plan.run_means()
        return back(plan.run_paste())


def color_match_repaired(original, repaired, mask) -> np.ndarray:
    """``color_match_repaired(original, repaired, mask)`` of the reference (:214-224) on uint8 arrays of one size ([h, w, 3], [h, w, 3],
    [h, w]) -> the adjusted [h, w, 3] array (the repaired bytes themselves when fewer than 16 pixels are selected), made on the GPU"""
    original, repaired, mask = (np.ascontiguousarray(a) for a in (original, repaired, mask))
    if original.dtype != np.uint8 or original.ndim != 3 or original.shape[2] != 3 or repaired.shape != original.shape or \
            repaired.dtype != np.uint8 or mask.dtype != np.uint8 or mask.shape != original.shape[:2]:
        raise ValueError("color_match_repaired: original and repaired must be [h, w, 3] uint8 of one size, mask [h, w] uint8")
    h, w = mask.shape
    device = compute_device()
    with torch.cuda.device(device):
        # the shift alone: pasted under a mask of 255 everywhere the result is the shifted crop
        plan = CompositePlan(torch.from_numpy(original[None]).to(device), [(0, 0, w, h)], [repaired], -1, True, [mask])
        plan.run_resize()
        plan.run_masks()
        plan.run_means()
        plan.masks = torch.full_like(plan.masks, 255)
        return plan.run_paste()[0].cpu().numpy()


def masked_means(original, repaired, mask) -> dict:
    """the record of the means kernel for one box (arrays as for ``color_match_repaired``): count, original_mean, repaired_mean, shift
    (float32 [3] each) and matched"""
    original, repaired, mask = (np.ascontiguousarray(a) for a in (original, repaired, mask))
    h, w = mask.shape
    device = compute_device()
    with torch.cuda.device(device):
        plan = CompositePlan(torch.from_numpy(original[None]).to(device), [(0, 0, w, h)], [repaired], -1, True, [mask])
        plan.run_resize()
        plan.run_masks()
        plan.run_means()
        rec = plan.stats.cpu().numpy().view(np.uint32)[:_hip.PIL_STATS_WORDS]
    return {"count": int(rec[0]), "original_mean": rec[1:4].view(np.float32).copy(), "repaired_mean": rec[4:7].view(np.float32).copy(),
            "shift": rec[7:10].view(np.float32).copy(), "matched": bool(rec[10])}


# ------------------------------------------------------------------------------------------------
# frames that stay on the host: only the boxes cross the bus (csrc/vrg_farface_packed.hip)
# ------------------------------------------------------------------------------------------------
PackedPlan = _packed.BoxPack        # one entry per frame that has a box; the repaired crops and the small tables go up besides


def packed_plan(frames, height, width, crop_boxes) -> PackedPlan:
    """The plan of a packed call on ``frames`` frames of ``height`` x ``width``: ``crop_boxes`` as ``composite_frames`` takes them (the
    same ValueErrors).  No pixels, no device."""
    frames, height, width = int(frames), int(height), int(width)
    boxes = _boxes(crop_boxes, frames, height, width)
    used = [(f, b) for f, b in enumerate(boxes) if b is not None]
    return PackedPlan([f for f, _ in used], [b for _, b in used], frames * height * width * 3)


def last_transfer() -> dict:
    """The bytes the last packed call of this thread moved: ``bytes_up`` / ``bytes_down`` the boxes' pixels (the plan's counts),
    ``repaired_up`` the repaired crops (and the saved masks), ``tables_up`` records and tables.  For tests and tools."""
    return _packed.last_transfer("repaired_up")


class PackedCompositePlan(CompositePlan):
    """``CompositePlan`` on ONE upload ``dev`` (uint8, on the device): the boxes of ``plan`` as dense blocks from byte 0, the repaired crops
    ``repaired[k]`` at ``rep_at + offsets[k]`` and -- ``feather < 0`` -- the saved masks ``masks[k]`` at ``mask_at + moffsets[k]``.  The
    resize and the masks read views of that upload; the means and the paste are the packed kernels, on the stream ``run_means`` /
    ``run_paste`` hand them."""

    def __init__(self, dev, plan, repaired, feather, color_match, rep_at, offsets, masks, mask_at, moffsets):
        device, total = dev.device, plan.bytes_up
        self.x, self.color_match, self.plan, self.total = dev[:total], bool(color_match), plan, total
        mask_offsets = self._plans(plan.boxes, feather, device, repaired, dev[rep_at:mask_at], offsets, masks, dev[mask_at:], moffsets)
        desc = np.zeros(len(plan.boxes), dtype=_PACKED_DESC)
        for k, ((_, _, w, h), offset) in enumerate(zip(plan.boxes, plan.offsets)):
            desc[k] = (offset, offset, w, h, int(self.color_match), 0, mask_offsets[k], self.resize.offsets[k])
        _host_check(_host().vrg_pil_packed_check(C.c_void_p(desc.ctypes.data), len(desc), C.c_void_p(plan.tile_prefix.ctypes.data), total,
                                                 self.resize.dst_bytes, self.mask_bytes, total), "vrg_pil_packed_check")
        self.desc, self.prefix = _packed.upload_with_prefix(desc, plan.tile_prefix, device)
        self.stats = torch.zeros(len(desc) * _hip.PIL_STATS_WORDS, dtype=torch.int32, device=device)
        self.out = torch.empty(total, dtype=torch.uint8, device=device)
        self.rep = self.masks = None

    def tables_up(self):
        parts = [self.desc, self.resize.tables, self.resize.desc] + \
                ([self.mask_plan.spans, self.mask_plan.records] if self.mask_plan is not None else [self.mask_resize.tables, self.mask_resize.desc])
        return int(sum(t.numel() * t.element_size() for t in parts if t is not None))

    def _packed(self):
        return (_hip.ptr(self.x), self.total, _hip.ptr(self.rep), self.resize.dst_bytes, _hip.ptr(self.masks), self.mask_bytes, _hip.ptr(self.desc))

    def _means(self, stream):
        _hip.check(_hip.lib().vrg_np_packed_masked_means_f32(*self._packed(), _hip.ptr(self.stats), len(self.plan.boxes), COLOR_MATCH_STRENGTH,
                                                             stream), "vrg_np_packed_masked_means_f32")

    def _paste(self, stream):
        _hip.check(_hip.lib().vrg_pil_packed_paste_u8(*self._packed(), self.prefix, len(self.plan.boxes), self.plan.tiles, _hip.ptr(self.stats),
                                                      _hip.ptr(self.out), self.total, stream), "vrg_pil_packed_paste_u8")
        return self.out


def _host_images(images):
    """the CPU images of a batch (tensors or arrays) as dense numpy arrays"""
    return [np.ascontiguousarray(i.numpy() if isinstance(i, torch.Tensor) else i) for i in images]


def _on_gpu(values):
    """is a batch of crops or masks (a tensor, or a sequence of images) on the GPU, or any image of it?"""
    if hasattr(values, "u8") or (isinstance(values, torch.Tensor) and values.is_cuda):
        return True
    return not isinstance(values, (torch.Tensor, np.ndarray)) and any(isinstance(v, torch.Tensor) and v.is_cuda for v in values)


def composite_boxes_packed(originals_u8, repaired, crop_boxes, feather=DEFAULT_FEATHER, color_match=False, masks=None):
    """The pixels of ``composite_frames`` for frames on the host (a CPU uint8 tensor [F, H, W, 3] or a list of numpy frames of one size),
    boxes only: the boxes of ``originals_u8``, the repaired crops and -- ``feather < 0`` -- the saved masks go up in one page-locked
    buffer, the composited boxes come down in one -> one ``[h, w, 3]`` array per frame with a box, in the order of
    ``packed_plan(...).frames`` (views of the download).  ``repaired`` / ``masks`` as ``composite_frames`` takes them.  Nothing outside a
    box crosses the bus; no input is written.  Frames or crops on the GPU raise TypeError: ``composite_frames`` keeps them there."""
    arrays = _packed.host_arrays(originals_u8, "originals", "composite_frames")
    for values, name in ((repaired, "repaired"), (masks, "masks")):
        if values is not None and _on_gpu(values):
            raise TypeError(f"{name} is on the GPU already: the packed route is for decoded frames on the host, use composite_frames")
    feather, _, rep, mk = _prepare(originals_u8, repaired, crop_boxes, feather, masks)
    plan = packed_plan(*_peek(originals_u8, "originals"), crop_boxes)
    if not plan.frames:
        _packed.note_transfer("repaired_up")
        return []
    rep, mk = _host_images(rep), (_host_images(mk) if mk is not None else None)
    starts = _packed.staged_layout(plan.bytes_up, [r.size for r in rep] + [m.size for m in mk or []])
    rep_at, mask_at = starts[0], starts[len(rep)]
    stage = _packed.staging(starts[-1])
    staged = stage.numpy()
    _packed.pack_boxes(arrays, plan, staged)
    for image, start in zip(rep + (mk or []), starts):
        staged[start:start + image.size] = image.reshape(-1)
    device = compute_device()
    with torch.cuda.device(device):
        dev = stage[:starts[-1]].to(device, non_blocking=True)
        work = PackedCompositePlan(dev, plan, rep, feather, color_match, rep_at, [s - rep_at for s in starts[:len(rep)]], mk, mask_at,
                                   [s - mask_at for s in starts[len(rep):-1]])
        work.run_resize()
        work.run_masks()
        work.run_means()
        host = _packed.download(work.run_paste()).numpy()
    _packed.note_transfer("repaired_up", bytes_up=plan.bytes_up, bytes_down=plan.bytes_down, repaired_up=starts[-1] - rep_at,
                          tables_up=work.tables_up())
    return plan.blocks(host)


def composite_frames_packed(originals_u8, repaired, crop_boxes, feather=DEFAULT_FEATHER, color_match=False, masks=None, *, inplace=False):
    """``composite_frames`` for frames on the host: ``composite_boxes_packed`` pasted into a host copy of ``originals_u8`` (the
    reference's ``original.copy()``; the result has the originals' form), or -- ``inplace=True`` -- into the caller's own frames, which
    are returned.  ``originals_u8`` is never written unless ``inplace=True``."""
    _packed.host_arrays(originals_u8, "originals", "composite_frames")       # frames on the GPU are refused before anything else
    plan = packed_plan(*_peek(originals_u8, "originals"), crop_boxes)
    results = composite_boxes_packed(originals_u8, repaired, crop_boxes, feather, color_match, masks)
    return _packed.paste_into_frames(originals_u8, plan, results, inplace)


# ------------------------------------------------------------------------------------------------
# the contact sheet
# ------------------------------------------------------------------------------------------------
def _sources(items, device):
    """the images as one source buffer -> (first byte, bytes, [offset per image], what keeps it alive): device images are read where they
    lie (a dense view stays a view, at any byte address), anything else is packed and uploaded"""
    if all(isinstance(i, torch.Tensor) and i.is_cuda and i.device == device for i in items):
        kept = [i if i.is_contiguous() else i.contiguous() for i in items]
        base = min(k.data_ptr() for k in kept)
        return base, max(k.data_ptr() + k.numel() for k in kept) - base, [k.data_ptr() - base for k in kept], kept
    buf, offsets = _pack(items, device)
    return buf.data_ptr(), buf.numel(), offsets, buf


class ThumbPlan:
    """The entries, tables and buffers of one sheet of thumbnails on ``device`` and its two launches (``contact_sheet`` and
    ``pil_thumbnail`` run them in order; tools/bench_contact_sheet.py times each).  ``lefts``: one RGB image per entry; ``rights``: None or
    one image or None per entry (an image makes the entry a pair); ``requests``: the (width, height) asked of ``Image.thumbnail`` per entry,
    or None with ``factors`` = (fx, fy): ``Image.reduce`` alone."""

    def __init__(self, lefts, rights, requests, device, resample="bicubic", reducing_gap=2.0, columns=1, factors=None):
        number = _filter_number(resample)
        n = len(lefts)
        rights = list(rights) if rights is not None else [None] * n
        images = list(lefts) + [r for l, r in zip(lefts, rights) if r is not None and r is not l]
        self.base, self.src_bytes, offsets, self._kept = _sources(images, device)
        entries = np.zeros(n, dtype=_THUMB_ENTRY)
        k = n
        for i, (left, right) in enumerate(zip(lefts, rights)):
            e = entries[i]
            e["left_offset"], e["left_h"], e["left_w"], e["right_offset"] = offsets[i], left.shape[0], left.shape[1], -1
            if right is not None:
                e["right_offset"], e["right_h"], e["right_w"] = offsets[i if right is left else k], right.shape[0], right.shape[1]
                k += right is not left
        sheet = np.zeros(5, dtype=np.int64)
        if factors is None:
            if reducing_gap is not None and not float(reducing_gap) >= 1.0:
                raise ValueError("reducing_gap must be 1.0 or greater")
            req = np.ascontiguousarray(np.asarray(requests, dtype=np.float64).reshape(n, 2))
            _host_check(_host().vrg_thumb_plan(C.c_void_p(entries.ctypes.data), n, C.c_void_p(req.ctypes.data), number,
                                               0.0 if reducing_gap is None else float(reducing_gap), int(columns),
                                               C.c_void_p(sheet.ctypes.data)), "vrg_thumb_plan")
        else:
            _host_check(_host().vrg_thumb_plan_reduce(C.c_void_p(entries.ctypes.data), n, int(factors[0]), int(factors[1]), int(columns),
                                                      C.c_void_p(sheet.ctypes.data)), "vrg_thumb_plan_reduce")
        self.columns, self.rows, self.cell_w, self.cell_h, self.tmp_bytes = (int(v) for v in sheet)
        self.width, self.height = self.columns * self.cell_w, self.rows * self.cell_h
        tables, table_at, n_ints = [], {}, 0
        for e in entries:
            pair = (int(e["left_w"]) * (2 if e["right_offset"] >= 0 else 1), int(e["left_h"]))
            for axis, f, red, out, ks, at in ((0, "fx", "red_w", "out_w", "h_ksize", "h_table"), (1, "fy", "red_h", "out_h", "v_ksize", "v_table")):
                if not e[ks]:
                    continue
                key = (int(e[red]), float(np.float32(pair[axis] / int(e[f]))), int(e[out]))
                if key not in table_at:
                    ksize, table = ops.pil_axis_table(number, key[0], key[2], (0.0, key[1]))
                    assert ksize == e[ks]
                    table_at[key] = n_ints
                    tables.append(table)
                    n_ints += len(table)
                e[at] = table_at[key]
        host_tables = np.concatenate(tables) if tables else np.zeros(1, np.int32)
        self.n, self.n_ints, self.entries_host = n, n_ints, entries
        _host_check(_host().vrg_thumb_check(C.c_void_p(entries.ctypes.data), n, C.c_void_p(host_tables.ctypes.data), n_ints, self.src_bytes,
                                            self.tmp_bytes, self.width, self.height, self.columns, self.cell_w, self.cell_h), "vrg_thumb_check")
        self.max_segments = max([-(-int(e["out_w"]) // int(e["cps"])) for e in entries] or [0])
        self.max_rows = max([int(e["red_h"]) for e in entries] or [0])
        self.tables = _upload(host_tables, device)
        self.entries = _upload(entries, device) if n else None
        self.tmp = torch.empty(max(self.tmp_bytes, 1), dtype=torch.uint8, device=device)
        self.out = torch.empty((self.height, self.width, 3), dtype=torch.uint8, device=device)

    def run_rows(self):
        _hip.check(_hip.lib().vrg_thumb_rows_u8(C.c_void_p(self.base), self.src_bytes, _hip.ptr(self.entries), self.n, _hip.ptr(self.tables),
                                                self.n_ints, _hip.ptr(self.tmp), self.tmp_bytes, self.max_segments, self.max_rows,
                                                _hip.current_stream()), "vrg_thumb_rows_u8")

    def run_compose(self):
        r, g, b = SHEET_CANVAS
        _hip.check(_hip.lib().vrg_thumb_compose_u8(_hip.ptr(self.entries), self.n, _hip.ptr(self.tables), self.n_ints, _hip.ptr(self.tmp),
                                                   self.tmp_bytes, _hip.ptr(self.out), self.width, self.height, self.columns, self.cell_w,
                                                   self.cell_h, r | g << 8 | b << 16, _hip.current_stream()), "vrg_thumb_compose_u8")
        return self.out

    def thumbnails(self):
        """the thumbnails cut out of the sheet, each of its own size"""
        return [self.out[int(e["dst_y"]):int(e["dst_y"]) + int(e["out_h"]), int(e["dst_x"]):int(e["dst_x"]) + int(e["out_w"])]
                for e in self.entries_host]


def _rgb_batch(images, name):
    """-> (the RGB images of a batch, the device they are on or None, how a device tensor goes back in the caller's form)"""
    items, _ = _image_list(images, name, 3)
    if any(i is not None and i.ndim != 3 for i in items):
        raise ValueError(f"{name} must be uint8 images of shape [h, w, 3]")
    first = next((i for i in items if i is not None), None)
    tensor = isinstance(images, torch.Tensor) or isinstance(first, torch.Tensor)
    on_device = tensor and first is not None and first.is_cuda and all(i is None or (isinstance(i, torch.Tensor) and i.is_cuda) for i in items)
    back = (lambda t: t) if on_device else (lambda t: t.cpu()) if tensor else (lambda t: t.cpu().numpy())
    return items, (first.device if on_device else None), back


def contact_sheet(originals, fixed=None, limit=24, columns=3, thumb_width=900):
    """``contact_sheet`` of the reference (:382-406) on decoded frames: for each of the first ``limit`` originals the pair original | fixed
    (the original again where ``fixed`` or its entry is None; a fixed frame of another size is pasted on black and clipped),
    ``pair.thumbnail((thumb_width, int(thumb_width * pair.height / pair.width)))``, and the thumbnails pasted ``columns`` to a row onto
    (24, 24, 24).  ``originals`` / ``fixed``: uint8 [n, H, W, 3] tensors or sequences of [H, W, 3] images of any sizes, on the device or
    the CPU.  -> the sheet, uint8 [rows * cell_h, columns * cell_w, 3], in the form the frames came in.  Raises the reference's
    RuntimeError when there is no frame.  The JPEG encode stays with the caller."""
    lefts, device, back = _rgb_batch(originals, "originals")
    if any(i is None for i in lefts):
        raise ValueError("originals must not hold None")
    rights = [None] * len(lefts)
    if fixed is not None:
        rights, fixed_device, _ = _rgb_batch(fixed, "fixed")
        if len(rights) != len(lefts):
            raise ValueError(f"fixed must hold one entry per original ({len(lefts)}), got {len(rights)}")
        if any(r is not None for r in rights) and fixed_device != device:
            device = None                                                    # mixed: everything is packed and uploaded
    lefts, rights = lefts[:int(limit)], rights[:int(limit)]
    if not lefts:
        raise RuntimeError(NO_FRAMES)
    thumb_width = int(thumb_width)
    requests = [(thumb_width, int(thumb_width * int(i.shape[0]) / (2 * int(i.shape[1])))) for i in lefts]
    if thumb_width < 1 or any(r[1] < 1 for r in requests):
        raise ValueError("thumb_width gives a thumbnail below 1 x 1")
    device = device if device is not None else compute_device()
    with torch.cuda.device(device):
        plan = ThumbPlan(lefts, [l if r is None else r for l, r in zip(lefts, rights)], requests, device, columns=columns)
        plan.run_rows()
        return back(plan.run_compose())


def _thumb_batch(images, plan_of, name):
    items, device, back = _rgb_batch(images, name)
    if any(i is None for i in items):
        raise ValueError(f"{name} must not hold None")
    if not items:
        return [] if not isinstance(images, (torch.Tensor, np.ndarray)) else images[:0]
    device = device if device is not None else compute_device()
    with torch.cuda.device(device):
        plan = plan_of(items, device)
        plan.run_rows()
        plan.run_compose()
        cut = plan.thumbnails()
        if isinstance(images, (torch.Tensor, np.ndarray)):
            return back(torch.stack(cut))
        return [back(c.contiguous()) for c in cut]


def pil_thumbnail(images, size, resample="bicubic", reducing_gap=2.0):
    """``Image.thumbnail(size, resample, reducing_gap)`` (size = (width, height)) of every RGB image of a batch: a uint8 tensor
    [n, h, w, 3] -> [n, h', w', 3], or a sequence of [h, w, 3] images of any sizes -> a list, each in the form it came in.  ``resample``:
    "bicubic" or "lanczos"; ``reducing_gap=None`` skips the reduce.  An image already within ``size`` comes back as a copy."""
    if not (size[0] >= 1 and size[1] >= 1):
        raise ValueError("size must be at least 1 x 1")
    return _thumb_batch(images, lambda items, device: ThumbPlan(items, None, [(size[0], size[1])] * len(items), device, resample, reducing_gap),
                        "images")


def pil_reduce(images, factor):
    """``Image.reduce(factor)`` (an integer or (fx, fy)) of every RGB image of a batch, in the forms of ``pil_thumbnail``"""
    fx, fy = (factor, factor) if not isinstance(factor, (tuple, list)) else factor
    return _thumb_batch(images, lambda items, device: ThumbPlan(items, None, None, device, factors=(fx, fy)), "images")

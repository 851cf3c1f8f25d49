"""The host side of the packed routes (``VRGDG_FaceFix``, ``far_face_repair``): decoded uint8 frames stay on the HOST and only their boxes
cross the bus.  A route gathers every active box into one page-locked buffer of dense ``[h][w][3]`` blocks (``BoxPack``, ``pack_boxes``) with
its second payload behind them (``staged_layout``), uploads it once, uploads its records with the ``int64 [n + 1]`` tile prefix behind them
(``upload_with_prefix``; the tile map is csrc/vrg_packed_tiles.hpp), runs its own kernels, downloads the packed result once (``download``)
and pastes the blocks into a copy of the frames (``paste_into_frames``).  The frame intake both routes share is here as well."""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np
import torch

from . import _hip
from ._devices import compute_device

TILE = _hip.FACEFIX_PACKED_TILE
assert TILE == _hip.PIL_PACKED_TILE            # one tile map: PACKED_TILE of csrc/vrg_packed_tiles.hpp


# frames in, frames out
def frames_in(frames, name):
    """-> (uint8 [F,H,W,3] on the GPU, a function that hands a GPU batch back in the caller's form)"""
    from .VRGDG_LUTVideoTools import _stack_frames, _unstack_frames
    from .VRGDG_StandaloneVideoEnhancerNodes import DecodedFrames
    if isinstance(frames, DecodedFrames):
        return check_frames(frames.u8, name), DecodedFrames
    if isinstance(frames, torch.Tensor):
        x = check_frames(frames, name)
        if x.is_cuda:
            return x, lambda t: t
        if x.shape[0] == 0:
            return x.to(compute_device()), lambda t: t.cpu()
        return _stack_frames(list(x.numpy())), lambda t: torch.from_numpy(np.stack(_unstack_frames(t))) if t.shape[0] else t.cpu()
    arrays = list(frames)
    if not arrays:
        raise ValueError(f"{name} must not be empty")
    return _stack_frames(arrays), lambda t: _unstack_frames(t) if t.shape[0] else []


def peek(frames, name):
    """(frames, height, width) of a batch in any of the accepted forms, checked before anything is uploaded"""
    t = getattr(frames, "u8", frames)
    if isinstance(t, torch.Tensor):
        check_frames(t, name)
        return int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    arrays = [np.asarray(f) for f in frames]
    if not arrays:
        raise ValueError(f"{name} must not be empty")
    for a in arrays:
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[-1] != 3 or a.shape != arrays[0].shape:
            raise ValueError(f"{name} must be HxWx3 uint8 arrays of one size")
    return len(arrays), int(arrays[0].shape[0]), int(arrays[0].shape[1])


def check_frames(t, name):
    if t.ndim != 4 or t.shape[-1] != 3 or t.dtype != torch.uint8:
        raise ValueError(f"{name} must be [frames, height, width, 3] uint8")
    if t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError(f"{name} must be at least 1 x 1")
    return t if t.is_contiguous() else t.contiguous()


def frame_boxes(crop_boxes, frames, height, width):
    """one (left, top, w, h) or None per frame; a box without pixels raises the reference's ValueError (:947-948)"""
    boxes = list(crop_boxes)
    if len(boxes) != frames:
        raise ValueError(f"crop_boxes must hold one box (or None) per frame: {len(boxes)} for {frames} frames")
    out = []
    for index, box in enumerate(boxes):
        if box is None:
            out.append(None)
            continue
        left, top, right, bottom = (int(v) for v in box)
        w, h = right - left, bottom - top
        if w <= 0 or h <= 0:
            raise ValueError(f"Invalid crop box for frame {index}.")
        if left < 0 or top < 0 or right > width or bottom > height:
            raise ValueError(f"crop box of frame {index} does not lie inside the {width} x {height} frame")
        out.append((left, top, w, h))
    return out


def host_arrays(frames, name, whole):
    """-> one HxWx3 numpy view per frame of a CPU batch (a uint8 tensor or numpy frames), the caller's own memory"""
    if hasattr(frames, "u8") or (isinstance(frames, torch.Tensor) and frames.is_cuda):
        raise TypeError(f"{name} is on the GPU already: the packed route is for decoded frames on the host, use {whole}")
    peek(frames, name)
    return list(frames.numpy()) if isinstance(frames, torch.Tensor) else [np.asarray(f) for f in frames]


# the plan: host integers
class BoxPack:
    """Host integers of one packed call, one entry per box that travels, in frame order: ``frames`` the frame indices, ``boxes``
    (left, top, w, h), ``offsets`` the byte offset of the box's dense [h][w][3] block in the packed buffers, ``tile_prefix`` int64 [n + 1]:
    0 and the running sum of ceil(w * h / 256), ``tiles`` its last entry.  ``bytes_up`` = ``bytes_down`` = the bytes of all these boxes.
    ``frame_bytes`` = frames * H * W * 3.  A route's ``PackedPlan`` is this class under the route's own description."""

    def __init__(self, frames, boxes, frame_bytes):
        self.frames, self.boxes, self.frame_bytes = frames, boxes, frame_bytes
        sizes = [w * h * 3 for _, _, w, h in boxes]
        self.offsets = [int(v) for v in np.cumsum([0] + sizes[:-1])] if sizes else []
        self.tile_prefix = np.concatenate([[0], np.cumsum([(w * h + TILE - 1) // TILE for _, _, w, h in boxes], dtype=np.int64)]).astype(np.int64)
        self.tiles = int(self.tile_prefix[-1])
        self.bytes_up = self.bytes_down = int(sum(sizes))

    def blocks(self, host):
        """the boxes' ``[h, w, 3]`` blocks as views of a packed uint8 numpy buffer"""
        return [host[offset:offset + w * h * 3].reshape(h, w, 3) for (_, _, w, h), offset in zip(self.boxes, self.offsets)]


def staged_layout(bytes_up, payload_sizes):
    """a route's second payload behind the boxes' ``bytes_up`` bytes, from the next multiple of 16 -> [every item's start, the end of the last]"""
    return [int(v) for v in -(-int(bytes_up) // 16) * 16 + np.cumsum([0] + [int(s) for s in payload_sizes])]


# bytes: gather, up, down, paste
def pack_boxes(arrays, plan, stage):
    """every box of ``plan`` cut out of ``arrays`` as a dense block at its offset of ``stage`` (a uint8 numpy array of at least plan.bytes_up)"""
    for f, (left, top, w, h), block in zip(plan.frames, plan.boxes, plan.blocks(stage)):
        block[...] = arrays[f][top:top + h, left:left + w]


def paste_boxes(arrays, plan, results):
    for f, (left, top, w, h), block in zip(plan.frames, plan.boxes, results):
        arrays[f][top:top + h, left:left + w] = block


def staging(nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, pin_memory=True)


def upload_with_prefix(desc, prefix, device):
    """the records of a tile grid with their int64 tile prefix behind them, in one upload -> (the device tensor, the prefix's address)"""
    table = _hip.upload_records(desc, device, trailing=(prefix,))
    return table, C.c_void_p(table.data_ptr() + desc.nbytes)


def download(dev):
    """a device tensor -> a page-locked host tensor of its shape, complete on return"""
    host = torch.empty(dev.shape, dtype=dev.dtype, pin_memory=True)
    host.copy_(dev, non_blocking=True)
    torch.cuda.current_stream(dev.device).synchronize()
    return host


def host_copy(dst, src):
    """src -> dst, two numpy arrays of one shape: the threaded copy of vrg_host_copy where both are dense"""
    if dst.flags.c_contiguous and src.flags.c_contiguous:
        _hip.check(_hip.host_library().vrg_host_copy(C.c_void_p(dst.ctypes.data), C.c_void_p(src.ctypes.data), src.nbytes, 0), "vrg_host_copy")
    else:
        dst[...] = src


def paste_into_frames(originals_u8, plan, results, inplace):
    """``results`` (one block per box of ``plan``) pasted into a host copy of ``originals_u8`` or -- ``inplace`` -- into the frames themselves"""
    arrays = host_arrays(originals_u8, "originals", "composite_frames")
    if inplace:
        out, target = originals_u8, arrays
    elif isinstance(originals_u8, torch.Tensor):
        out = torch.empty(originals_u8.shape, dtype=torch.uint8)
        if out.numel():
            host_copy(out.numpy(), originals_u8.numpy())
        target = list(out.numpy())
    else:
        out = target = [np.empty(a.shape, dtype=np.uint8) for a in arrays]
        for dst, src in zip(target, arrays):
            host_copy(dst, src)
    paste_boxes(target, plan, results)
    return out


# what the last packed call of this thread moved (nothing given: nothing), per route: a route is named by the key of its second payload
_ledger = threading.local()


def note_transfer(payload_key, **moved):
    setattr(_ledger, payload_key, moved)


def last_transfer(payload_key) -> dict:
    moved = getattr(_ledger, payload_key, {})
    return {key: moved.get(key, 0) for key in ("bytes_up", "bytes_down", payload_key, "tables_up")}

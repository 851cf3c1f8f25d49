"""Video Enhance on the MI355X: the frame resize helpers and the "Restore Original Resolution" node of the reference's
VRGDG_VideoEnhanceNodes.py with the same names, signatures, widget specs and messages; the pixels come from csrc/vrg_resize.hip.

What is here: `_resize_batch`, `_restore_batch`, `_interpolation`, `_round_dimension` and `VRGDGVideoEnhanceRestoreOriginal`.  The
resize + blend + clamp of the node is ONE pass over the originals (ops.restore_frames) instead of the reference's 3-6 full-size eager
kernels and temporaries.  CPU tensors (what ComfyUI hands a node) go through the host-fed pipeline of _devices (staging ring, pieces
along the frame axis, upload / kernel / download overlapped); device tensors are processed where they are.

What is NOT here: the Prepare node (it has a module of its own, VRGDG_VideoEnhancePrepare.py), the anchor
and collect nodes, and the registration in the package's NODE_CLASS_MAPPINGS: INTEGRATION.md shows the two lines that merge this
module's mapping.  The node is eager: it is not part of the deferred graph fusion of nodes.py.
"""
from __future__ import annotations

import torch

from . import ops
from ._devices import compute_device, intermediate_device, piece_frames, stream_frames

VIDEO_ENHANCE_CONTEXT = "VRGDG_VIDEO_ENHANCE_CONTEXT"


def _log(message):
    print(f"[VRGDG Video Enhance] {message}", flush=True)


def _round_dimension(value, multiple):
    """`value` (at least 8) to the nearest multiple of `multiple` (at least 1), never below one multiple; Python's round() decides ties."""
    step = int(multiple) if int(multiple) > 1 else 1
    size = int(value) if int(value) > 8 else 8
    steps = int(round(size / step))
    return steps * step if steps >= 1 else step


def _interpolation(mode):
    return ops.interpolation_mode(mode)


def _resample(images, geometry, resize_method):
    """`images` through ops.resize_geometry_frames wherever they live: device frames in place, host frames in pieces along the frame
    axis (the result has another frame size than the input, so it does not go through stream_frames: upload, kernel, download per piece)."""
    if images.dtype != torch.float32:
        images = images.float()
    if images.is_cuda:
        return ops.resize_geometry_frames(images, geometry, resize_method)
    dev = compute_device()
    out_dev = intermediate_device()
    frames = int(images.shape[0])
    in_fb = int(images.shape[1]) * int(images.shape[2]) * int(images.shape[3]) * 4
    out = torch.empty((frames, geometry.out_h, geometry.out_w, 3), dtype=torch.float32, device=out_dev)
    per = piece_frames(frames, max(in_fb, geometry.out_h * geometry.out_w * 12))
    with torch.cuda.device(dev):
        for s in range(0, frames, per):
            e = min(frames, s + per)
            out[s:e].copy_(ops.resize_geometry_frames(images[s:e].to(dev), geometry, resize_method))
    return out


def _check_batch(images):
    if not isinstance(images, torch.Tensor) or images.ndim != 4 or images.shape[0] < 1:
        raise ValueError("Video Enhance requires a non-empty IMAGE batch.")


def _resize_batch(images, target_width, target_height, fit_mode, resize_method):
    _check_batch(images)
    geometry = ops.resize_geometry(images.shape[1], images.shape[2], target_width, target_height, fit_mode)
    return _resample(images, geometry, resize_method)


def _restore_batch(images, source_width, source_height, fit_mode, resize_method):
    """Undo temporary letterboxing before returning frames to source dimensions."""
    _check_batch(images)
    geometry = ops.restore_geometry(images.shape[1], images.shape[2], source_width, source_height, fit_mode)
    return _resample(images, geometry, resize_method)


def _restore_blend(work, originals, source_width, source_height, fit_mode, resize_method, strength, usable):
    """The fused restore wherever the frames live.  Shaped like `originals`."""
    if originals.dtype != torch.float32:
        originals = originals.float()
    if work.dtype != torch.float32:
        work = work.float()
    if originals.is_cuda:
        return ops.restore_frames(work.to(originals.device), originals, source_width, source_height, fit_mode, resize_method, strength, usable)
    dev = compute_device()
    if originals.shape[0] == 0 or intermediate_device().type != "cpu":
        return ops.restore_frames(work.to(dev), originals.to(dev), source_width, source_height, fit_mode, resize_method, strength,
                                  usable).to(intermediate_device())
    # host-fed: the originals (the large side, 24 B per pixel up and down) stream through the staging pipeline; the working-resolution
    # frames that will be used (6-16x fewer bytes) are uploaded once, ahead of it
    with torch.cuda.device(dev):
        work_dev = work[:max(usable, 1)].to(dev)

    def fn(gpu_originals, first_frame):
        s = min(first_frame, usable)
        e = min(first_frame + int(gpu_originals.shape[0]), usable)
        piece = work_dev[s:e] if e > s else work_dev[:1]
        return ops.restore_frames(piece, gpu_originals, source_width, source_height, fit_mode, resize_method, strength, e - s)

    return stream_frames(originals, fn)


class VRGDGVideoEnhanceRestoreOriginal:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {
            "ltx_enhanced_frames": ("IMAGE", {"tooltip": "Connect the final decoded IMAGE batch from LTX. These temporary working-resolution frames are resized back to the exact source dimensions."}),
            "video_enhance_context": (VIDEO_ENHANCE_CONTEXT, {"tooltip": "Connect Collect LTX Inputs context. It contains the untouched source frames, exact source dimensions, and frame count."}),
            "resize_method": (["Bicubic (recommended)", "Bilinear", "Area", "Nearest"], {"default": "Bicubic (recommended)", "tooltip": "Interpolation used to restore LTX frames to the exact source width and height. This changes dimensions only; optional AI upscalers may be inserted before this node if desired."}),
            "enhancement_strength": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.05, "tooltip": "Blends the restored LTX result with the untouched original video. 1 uses the complete LTX result; lower values retain more original pixels and can reduce over-processing."}),
        }}

    RETURN_TYPES = ("IMAGE", "INT", "INT", "INT", "FLOAT")
    RETURN_NAMES = ("enhanced_video_frames", "frame_count", "original_width", "original_height", "fps")
    FUNCTION = "restore"
    CATEGORY = "VRGameDevGirl/Video Enhance"
    DESCRIPTION = "Restores decoded LTX output to the exact input resolution and frame count, preserving unmatched source-tail frames and optionally blending with the untouched source video."

    def restore(self, ltx_enhanced_frames, video_enhance_context, resize_method, enhancement_strength):
        ctx = video_enhance_context
        originals = ctx.get("original_frames")
        if not (isinstance(originals, torch.Tensor) and originals.ndim == 4):
            raise ValueError("Video Enhance context does not contain valid original frames.")
        # a missing or zero entry of the context falls back to what the original frames say
        frame_count, source_height, source_width = (int(ctx.get(key) or originals.shape[axis])
                                                    for axis, key in enumerate(("frame_count", "source_height", "source_width")))
        work_frames = int(ltx_enhanced_frames.shape[0])
        if not -7 <= frame_count - work_frames <= 7:
            raise ValueError(f"LTX returned {work_frames} frames for {frame_count} source frames.")
        _check_batch(ltx_enhanced_frames)
        usable = min(frame_count, work_frames)
        strength = float(enhancement_strength)
        output = _restore_blend(ltx_enhanced_frames, originals, source_width, source_height, str(ctx.get("fit_mode") or ops.FIT_STRETCH),
                                resize_method, strength, usable)
        _log(f"Restore finished: {usable}/{frame_count} LTX frame(s) restored to {source_width}x{source_height}; "
             f"source tail preserved={max(0, frame_count - work_frames)}; strength={strength:.2f}.")
        return output, frame_count, source_width, source_height, float(ctx.get("fps") or 0.0)


NODE_CLASS_MAPPINGS = {
    "VRGDGVideoEnhanceRestoreOriginal": VRGDGVideoEnhanceRestoreOriginal,
}


NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDGVideoEnhanceRestoreOriginal": "Video Enhance - Restore Original Resolution",
}

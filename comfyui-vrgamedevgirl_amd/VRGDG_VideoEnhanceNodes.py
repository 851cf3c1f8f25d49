"""Video Enhance on the MI355X: the frame resize helpers and the "Restore Original Resolution" node of the reference's
VRGDG_VideoEnhanceNodes.py with the same names, signatures, widget specs and messages; the pixels come from csrc/vrg_resize.hip.

What is here: `_resize_batch`, `_restore_batch`, `_interpolation`, `_round_dimension` and `VRGDGVideoEnhanceRestoreOriginal`.  The
resize + blend + clamp of the node is ONE pass over the originals (ops.restore_frames) instead of the reference's 3-6 full-size eager
kernels and temporaries.  CPU tensors (what ComfyUI hands a node) go through the host-fed pipeline of _devices (staging ring, pieces
along the frame axis, upload / kernel / download overlapped); device tensors are processed where they are.

The anchor round trip between Prepare and Restore is here too: `VRGDGVideoEnhanceLoadAnchorsMetaBatch` (the anchor files of a job through
VHS Meta Batch: the protocol and the decode seam `image_loader` are in _anchors.py, the pixels come from ops.anchor_frames, one launch a
call), `VRGDGVideoEnhanceStoreAnchors` (ops.anchor_store_bytes, one page-locked download, then the PNG writer `_save_image_batch` of
VRGDG_VideoEnhancePrepare.py) and `VRGDGVideoEnhanceCollectLTXInputs` (host logic only).  They are listed in ANCHOR_NODE_CLASS_MAPPINGS /
ANCHOR_NODE_DISPLAY_NAME_MAPPINGS: this module's NODE_CLASS_MAPPINGS keeps its one key (an existing test pins that set).

What is NOT here: the Prepare node (it has a module of its own, VRGDG_VideoEnhancePrepare.py) and the registration
in the package's NODE_CLASS_MAPPINGS: INTEGRATION.md shows the lines that merge this module's mappings.  The nodes are eager: they are
not part of the deferred graph fusion of nodes.py.
"""
from __future__ import annotations

import os

import torch

from . import _anchors, ops
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


# ------------------------------------------------------------------------------------------------
# the anchor round trip: Load Anchors (Meta Batch) -> the image model -> Store Enhanced Anchors -> Collect LTX Inputs
# ------------------------------------------------------------------------------------------------
image_loader = _anchors.image_loader      # the decode seam of the Load node: path -> [h, w, 3] uint8 R,G,B

_NO_ANCHOR_FOLDER = "Prepared Video Enhance anchor folder was not found: {}"
_NO_ANCHOR_FILES = "No Video Enhance anchor images were found in {}"
_NO_ANCHORS_LEFT = "The Video Enhance Meta Batch has no anchor images left to load."
_SAFE_REACH = 8                           # how far from an anchor a conditioning position is looked for
_LTX_PERIOD, _LTX_REFUSED = 8, 1          # LTX takes no conditioning position p with p % 8 == 1


def _save_image_batch(images_or_bytes, folder, prefix):
    """the PNG writer seam: VRGDG_VideoEnhancePrepare._save_image_batch (image files of an earlier run in `folder` go first)"""
    from .VRGDG_VideoEnhancePrepare import _save_image_batch as save
    save(images_or_bytes, folder, prefix)


def _count_error(got, expected):
    return ValueError(f"Z-Image returned {got} anchors; expected {expected}.")


def _joined(indices):
    return ",".join(str(value) for value in indices)


class VRGDGVideoEnhanceLoadAnchorsMetaBatch:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "video_enhance_context": (VIDEO_ENHANCE_CONTEXT, {"tooltip": "Connect Prepare Video and Anchors context. It contains the automatically generated full-frame anchor folder."}),
                "meta_batch": ("VHS_BatchManager", {"tooltip": "Connect VHS Meta Batch Manager and set frames_per_batch from Prepare anchor_count so Z-Image receives the managed anchor sequence in one queued workflow."}),
            },
            "hidden": {"unique_id": "UNIQUE_ID"},
        }

    RETURN_TYPES = ("IMAGE", "MASK", "INT", VIDEO_ENHANCE_CONTEXT)
    RETURN_NAMES = ("anchor_images", "mask", "batch_frame_count", "video_enhance_context")
    FUNCTION = "load"
    CATEGORY = "VRGameDevGirl/Video Enhance"
    DESCRIPTION = "Loads full-frame Video Enhance anchors through VHS Meta Batch for sequential Z-Image enhancement."

    def load(self, video_enhance_context, meta_batch, unique_id):
        directory = str(video_enhance_context.get("anchor_sources_folder") or "")
        if not os.path.isdir(directory):
            raise FileNotFoundError(_NO_ANCHOR_FOLDER.format(directory))
        images, masks, count = _anchors.load_chunk(directory, meta_batch, unique_id, lambda path: image_loader(path), _NO_ANCHOR_FILES,
                                                   _NO_ANCHORS_LEFT)
        _log(f"Meta Batch returned {count} anchor(s) at {int(images.shape[2])}x{int(images.shape[1])}.")
        return images, masks, count, video_enhance_context


class VRGDGVideoEnhanceStoreAnchors:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {
            "enhanced_anchors": ("IMAGE", {"tooltip": "Connect the decoded Z-Image IMAGE result. Its count and order must match the anchors loaded through Meta Batch."}),
            "video_enhance_context": (VIDEO_ENHANCE_CONTEXT, {"tooltip": "Connect the context from Load Anchors (Meta Batch) so enhanced results are stored in the correct job."}),
        }}

    RETURN_TYPES = ("STRING", "STRING", "INT", VIDEO_ENHANCE_CONTEXT)
    RETURN_NAMES = ("enhanced_anchor_folder", "anchor_indices", "anchor_count", "video_enhance_context")
    FUNCTION = "store"
    CATEGORY = "VRGameDevGirl/Video Enhance"
    OUTPUT_NODE = True
    DESCRIPTION = "Stores enhanced full-frame anchors in deterministic order for LTX conditioning."

    def store(self, enhanced_anchors, video_enhance_context):
        context = dict(video_enhance_context)
        indices = list(context.get("anchor_indices") or [])
        if int(enhanced_anchors.shape[0]) != len(indices):
            raise _count_error(enhanced_anchors.shape[0], len(indices))
        folder = os.path.join(context["job_folder"], "enhanced_anchors")
        no_frames = torch.zeros((0, 1, 1, 3), dtype=torch.uint8)                  # an empty batch still clears the folder
        _save_image_batch(_anchors.stored_bytes(enhanced_anchors) if indices else no_frames, folder, "anchor")
        context["enhanced_anchor_folder"] = folder
        _log(f"Stored {len(indices)} enhanced anchor(s) in {folder}")
        return folder, _joined(indices), len(indices), context


class VRGDGVideoEnhanceCollectLTXInputs:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {
            "prepared_video_context": (VIDEO_ENHANCE_CONTEXT, {"tooltip": "Connect Prepare Video and Anchors context. This proves the temporary full-frame LTX MP4 exists."}),
            "enhanced_anchor_context": (VIDEO_ENHANCE_CONTEXT, {"tooltip": "Connect Store Enhanced Anchors context. This proves all Z-Image anchor results were saved."}),
        }}

    RETURN_TYPES = ("STRING", "STRING", "STRING", "INT", "INT", "INT", VIDEO_ENHANCE_CONTEXT)
    RETURN_NAMES = ("ltx_video_path", "enhanced_anchor_folder", "anchor_indices", "anchor_count", "ltx_width", "ltx_height", "video_enhance_context")
    FUNCTION = "collect"
    CATEGORY = "VRGameDevGirl/Video Enhance"
    DESCRIPTION = "Validates both Video Enhance branches, adjusts LTX-incompatible conditioning positions, and exposes the paths and dimensions required by the LTX workflow."

    @staticmethod
    def _safe_indices(indices, frame_count):
        """Every anchor position moved to the nearest frame LTX takes: the position itself, else 1 below, 1 above, 2 below, ... up to 8
        away, inside the video, not taken by an earlier anchor and not 1 modulo 8."""
        taken, safe = set(), []
        for anchor in indices:
            near = [anchor] + [anchor + sign * step for step in range(1, _SAFE_REACH + 1) for sign in (-1, 1)]
            fits = [p for p in near if 0 <= p < frame_count and p not in taken and p % _LTX_PERIOD != _LTX_REFUSED]
            if not fits:
                raise ValueError(f"Could not find a safe LTX conditioning position near anchor {anchor}.")
            taken.add(fits[0])
            safe.append(fits[0])
        return safe

    def collect(self, prepared_video_context, enhanced_anchor_context):
        prepared, enhanced = prepared_video_context, enhanced_anchor_context
        job = str(prepared.get("job_id") or "")
        if not job or job != str(enhanced.get("job_id") or ""):
            raise ValueError("The prepared video and enhanced anchors belong to different Video Enhance jobs.")
        video_path, folder = str(prepared.get("ltx_video_path") or ""), str(enhanced.get("enhanced_anchor_folder") or "")
        indices = list(enhanced.get("anchor_indices") or [])
        if not os.path.isfile(video_path):
            raise FileNotFoundError(f"The Video Enhance LTX working video is missing: {video_path}")
        if not os.path.isdir(folder):
            raise FileNotFoundError(f"The enhanced Video Enhance anchor folder is missing: {folder}")
        stored = [name for name in os.listdir(folder) if name.lower().endswith(".png")]
        if len(stored) != len(indices):
            raise ValueError(f"Enhanced anchor folder contains {len(stored)} images; expected {len(indices)}.")
        safe = self._safe_indices(indices, int(prepared.get("frame_count") or 0))
        moved = [f"{old}->{new}" for old, new in zip(indices, safe) if old != new]
        if moved:
            _log("Adjusted LTX-incompatible anchor position(s): " + ", ".join(moved))
        context = dict(prepared, enhanced_anchor_folder=folder, anchor_indices=safe)
        return video_path, folder, _joined(safe), len(safe), int(context["ltx_width"]), int(context["ltx_height"]), context


ANCHOR_NODE_CLASS_MAPPINGS = {
    "VRGDGVideoEnhanceLoadAnchorsMetaBatch": VRGDGVideoEnhanceLoadAnchorsMetaBatch,
    "VRGDGVideoEnhanceStoreAnchors": VRGDGVideoEnhanceStoreAnchors,
    "VRGDGVideoEnhanceCollectLTXInputs": VRGDGVideoEnhanceCollectLTXInputs,
}


ANCHOR_NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDGVideoEnhanceLoadAnchorsMetaBatch": "Video Enhance - Load Anchors (Meta Batch)",
    "VRGDGVideoEnhanceStoreAnchors": "Video Enhance - Store Enhanced Anchors",
    "VRGDGVideoEnhanceCollectLTXInputs": "Video Enhance - Collect LTX Inputs",
}

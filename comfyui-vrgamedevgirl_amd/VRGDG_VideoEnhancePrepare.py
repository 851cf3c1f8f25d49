"""Video Enhance on the MI355X, the front of the pipeline: the "Prepare Video and Anchors" node of the reference's
VRGDG_VideoEnhanceNodes.py (:170-252) with the same name, widget specs, return conventions, messages, job folder, file names, ffmpeg command
line and context; the pixels come from csrc/vrg_prepare.hip.

The reference resizes every frame to the LTX size, gathers the anchor frames and resizes those to the anchor size (fp32, on the CPU), then
turns both sets into bytes frame by frame for the PNG files.  Here that is two ops.prepare_frames calls -- all frames to the LTX
geometry, the anchor index list to the anchor geometry -- each giving the fp32 frames the node returns AND the bytes of the PNG files from
the same computed value: no gathered copy of the anchors, no second and third pass for the bytes.  CPU frames (what ComfyUI hands a
node) go up in pieces along the frame axis, each piece once, and both launches run on the uploaded piece with the anchor indices
translated into it; 12 + 3 bytes per OUTPUT pixel come back, whole source frames never do.  Device frames are processed where they are.

Pillow writes the PNG files (the only encoder here) and ffmpeg the working video: `_encode_mp4` is a subprocess seam and a module
attribute a caller may replace.  This module has its own mapping, PREPARE_NODE_CLASS_MAPPINGS / PREPARE_NODE_DISPLAY_NAME_MAPPINGS:
VRGDG_VideoEnhanceNodes.NODE_CLASS_MAPPINGS and the package's mapping keep their pinned key sets (INTEGRATION.md has the import lines).
The Load Anchors, Store Anchors and Collect nodes are not here.  The node is eager: it is not part of the deferred graph of nodes.py.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import time
import uuid

import numpy as np
import torch

from . import ops
from ._devices import compute_device, intermediate_device, piece_frames
from .VRGDG_VideoEnhanceNodes import VIDEO_ENHANCE_CONTEXT, _log, _round_dimension

_IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".webp", ".bmp")
_FPS_KEYS = ("loaded_fps", "source_fps", "fps")            # the order in which a VHS video_info is asked for the frame rate
_FRAME_PATTERN = "frame_%06d.png"                          # what ffmpeg reads; _save_image_batch(.., "frame") writes these names
# what follows `ffmpeg -y -framerate <fps> -i <frames>` on the working video's command line, up to the output path
_MP4_OPTIONS = (("-frames:v", "{frames}"), ("-an",), ("-c:v", "libx264"), ("-preset", "slow"), ("-crf", "10"), ("-pix_fmt", "yuv420p"),
                ("-movflags", "+faststart"))
_NO_FFMPEG = "FFmpeg is required to create the Video Enhance working video."
_MP4_FAILED = "Could not create the Video Enhance working MP4: "
_MP4_TAIL = 1600                                           # characters of ffmpeg's output kept in the message


def _progress(index, total, label, checkpoints=10):
    """A log line after the first item, after the last, and after every max(total // checkpoints, 1)-th one."""
    done = index + 1
    if total > 0 and (done in (1, total) or done % max(total // checkpoints, 1) == 0):
        _log(f"{label}: {done}/{total}")


def _positive(value):
    """`value` as a float where it is a positive number (a string of one included), else 0.0"""
    try:
        number = float(value or 0)
    except (TypeError, ValueError):
        return 0.0
    return number if number > 0 else 0.0


def _fps(video_info, fallback):
    """The first positive rate a video_info dictionary holds under _FPS_KEYS; float(fallback) without one, or without a dictionary."""
    rates = [_positive(video_info.get(key)) for key in _FPS_KEYS] if isinstance(video_info, dict) else []
    return next((rate for rate in rates if rate), float(fallback))


def _as_bytes(images_or_bytes):
    """[N, H, W, 3] uint8 on the host.  Bytes (what ops.prepare_frames hands out) pass through; float images are quantised on the host,
    (clamp(x, 0, 1) * 255).round() in fp32 -- the node itself never takes that route."""
    x = images_or_bytes
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return np.ascontiguousarray(x[..., :3])
    return (np.clip(x[..., :3].astype(np.float32), 0, 1) * np.float32(255)).round().astype(np.uint8)


def _save_image_batch(images_or_bytes, folder, prefix):
    """The frames as `folder`/`prefix`_000000.png, `prefix`_000001.png, ...; image files of an earlier run in `folder` go first."""
    from PIL import Image

    os.makedirs(folder, exist_ok=True)
    stale = [entry.path for entry in os.scandir(folder) if entry.name.lower().endswith(_IMAGE_SUFFIXES)]
    for path in stale:
        os.remove(path)
    frames = _as_bytes(images_or_bytes)
    for number, frame in enumerate(frames):
        Image.fromarray(frame, "RGB").save(os.path.join(folder, "%s_%06d.png" % (prefix, number)))
        _progress(number, len(frames), f"Saving {prefix} frames")


def _ffmpeg_executable():
    """ffmpeg from the PATH, else the one the imageio_ffmpeg package brings"""
    on_path = shutil.which("ffmpeg")
    if on_path:
        return on_path
    try:
        from imageio_ffmpeg import get_ffmpeg_exe
        return get_ffmpeg_exe()
    except Exception as exc:
        raise RuntimeError(_NO_FFMPEG) from exc


def _mp4_argv(executable, frames_folder, frame_count, fps, output_path):
    argv = [executable, "-y", "-framerate", format(fps, ".12g"), "-i", os.path.join(frames_folder, _FRAME_PATTERN)]
    for option in _MP4_OPTIONS:
        argv += [word.format(frames=int(frame_count)) for word in option]
    return argv + [output_path]


def _encode_mp4(frames_folder, frame_count, fps, output_path):
    """The PNG frames of `frames_folder` as an H.264 video at `output_path`: one ffmpeg run.  It has failed when ffmpeg says so or
    leaves no file; the end of what it printed goes into the error."""
    argv = _mp4_argv(_ffmpeg_executable(), frames_folder, frame_count, fps, output_path)
    run = subprocess.run(argv, capture_output=True, text=True, errors="replace", check=False)
    if run.returncode == 0 and os.path.isfile(output_path):
        return
    said = (run.stderr or run.stdout or "FFmpeg failed").strip()
    raise RuntimeError(_MP4_FAILED + said[-_MP4_TAIL:])


def _anchor_indices(frame_count, interval):
    """Frames 0, interval, 2 * interval, ... and the last frame, ascending"""
    return sorted(set(range(0, frame_count, interval)) | {frame_count - 1})


def _prepare_pixels(video_frames, ltx_geometry, anchor_geometry, anchor_indices, resize_method):
    """(ltx fp32, ltx bytes, anchor fp32, anchor bytes): the fp32 frames where the node's results live, the bytes on the host."""
    images = video_frames if video_frames.dtype == torch.float32 else video_frames.float()
    if images.is_cuda:
        ltx, ltx_u8 = ops.prepare_frames(images, ltx_geometry, resize_method)
        anchors, anchors_u8 = ops.prepare_frames(images, anchor_geometry, resize_method, anchor_indices)
        return ltx, ltx_u8.cpu(), anchors, anchors_u8.cpu()
    dev, out_dev = compute_device(), intermediate_device()
    frames = int(images.shape[0])
    shapes = [(n, g.out_h, g.out_w, 3) for n, g in ((frames, ltx_geometry), (len(anchor_indices), anchor_geometry))]
    ltx, anchors = (torch.empty(s, dtype=torch.float32, device=out_dev) for s in shapes)
    ltx_u8, anchors_u8 = (torch.empty(s, dtype=torch.uint8) for s in shapes)
    per = piece_frames(frames, int(images.shape[1]) * int(images.shape[2]) * int(images.shape[3]) * 4)
    done = 0                                                  # anchors written so far: the list ascends, so a piece's anchors are a run of it
    with torch.cuda.device(dev):
        for s in range(0, frames, per):
            e = min(frames, s + per)
            piece = images[s:e].to(dev)
            f32, u8 = ops.prepare_frames(piece, ltx_geometry, resize_method)
            ltx[s:e].copy_(f32)
            ltx_u8[s:e].copy_(u8)
            local = [i - s for i in anchor_indices[done:] if i < e]
            if local:
                f32, u8 = ops.prepare_frames(piece, anchor_geometry, resize_method, local)
                anchors[done:done + len(local)].copy_(f32)
                anchors_u8[done:done + len(local)].copy_(u8)
                done += len(local)
    return ltx, ltx_u8, anchors, anchors_u8


_EMPTY_BATCH = "Video Enhance Prepare requires a non-empty IMAGE batch from a video loader."
#: the keys of the context dictionary, in the order the downstream nodes of the pipeline were written against
_CONTEXT_KEYS = ("version", "job_id", "job_folder", "original_frames", "source_width", "source_height", "frame_count", "fps", "anchor_indices",
                 "anchor_sources_folder", "anchor_width", "anchor_height", "ltx_width", "ltx_height", "ltx_video_path", "fit_mode",
                 "resize_method")


def _leading_int(choice):
    """the number a widget choice such as '16 frames (recommended)' or '32 (recommended)' begins with"""
    return int(str(choice).split()[0])


class _Job:
    """The folders and files of one Prepare run under ComfyUI's output directory:
    video_enhance/jobs/video_enhance_<date>_<time>_<8 hex digits>/ with anchor_sources/, ltx_working_frames/ and ltx_working_video.mp4"""

    def __init__(self, output_directory):
        self.job_id = "_".join(("video_enhance", time.strftime("%Y%m%d_%H%M%S"), uuid.uuid4().hex[:8]))
        self.folder = os.path.join(output_directory, "video_enhance", "jobs", self.job_id)
        self.anchors = os.path.join(self.folder, "anchor_sources")
        self.frames = os.path.join(self.folder, "ltx_working_frames")
        self.video = os.path.join(self.folder, "ltx_working_video.mp4")


class VRGDGVideoEnhancePrepare:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "video_frames": ("IMAGE", {"tooltip": "Connect the full IMAGE batch from VHS Load Video. These original frames remain unchanged in the context and are used to enforce the exact final resolution and frame count."}),
                "anchor_interval": (["8 frames", "16 frames (recommended)", "24 frames", "32 frames", "48 frames", "64 frames", "96 frames", "120 frames"], {"default": "16 frames (recommended)", "tooltip": "Spacing between full-frame Z-Image guide anchors. The first and final frames are always included. Smaller spacing gives LTX more enhanced references but requires more Z-Image runs."}),
                "anchor_width": ("INT", {"default": 768, "min": 128, "max": 4096, "step": 8, "tooltip": "Requested width used only for Z-Image anchor enhancement. It does not change the source or final video resolution."}),
                "anchor_height": ("INT", {"default": 432, "min": 128, "max": 4096, "step": 8, "tooltip": "Requested height used only for Z-Image anchor enhancement. Choose dimensions matching the source aspect ratio unless using Fit with letterbox."}),
                "ltx_width": ("INT", {"default": 960, "min": 128, "max": 4096, "step": 8, "tooltip": "Temporary LTX working width. Higher values can improve spatial detail but substantially increase VRAM use and runtime. Final output is restored to the source width."}),
                "ltx_height": ("INT", {"default": 544, "min": 128, "max": 4096, "step": 8, "tooltip": "Temporary LTX working height. Higher values can improve spatial detail but substantially increase VRAM use and runtime. Final output is restored to the source height."}),
                "dimension_multiple": (["8", "16", "32 (recommended)", "64"], {"default": "32 (recommended)", "tooltip": "Rounds requested anchor and LTX dimensions to a model-friendly multiple. The resolved dimensions are exposed as outputs so downstream loaders can match them exactly."}),
                "fit_mode": (["Fit with letterbox (preserve all)", "Crop to fill", "Stretch to dimensions"], {"default": "Fit with letterbox (preserve all)", "tooltip": "Fit preserves the entire frame and adds black bars if aspect ratios differ. Crop fills the dimensions while trimming edges. Stretch changes aspect ratio and is usually not recommended."}),
                "resize_method": (["Bicubic (recommended)", "Bilinear", "Area", "Nearest"], {"default": "Bicubic (recommended)", "tooltip": "Interpolation used for temporary anchor and LTX resizing. Bicubic is a strong general default. Area can be useful for large downscales."}),
                "fallback_fps": ("FLOAT", {"default": 24.0, "min": 1.0, "max": 240.0, "step": 0.001, "tooltip": "Used only when video_info is not connected or lacks FPS metadata. Connect video_info to preserve exact source timing."}),
            },
            "optional": {
                "video_info": ("VHS_VIDEOINFO", {"tooltip": "Connect VHS Load Video video_info so the temporary LTX video uses the exact source FPS."}),
            },
        }

    RETURN_TYPES = ("IMAGE", "IMAGE", "INT", "STRING", "STRING", "INT", "INT", "FLOAT", VIDEO_ENHANCE_CONTEXT)
    RETURN_NAMES = ("ltx_working_frames", "anchor_images", "anchor_count", "anchor_indices", "ltx_video_path", "ltx_width", "ltx_height", "fps", "video_enhance_context")
    FUNCTION = "prepare"
    CATEGORY = "VRGameDevGirl/Video Enhance"
    DESCRIPTION = "Creates an independent full-frame Video Enhance job, temporary LTX video, and regularly spaced Z-Image anchors while preserving the exact source frames and metadata for final restoration."

    def prepare(self, video_frames, anchor_interval, anchor_width, anchor_height, ltx_width, ltx_height,
                dimension_multiple, fit_mode, resize_method, fallback_fps, video_info=None):
        import folder_paths

        if video_frames.ndim != 4 or video_frames.shape[0] < 1:
            raise ValueError(_EMPTY_BATCH)
        frame_count, source_height, source_width = (int(side) for side in video_frames.shape[:3])
        step = _leading_int(dimension_multiple)
        sizes = {name: _round_dimension(asked, step) for name, asked in
                 (("anchor_width", anchor_width), ("anchor_height", anchor_height), ("ltx_width", ltx_width), ("ltx_height", ltx_height))}
        fps = _fps(video_info, fallback_fps)
        anchors_at = _anchor_indices(frame_count, _leading_int(anchor_interval))

        job = _Job(folder_paths.get_output_directory())
        os.makedirs(job.folder, exist_ok=True)
        _log(f"Prepare: job {job.job_id}, {frame_count} frame(s) of {source_width}x{source_height} at {fps:.6g} fps -> "
             f"LTX {sizes['ltx_width']}x{sizes['ltx_height']}, {len(anchors_at)} anchor(s) of "
             f"{sizes['anchor_width']}x{sizes['anchor_height']} ({anchor_interval}); {fit_mode}, {resize_method}.")
        geometry = {which: ops.resize_geometry(source_height, source_width, sizes[which + "_width"], sizes[which + "_height"], fit_mode)
                    for which in ("ltx", "anchor")}
        ltx_frames, ltx_bytes, anchors, anchor_bytes = _prepare_pixels(video_frames, geometry["ltx"], geometry["anchor"], anchors_at, resize_method)
        _save_image_batch(anchor_bytes, job.anchors, "anchor")
        _save_image_batch(ltx_bytes, job.frames, "frame")
        _encode_mp4(job.frames, frame_count, fps, job.video)

        known = dict(sizes, version=1, job_id=job.job_id, job_folder=job.folder, original_frames=video_frames, source_width=source_width,
                     source_height=source_height, frame_count=frame_count, fps=fps, anchor_indices=anchors_at,
                     anchor_sources_folder=job.anchors, ltx_video_path=job.video, fit_mode=fit_mode, resize_method=resize_method)
        context = {key: known[key] for key in _CONTEXT_KEYS}
        _log(f"Prepare: job {job.job_id} done, working video at {job.video}.")
        results = dict(context, ltx_working_frames=ltx_frames, anchor_images=anchors, anchor_count=len(anchors_at),
                       anchor_indices=",".join(str(i) for i in anchors_at), video_enhance_context=context)
        return tuple(results[name] for name in self.RETURN_NAMES)


PREPARE_NODE_CLASS_MAPPINGS = {
    "VRGDGVideoEnhancePrepare": VRGDGVideoEnhancePrepare,
}


PREPARE_NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDGVideoEnhancePrepare": "Video Enhance - Prepare Video and Anchors",
}

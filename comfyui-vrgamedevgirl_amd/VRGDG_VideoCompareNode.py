"""VRGDG_VideoCompareSlider of the reference (VRGDG_VideoCompareNode.py) with its pixel work on the GPU.

The node turns a *before* and an *after* IMAGE batch into two H.264 previews through an ffmpeg pipe that takes rgb24 bytes.  The
reference downloads each fp32 batch whole (12 B/px, 16 with alpha) and quantises it frame by frame with numpy.  Here each connected
batch goes through ``ops.stream_rgb24``: quantised where it lives (csrc/vrg_compare.hip), downloaded as bytes (3 B/px) in pieces into
page-locked memory, and written to the pipe while the next piece is on its way.  A pending result of this pack -- the usual *after*
input -- is read in HBM and never becomes fp32 on the host.

The node keeps the reference's key, display name, ``INPUT_TYPES``, return types, ``FUNCTION``, ``OUTPUT_NODE``, ``CATEGORY``, its
``ui`` / ``result`` dictionary, the 24 fps of image inputs, the temp-folder file names, the ffmpeg command line and the error texts.
The legacy ``VHS_FILENAMES`` inputs are resolved by ``resolve_video_path`` (host logic, held to the reference by
tests/golden/compare_paths.json).

Seams, module attributes looked up when the node runs, so that the module imports without ComfyUI and without ffmpeg:
``folder_paths()`` returns ComfyUI's module of that name; ``video_writer(path, width, height, fps)`` returns an object with
``write(buffer)`` and ``close()`` (and, optionally, ``abort()`` for a hand-off that failed).  The module has mappings of its own
(register them as INTEGRATION.md shows).  The reference's save-recording route, its JavaScript widget and VRGDG_ImageCompare (one frame
through ComfyUI's PreviewImage) stay the reference's.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import tempfile
import uuid

import numpy as np
import torch

from . import ops

IMAGE_FPS = 24.0
VIDEO_SUFFIXES = frozenset((".mp4", ".mov", ".webm", ".mkv", ".avi", ".m4v"))
_NAME_KEYS = ("fullpath", "path", "video_path", "filename")
_LIST_KEYS = ("files", "filenames", "videos", "gifs")
_NO_FFMPEG = "The compare slider needs FFmpeg to convert IMAGE batches into a browser-playable video."


def folder_paths():
    """ComfyUI's ``folder_paths`` module"""
    import folder_paths as module
    return module


def find_ffmpeg():
    """the ffmpeg on the PATH, else imageio_ffmpeg's, else None"""
    found = shutil.which("ffmpeg")
    if found:
        return found
    try:
        import imageio_ffmpeg
        return imageio_ffmpeg.get_ffmpeg_exe()
    except Exception:
        return None


class FfmpegWriter:
    """rgb24 frames of ``width`` x ``height`` on stdin to an H.264 file at ``path``: the reference's command line.  ffmpeg's messages go
    to a temporary file, so a long encode cannot fill a pipe nobody reads."""

    def __init__(self, path, width, height, fps):
        executable = find_ffmpeg()
        if not executable:
            raise RuntimeError(_NO_FFMPEG)
        command = [
            executable, "-y",
            "-f", "rawvideo", "-vcodec", "rawvideo",
            "-pix_fmt", "rgb24", "-s", f"{int(width)}x{int(height)}",
            "-r", str(max(1.0, float(fps))), "-i", "-",
            "-an", "-c:v", "libx264", "-pix_fmt", "yuv420p",
            "-movflags", "+faststart", path,
        ]
        self.messages = tempfile.TemporaryFile()
        self.process = subprocess.Popen(command, stdin=subprocess.PIPE, stdout=subprocess.DEVNULL, stderr=self.messages)

    def write(self, buffer):
        self.process.stdin.write(buffer)

    def abort(self):
        if self.process.poll() is None:
            self.process.kill()
            self.process.wait()
        self.messages.close()

    def close(self):
        try:
            self.process.stdin.close()
            code = self.process.wait()
            if code != 0:
                self.messages.seek(0)
                text = self.messages.read().decode("utf-8", errors="replace")
                raise RuntimeError(f"FFmpeg could not create the compare video: {text[-1000:]}")
        finally:
            self.abort()


def video_writer(path, width, height, fps):
    return FfmpegWriter(path, width, height, fps)


def video_path_candidates(value) -> list:
    """every string a ``VHS_FILENAMES`` value may name its video by, in the order met: a string itself; of a dictionary its name keys, then
    what its list keys hold; of a list or tuple what its items hold"""
    if isinstance(value, str):
        return [value]
    if isinstance(value, dict):
        found = [value[key] for key in _NAME_KEYS if isinstance(value.get(key), str)]
        for key in _LIST_KEYS:
            found += video_path_candidates(value.get(key))
        return found
    if isinstance(value, (list, tuple)):
        return [name for item in value for name in video_path_candidates(item)]
    return []


def resolve_video_path(value, label) -> str:
    """The last candidate of ``value`` that has a video suffix and names a file -- as it stands, or under ComfyUI's output, temp or input
    folder, in that order -- as a normalised absolute path; the reference's ValueError where there is none."""
    paths = folder_paths()
    roots = ("", paths.get_output_directory(), paths.get_temp_directory(), paths.get_input_directory())
    for name in reversed(video_path_candidates(value)):
        text = str(name or "").strip().strip('"')
        if not text or os.path.splitext(text)[1].lower() not in VIDEO_SUFFIXES:
            continue
        for root in roots:
            path = os.path.join(root, text) if root and not os.path.isabs(text) else text
            path = os.path.normpath(os.path.abspath(path))
            if os.path.isfile(path):
                return path
    raise ValueError(f"{label} video was not found. Connect the Filenames output from a "
                     "Video Combine node that has already created a video.")


def write_image_batch_video(images, label, fps) -> str:
    """One IMAGE batch as ``<temp>/vrgdg_compare_<label>_<32 hex>.mp4``: ``ops.stream_rgb24`` into ``video_writer``."""
    if isinstance(images, np.ndarray):
        images = torch.from_numpy(np.ascontiguousarray(images))
    shape = tuple(int(v) for v in getattr(images, "shape", ()))
    shape = (1,) + shape if len(shape) == 3 else shape
    if not isinstance(images, torch.Tensor) or len(shape) != 4 or shape[0] < 1 or shape[3] < 3:
        raise ValueError(f"{label} image input must be a non-empty IMAGE batch.")
    if images.dtype != torch.float32:
        images = images.to(torch.float32)
    height, width = shape[1], shape[2]
    folder = folder_paths().get_temp_directory()
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, f"vrgdg_compare_{label.lower()}_{uuid.uuid4().hex}.mp4")
    writer = video_writer(path, width, height, fps)
    try:
        ops.stream_rgb24(images, writer.write)
    except BaseException:
        getattr(writer, "abort", lambda: None)()
        raise
    writer.close()
    return path


class VRGDG_VideoCompareSlider:
    @classmethod
    def INPUT_TYPES(cls):
        unit = {"default": 0.5, "min": 0.0, "max": 1.0, "step": 0.01, "tooltip": "Starting position of the before/after wipe."}
        seconds = {"default": 5.0, "min": 0.5, "max": 300.0, "step": 0.5,
                   "tooltip": "How long the browser Record button captures the labeled slider preview."}
        return {
            "required": {
                "slider_position": ("FLOAT", unit),
                "before_label": ("STRING", {"default": "Before", "tooltip": "Label shown over the original video."}),
                "after_label": ("STRING", {"default": "After", "tooltip": "Label shown over the processed video."}),
                "show_labels": ("BOOLEAN", {"default": True}),
                "loop": ("BOOLEAN", {"default": True}),
                "muted": ("BOOLEAN", {"default": True, "tooltip": "Mute playback. When unmuted, audio comes from the before video."}),
                "record_duration": ("FLOAT", seconds),
            },
            "optional": {
                "before_images": ("IMAGE", {"tooltip": "Connect the IMAGE output from a video loader for the original video."}),
                "after_images": ("IMAGE", {"tooltip": "Connect the IMAGE output from a video loader for the processed video."}),
                "before_video": ("VHS_FILENAMES", {"tooltip": "Legacy: connect a Filenames output for the original video."}),
                "after_video": ("VHS_FILENAMES", {"tooltip": "Legacy: connect a Filenames output for the processed video."}),
            },
        }

    RETURN_TYPES = ("VHS_FILENAMES", "VHS_FILENAMES")
    RETURN_NAMES = ("before_video", "after_video")
    FUNCTION = "compare"
    OUTPUT_NODE = True
    CATEGORY = "VRGDG/Image"

    def compare(self, slider_position, before_label, after_label, show_labels, loop, muted, record_duration, before_images=None,
                after_images=None, before_video=None, after_video=None):
        # an IMAGE input wins over the legacy input of its side
        sides = []
        for images, legacy, role in ((before_images, before_video, "before"), (after_images, after_video, "after")):
            path = write_image_batch_video(images, role, IMAGE_FPS) if images is not None else resolve_video_path(legacy, role.capitalize())
            sides.append({"compare_role": role, "path": path, "name": os.path.basename(path)})
        settings = {
            "slider_position": float(slider_position),
            "before_label": str(before_label or "Before"),
            "after_label": str(after_label or "After"),
            "show_labels": bool(show_labels),
            "loop": bool(loop),
            "muted": bool(muted),
            "record_duration": max(0.5, float(record_duration)),
        }
        return {"ui": {"compare_videos": sides, "compare_video_settings": settings},
                "result": tuple((True, [side["path"]]) for side in sides)}


NODE_CLASS_MAPPINGS = {
    "VRGDG_VideoCompareSlider": VRGDG_VideoCompareSlider,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDG_VideoCompareSlider": "VRGDG Video Compare Slider",
}

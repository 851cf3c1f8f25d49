"""The assembly nodes of the music-video automation on the GPU: VRGDG_CombinevideosV2 and VRGDG_CombinevideosV3 (HumoAutomation.py:50-133,
:892-1030 of the reference), VRGDG_CombinevideosV5 (HumoAutomationExtra2.py:309-498), VRGDG_PadVideoWithLastFrame
(GeneralVideoNodes.py:1945-1987) and VRGDG_LoadVideos (nodes.py:1327-1377).

The reference trims, pads and joins up to 16 clips on one CPU thread, and with ``with_labels`` V5 walks every frame four more times in
numpy to build the bytes of its labelled MP4.  Here ``ops.assemble_plan`` restates the integer arithmetic on the host and ONE launch
(csrc/vrg_assemble.hip) writes the joined batch; V5's launch also writes the writer's B,G,R bytes, bar and label included, from the same
read.  Clips on the GPU stay there; of CPU clips only the kept frames are uploaded and the batch comes back on the intermediate device.
Names, ``INPUT_TYPES``, return types, ``FUNCTION``, ``CATEGORY`` and error texts are the reference's.

The labelled bytes equal the reference's for finite pixels with ``0 <= x * 255 < 256`` -- every real IMAGE; its ``astype(uint8)`` is
undefined outside that range, where this pack saturates to 0 / 255 and turns NaN into 0.

Three seams are module attributes a caller may replace.  ``label_renderer``: the 60-row label bar of a clip as B,G,R bytes
(``cv2.putText``; without ``cv2`` the bar is black).  ``video_writer``: the MP4 writer of ``_save_video``; it receives the B,G,R byte
batch, the file's path and ``fps``.  ``video_decoder``: the frames of one file as uint8 R,G,B (imageio).  ``folder_paths`` is looked up
when a relative folder is first resolved, so this module imports without ComfyUI, ``cv2`` and ``imageio``.  It has mappings of its own
(register them as INTEGRATION.md shows).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops

BAR_HEIGHT = ops.ASSEMBLE_BAR


def label_renderer(text, width):
    """the label bar of ``_add_label_bar``: white ``text`` centred on black, uint8 ``[60, width, 3]`` B,G,R -- or None (a black bar)
    where ``cv2`` is not installed"""
    try:
        import cv2
    except ImportError:
        return None
    bar = np.zeros((BAR_HEIGHT, int(width), 3), dtype=np.uint8)
    size = cv2.getTextSize(text, cv2.FONT_HERSHEY_SIMPLEX, 1.0, 2)[0]
    cv2.putText(bar, text, ((int(width) - size[0]) // 2, int(BAR_HEIGHT * 0.7)), cv2.FONT_HERSHEY_SIMPLEX, 1.0, (255, 255, 255), 2, cv2.LINE_AA)
    return bar


def video_writer(frames_bgr, path, fps):
    """``frames_bgr``: uint8 ``[N, H, W, 3]`` B,G,R on the host -> the MP4 at ``path`` (``cv2.VideoWriter``, mp4v)"""
    import cv2
    frames = np.asarray(frames_bgr)
    writer = cv2.VideoWriter(path, cv2.VideoWriter_fourcc(*"mp4v"), fps, (int(frames.shape[2]), int(frames.shape[1])))
    for frame in frames:
        writer.write(frame)
    writer.release()
    return path


def video_decoder(path):
    """the frames of the file at ``path``, uint8 ``[F, H, W, 3]`` R,G,B (``imageio``'s ffmpeg reader), or None for a file without frames"""
    import imageio
    reader = imageio.get_reader(path, "ffmpeg")
    frames = [np.asarray(frame) for frame in reader]
    reader.close()
    return np.stack(frames) if frames else None


def _output_directory():
    import folder_paths
    return folder_paths.get_output_directory()


def _slots(kwargs):
    return [kwargs.get(f"video_{i}") for i in range(1, ops.ASSEMBLE_SLOTS + 1)]


def _shapes(videos):
    return [None if v is None else tuple(v.shape) for v in videos]


def _join(videos, plan):
    if not plan:
        raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")         # what the reference's cat of no clips raises
    return ops.assemble_frames(videos, plan)


def _video_inputs():
    return {f"video_{i}": ("IMAGE",) for i in range(1, ops.ASSEMBLE_SLOTS + 1)}


class VRGDG_CombinevideosV2:
    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("blended_video_frames",)
    FUNCTION = "blend_videos"
    CATEGORY = "Video"

    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "fps": ("FLOAT", {"default": 25.0, "min": 1.0}),
                "audio_meta": ("DICT",),
            },
            "optional": {**_video_inputs()},
        }

    def blend_videos(self, fps, audio_meta, **kwargs):
        videos = _slots(kwargs)
        return (_join(videos, ops.assemble_plan("v2", _shapes(videos), fps, audio_meta)),)


class VRGDG_CombinevideosV3:
    VERSION = "v3.1_fixed"
    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("blended_video_frames",)
    FUNCTION = "blend_videos"
    CATEGORY = "Video"

    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "fps": ("FLOAT", {"default": 25.0, "min": 1.0}),
                "duration": ("FLOAT", {"default": 4.0, "min": 0.01}),
                "audio_meta": ("DICT",),
                "index": ("INT", {"default": 0, "min": 0}),
                "total_sets": ("INT", {"default": 1, "min": 1}),
                "groups_in_last_set": ("INT", {"default": 16, "min": 0, "max": 16}),
            },
            "optional": {**_video_inputs()},
        }

    def blend_videos(self, fps, duration, audio_meta=None, index=0, total_sets=1, groups_in_last_set=16, **kwargs):
        videos = _slots(kwargs)
        return (_join(videos, ops.assemble_plan("v3", _shapes(videos), fps, audio_meta, index, total_sets, groups_in_last_set)),)


class VRGDG_CombinevideosV5:
    VERSION = "v3.9_label_safe"
    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("blended_video_frames",)
    FUNCTION = "blend_videos"
    CATEGORY = "Video"

    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "fps": ("FLOAT", {"default": 25.0, "min": 1.0}),
                "duration": ("FLOAT", {"default": 4.0, "min": 0.01}),
                "audio_meta": ("DICT",),
                "index": ("INT", {"default": 0, "min": 0}),
                "total_sets": ("INT", {"default": 1, "min": 1}),
                "groups_in_last_set": ("INT", {"default": 16, "min": 0, "max": 16}),
                "folder_path": ("STRING", {"default": "./output_videos"}),
                "with_labels": ("BOOLEAN", {
                    "default": True,
                    "label": "Add Labels and Save Video",
                    "tooltip": "If enabled, adds label bars and saves labeled video to WithLabels/."
                }),
            },
            "optional": {**_video_inputs()},
        }

    def _save_video(self, frames_bgr, folder_path, filename, fps):
        """the reference's ``_save_video`` after its per-frame quantisation, which the launch has already done"""
        folder_path = folder_path.strip()
        if not os.path.isabs(folder_path):
            folder_path = os.path.join(_output_directory(), folder_path)
        os.makedirs(folder_path, exist_ok=True)
        return video_writer(frames_bgr, os.path.join(folder_path, filename), fps)

    def blend_videos(self, fps, duration, audio_meta=None, index=0, total_sets=1, groups_in_last_set=16, folder_path="./output_videos",
                     with_labels=True, **kwargs):
        videos = _slots(kwargs)
        plan = ops.assemble_plan("v5", _shapes(videos), fps, audio_meta, index, total_sets, groups_in_last_set)
        if not with_labels:
            return (_join(videos, plan),)
        if not plan:
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")
        width = int(videos[plan[0][0]].shape[2])
        overlays = [None] * len(videos)
        for slot in sorted({s for s, _ in plan}):
            overlays[slot] = label_renderer(f"set {index+1} - group {slot + 1}", width)
        data, final = ops.assemble_labelled_bytes(videos, plan, overlays, clean_out=True)
        self._save_video(data.cpu().numpy(), os.path.join(folder_path, "WithLabels"), f"set{index+1}_combined.mp4", fps)
        return (final,)


class VRGDG_PadVideoWithLastFrame:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "images": ("IMAGE",),
                "pad_frames": ("INT", {
                    "default": 1,
                    "min": 0,
                    "max": 1000,
                    "step": 1
                }),
                "pad_front": ("BOOLEAN", {
                    "default": False
                }),
            }
        }

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("images",)
    FUNCTION = "pad_video"
    CATEGORY = "video/utils"

    def pad_video(self, images, pad_frames, pad_front):
        if images.shape[0] == 0 or pad_frames <= 0:
            return (images,)
        return (ops.assemble_frames([images], ops.assemble_plan("pad", [tuple(images.shape)], pad_frames=pad_frames, pad_front=pad_front)),)


class VRGDG_LoadVideos:
    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("video",)
    FUNCTION = "load_videos"
    CATEGORY = "Video"

    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "trigger": ("*", {}),
                "video_folder": ("STRING", {"default": "./videos", "multiline": False}),
                "scene_count": ("INT", {"default": 3, "min": 1, "max": 5}),
            }
        }

    def load_videos(self, trigger, video_folder, scene_count=3):
        videos = sorted(f for f in os.listdir(video_folder) if f.lower().endswith((".mp4", ".mov", ".avi", ".mkv")))
        if not videos:
            raise ValueError(f"No video files found in {video_folder}")
        clips = []
        for name in videos[:scene_count]:
            frames = video_decoder(os.path.join(video_folder, name))
            if frames is not None and len(frames):
                clips.append(torch.from_numpy(np.ascontiguousarray(frames)))        # the bytes go up: 3 B/px instead of 12
        if not clips:
            raise ValueError("No frames loaded from any videos.")
        return (ops.assemble_frames(clips, ops.assemble_plan("load", [tuple(c.shape) for c in clips])),)


ASSEMBLY_NODE_CLASS_MAPPINGS = {
    "VRGDG_CombinevideosV2": VRGDG_CombinevideosV2,
    "VRGDG_CombinevideosV3": VRGDG_CombinevideosV3,
    "VRGDG_CombinevideosV5": VRGDG_CombinevideosV5,
    "VRGDG_PadVideoWithLastFrame": VRGDG_PadVideoWithLastFrame,
    "VRGDG_LoadVideos": VRGDG_LoadVideos,
}

ASSEMBLY_NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDG_CombinevideosV2": "🌀 VRGDG_CombinevideosV2",
    "VRGDG_CombinevideosV3": "🎬 VRGDG Combine Videos V3",
    "VRGDG_CombinevideosV5": "VRGDG_CombinevideosV5",
    "VRGDG_PadVideoWithLastFrame": "VRGDG_PadVideoWithLastFrame",
    "VRGDG_LoadVideos": "VRGDG_LoadVideos",
}

"""Video Folder Grid Plot on the MI355X: `VRGDG_VideoFolderGridPlot` of the reference's LTXLoraTrain.py with the same name, widget specs,
return values and status strings; the pixels come from csrc/vrg_grid.hip (ops.video_grid / ops.video_grid_bytes): every tile of every
output frame is quantised, resized as cv2.resize(..., INTER_AREA) does and written as fp32 / 255 into its place in the grid frame in one
launch, instead of one single-threaded cv2 resize per tile and frame on the CPU.

What is here: the node alone.  It has no parent class: `_choose_columns`, `_safe_name`, `LABEL_BAND_HEIGHT` and `VIDEO_EXTENSIONS` of the
reference's VRGDG_LTXPreviewXYZPlot are restated in it.  Two things stay outside the GPU and are seams of this module:
  render_label(text, cell_w, cell_h, band)   the label of one tile on a zero canvas, uint8 [cell_h, cell_w, 3]; the default calls
                                             cv2.putText with the reference's parameters and needs cv2
  open_capture(path)                         an object with read() -> (ok, B,G,R uint8 frame) and release(); the default is
                                             cv2.VideoCapture and needs cv2
A label that leaves the band (any non-zero byte at or below row `band`) would be blended over moving pixels by the reference; that is not
reproduced and raises ValueError.

What is NOT here: the other nodes of LTXLoraTrain.py, and the registration in the package's NODE_CLASS_MAPPINGS (INTEGRATION.md shows the
two lines that merge this module's mapping).
"""
from __future__ import annotations

import math
import os
import re

import numpy as np
import torch

from . import ops
from ._devices import intermediate_device

FOLDER_PIECE_FRAMES = 16            # output frames of the folder branch that go through one launch


def _cv2(what):
    try:
        import cv2  # type: ignore
    except Exception as exc:
        raise RuntimeError(f"VRGDG_VideoFolderGridPlot: {what} needs cv2 (opencv-python), which cannot be imported here: {exc}") from exc
    return cv2


def render_label(text, cell_w, cell_h, band):
    """The label `_fit_frame_to_tile` draws (LTXLoraTrain.py:8076-8084 of the reference), on a zero canvas: uint8 [cell_h, cell_w, 3]."""
    cv2 = _cv2("drawing tile labels")
    canvas = np.zeros((int(cell_h), int(cell_w), 3), dtype=np.uint8)
    font = cv2.FONT_HERSHEY_SIMPLEX
    font_scale = max(0.45, min(1.0, float(cell_w) / 420.0))
    thickness = 2
    text = str(text or "")
    text_size, baseline = cv2.getTextSize(text, font, font_scale, thickness)
    text_x = max(8, (int(cell_w) - text_size[0]) // 2)
    text_y = max(text_size[1] + 6, (int(band) + text_size[1]) // 2 - baseline)
    cv2.putText(canvas, text, (text_x, text_y), font, font_scale, (255, 255, 255), thickness, cv2.LINE_AA)
    return canvas


def open_capture(path):
    """The decoder of one video file: read() -> (ok, B,G,R uint8 [H, W, 3]) and release()."""
    cap = _cv2("decoding video files").VideoCapture(path)
    if not cap.isOpened():
        raise RuntimeError(f"Could not open video for grid render: {path}")
    return cap


def _overlays(labels, cell_w, cell_h, band):
    """The first `band` rows of every tile's label as R,G,B bytes (the reference draws on the B,G,R tile and flips the grid)."""
    out = []
    for text in labels:
        canvas = np.asarray(render_label(text, cell_w, cell_h, band))
        if canvas.dtype != np.uint8 or canvas.shape != (cell_h, cell_w, 3):
            raise ValueError(f"render_label must return uint8 [{cell_h}, {cell_w}, 3]")
        if canvas[band:].any():
            raise ValueError(f"VRGDG_VideoFolderGridPlot: the label {str(text)!r} leaves the {band}-row band of a {cell_w} x {cell_h} tile; "
                             "the reference blends it over the picture there, which is not reproduced")
        out.append(np.ascontiguousarray(canvas[:band, :, ::-1]))
    return out


_TOOLTIPS = {
    "video_folder": "Folder containing the videos to place into the grid. Leave this as the source, or connect explicit video inputs below if you want to include only selected videos.",
    "output_name": "Base filename prefix to send downstream into a video combine node.",
    "filename_prefix": "Filename prefix to pass downstream to a video combine node. Example: VRGDG/MyGrid or tests/compare_grid.",
    "video_count": "How many explicit video input slots and matching label fields to show. If any connected video inputs are present, those are used instead of scanning the folder.",
    "cell_width": "Width of each tile. Use 0 to auto-detect from the first video.",
    "cell_height": "Height of each tile. Use 0 to auto-detect from the first video. If labels are enabled, the label band is added automatically.",
    "label_tiles": "Adds a label above each tile using the video filename.",
    "output_fps": "FPS to pass downstream to a video combine node.",
}


class VRGDG_VideoFolderGridPlot:
    RETURN_TYPES = ("IMAGE", "STRING", "INT", "STRING")
    RETURN_NAMES = ("images", "filename_prefix", "output_fps", "status")
    FUNCTION = "run"
    CATEGORY = "VRGDG/Video"
    DESCRIPTION = (
        "Creates a simple labeled grid image sequence from videos in a folder or connected inputs."
    )
    MAX_VIDEO_SLOTS = 20
    VIDEO_EXTENSIONS = {".mp4", ".mov", ".mkv", ".webm", ".avi"}
    LABEL_BAND_HEIGHT = 40

    @classmethod
    def INPUT_TYPES(cls):
        slots = range(1, cls.MAX_VIDEO_SLOTS + 1)
        optional = {f"video{i}": ("IMAGE", {"forceInput": True}) for i in slots}
        optional.update({f"label_{i}": ("STRING", {"default": "", "multiline": False}) for i in slots})

        def text(name, default):
            return ("STRING", {"default": default, "multiline": False, "tooltip": _TOOLTIPS[name]})

        def number(name, default, low, high):
            return ("INT", {"default": default, "min": low, "max": high, "step": 1, "tooltip": _TOOLTIPS[name]})

        return {
            "required": {
                "video_folder": text("video_folder", ""),
                "output_name": text("output_name", "VideoGrid"),
                "filename_prefix": text("filename_prefix", "VRGDG/VideoGrid"),
                "video_count": number("video_count", 4, 1, cls.MAX_VIDEO_SLOTS),
                "cell_width": number("cell_width", 0, 0, 4096),
                "cell_height": number("cell_height", 0, 0, 4096),
                "label_tiles": ("BOOLEAN", {"default": True, "tooltip": _TOOLTIPS["label_tiles"]}),
                "output_fps": number("output_fps", 24, 1, 120),
            },
            "optional": optional,
        }

    # ---- restated from the reference's VRGDG_LTXPreviewXYZPlot ----
    @staticmethod
    def _safe_name(value, default_value):
        raw = str(value or "").strip() or default_value
        cleaned = re.sub(r"[^A-Za-z0-9._-]+", "_", raw)
        return cleaned.strip("._-") or default_value

    @staticmethod
    def _choose_columns(item_count):
        if item_count <= 0:
            return 1
        return max(1, math.ceil(math.sqrt(item_count)))

    @staticmethod
    def _resolve_preview_folder(preview_folder):
        preview_folder = str(preview_folder or "").strip()
        if not preview_folder:
            raise ValueError("preview_folder is required.")
        if os.path.isabs(preview_folder):
            resolved = preview_folder
        else:
            import folder_paths  # type: ignore  -- ComfyUI's
            resolved = os.path.join(folder_paths.get_output_directory(), preview_folder)
        resolved = os.path.normpath(resolved)
        if not os.path.isdir(resolved):
            parent = os.path.dirname(resolved)
            if parent and os.path.isdir(parent):
                return parent
            raise ValueError(f"preview_folder does not exist: {resolved}")
        return resolved

    # ---- the node's own helpers ----
    def _find_all_videos(self, video_folder):
        matches = []
        for entry in os.scandir(video_folder):
            name = entry.name
            if not entry.is_file() or os.path.splitext(name)[1].lower() not in self.VIDEO_EXTENSIONS:
                continue
            if "_XYZ_COMPARE_" in name.upper() or "_VIDEOGRID_" in name.upper():
                continue
            matches.append((name.lower(), entry.stat().st_mtime, entry.path))
        matches.sort()
        return [os.path.normpath(item[2]) for item in matches]

    def _extract_image_batches_from_value(self, value):
        if isinstance(value, torch.Tensor):
            return [value.unsqueeze(0)] if value.ndim == 3 else ([value] if value.ndim == 4 else [])
        if isinstance(value, dict):
            value = list(value.values())
        if isinstance(value, (list, tuple, set)):
            return [b for nested in value for b in self._extract_image_batches_from_value(nested)]
        return []

    def _collect_selected_image_batches(self, kwargs):
        return [b for i in range(1, self.MAX_VIDEO_SLOTS + 1) for b in self._extract_image_batches_from_value(kwargs.get(f"video{i}"))]

    def _collect_dynamic_labels(self, kwargs):
        return [str(kwargs.get(f"label_{i}", "") or "").strip() for i in range(1, self.MAX_VIDEO_SLOTS + 1)]

    def _resolve_labels(self, defaults, kwargs):
        labels = self._collect_dynamic_labels(kwargs)
        return [(labels[i] if i < len(labels) else "") or default for i, default in enumerate(defaults)]

    def _cell_size(self, first_size, cell_width, cell_height, label_tiles):
        """`first_size`: a callable giving (width, height) of the first source; asked only when a side is 0"""
        cell_width, cell_height = int(cell_width), int(cell_height)
        if cell_width > 0 and cell_height > 0:
            return cell_width, cell_height
        width, height = first_size()
        if cell_width <= 0:
            cell_width = width
        if cell_height <= 0:
            cell_height = height + (self.LABEL_BAND_HEIGHT if label_tiles else 0)
        return int(cell_width), int(cell_height)

    @staticmethod
    def _result(grid, like_cpu):
        return grid.to(intermediate_device()) if like_cpu else grid

    def _build_grid_frames_from_images(self, image_batches, cell_width, cell_height, columns, label_tiles, tile_labels):
        band = self.LABEL_BAND_HEIGHT if label_tiles else 0
        overlays = _overlays(tile_labels, cell_width, cell_height, band) if label_tiles else None
        grid = ops.video_grid(image_batches, cell_width, cell_height, columns, band, overlays)
        return self._result(grid, not any(b.is_cuda for b in image_batches))

    def _build_grid_frames(self, video_paths, cell_width, cell_height, columns, label_tiles, tile_labels):
        """The read loop of the reference (:8104-8154): every video holds its last frame, one that never gave a frame shows black, the
        loop stops when all are finished; the frames go to the GPU FOLDER_PIECE_FRAMES output frames at a time."""
        band = self.LABEL_BAND_HEIGHT if label_tiles else 0
        overlays = _overlays(tile_labels, cell_width, cell_height, band) if label_tiles else None
        captures = [open_capture(path) for path in video_paths]
        n = len(captures)
        finished, pieces = [False] * n, []
        store = [[] for _ in range(n)]          # the frames this piece shows: the held one first, then those read since the last launch
        index = [[] for _ in range(n)]          # per output frame of this piece: which frame of store, -1 = none yet

        def flush():
            if not index[0]:
                return
            batches = [torch.from_numpy(np.stack(frames)) if frames else None for frames in store]
            pieces.append(ops.video_grid_bytes(batches, index, cell_width, cell_height, columns, band, overlays))
            for i in range(n):
                store[i], index[i] = store[i][-1:], []

        try:
            while captures:
                for i, cap in enumerate(captures):
                    if not finished[i]:
                        ok, frame = cap.read()
                        if ok and frame is not None:
                            store[i].append(np.ascontiguousarray(frame, dtype=np.uint8))
                        else:
                            finished[i] = True
                if all(finished):                   # nothing fresh in this round: the reference leaves without a frame
                    break
                for i in range(n):
                    index[i].append(len(store[i]) - 1)
                if len(index[0]) >= FOLDER_PIECE_FRAMES:
                    flush()
            flush()
        finally:
            for cap in captures:
                cap.release()
        if not pieces:
            raise RuntimeError("No grid frames could be created from the provided videos.")
        return self._result(pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=0), True)

    def _first_video_size(self, path):
        cap = open_capture(path)
        try:
            ok, frame = cap.read()
        finally:
            cap.release()
        if not ok or frame is None:
            raise RuntimeError(f"Could not determine video resolution: {path}")
        return int(frame.shape[1]), int(frame.shape[0])

    def run(self, video_folder, output_name, filename_prefix, video_count, cell_width, cell_height, label_tiles, output_fps, **kwargs):
        selected = self._collect_selected_image_batches(kwargs)
        if selected:
            item_count = len(selected)
            output_name = self._safe_name(output_name, "VideoGrid")
            tile_labels = self._resolve_labels([f"video{i + 1}" for i in range(item_count)], kwargs)
            cell_width, cell_height = self._cell_size(lambda: (int(selected[0].shape[2]), int(selected[0].shape[1])), cell_width, cell_height,
                                                      bool(label_tiles))
            columns = self._choose_columns(item_count)
            grid_frames = self._build_grid_frames_from_images(selected, cell_width, cell_height, int(columns), bool(label_tiles), tile_labels)
            source_status = f"Created grid image sequence from {item_count} connected video/image input(s)."
        else:
            video_folder = self._resolve_preview_folder(video_folder)
            output_name = self._safe_name(output_name, self._safe_name(os.path.basename(video_folder), "VideoGrid"))
            video_paths = self._find_all_videos(video_folder)
            tile_labels = self._resolve_labels([os.path.splitext(os.path.basename(p))[0] for p in video_paths], kwargs)
            if not video_paths:
                return (
                    torch.zeros((1, 64, 64, 3), dtype=torch.float32),
                    str(filename_prefix or output_name),
                    int(output_fps),
                    f"No video files were found in {video_folder}. Connect video inputs or point video_folder at a folder with videos.",
                )
            cell_width, cell_height = self._cell_size(lambda: self._first_video_size(video_paths[0]), cell_width, cell_height, bool(label_tiles))
            columns = self._choose_columns(len(video_paths))
            grid_frames = self._build_grid_frames(video_paths, cell_width, cell_height, int(columns), bool(label_tiles), tile_labels)
            item_count = len(video_paths)
            source_status = f"Created grid image sequence from {item_count} videos."
        rows = int(math.ceil(item_count / max(1, int(columns))))
        resolved_prefix = str(filename_prefix or output_name or "VRGDG/VideoGrid").strip() or "VRGDG/VideoGrid"
        print(f"[VRGDG] Creating folder grid image sequence using a {int(columns)}x{int(rows)} grid at {int(cell_width)}x{int(cell_height)} per tile.")
        return (grid_frames, resolved_prefix, int(output_fps), source_status)


NODE_CLASS_MAPPINGS = {"VRGDG_VideoFolderGridPlot": VRGDG_VideoFolderGridPlot}
NODE_DISPLAY_NAME_MAPPINGS = {"VRGDG_VideoFolderGridPlot": "VRGDG Video Folder Grid Plot"}

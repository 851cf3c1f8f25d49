"""The three reference sheets of the AI Video Builder (VRGDG_MusicVideoBuilderNodes.py:7169-7238 of the reference) on the GPU:
``combine_subject_location_images``, ``combine_flux_ingredient_images`` and ``combine_story_reference_batch`` take PIL images or uint8
``[h, w, 3]`` / ``[h, w]`` arrays and return the PIL image the reference's functions build -- every picture resized with
``Image.resize(..., LANCZOS)`` to ``int()``-truncated sizes and pasted plainly onto a (20, 20, 20) canvas, byte for byte
(``ops.reference_sheet`` with byte sources and byte output).  Nothing else of that module is here.
"""
from __future__ import annotations

import math

import numpy as np

from . import ops

NODE_CLASS_MAPPINGS = {}
NODE_DISPLAY_NAME_MAPPINGS = {}

SHEET_BACKGROUND = (20, 20, 20)


def _rgb(image):
    """uint8 [h, w, 3] of a PIL image (converted to RGB) or an array"""
    if hasattr(image, "convert"):
        image = np.asarray(image.convert("RGB"))
    a = np.ascontiguousarray(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("a sheet picture must be a PIL image or a uint8 array [h, w, 3] / [h, w]")
    return a


def _shrunk(a, scale):
    return max(1, int(a.shape[1] * scale)), max(1, int(a.shape[0] * scale))


def _sheet(arrays, boxes, size):
    from PIL import Image
    panels = [ops.SheetPanel(i, box, "resize") for i, box in enumerate(boxes)]
    out = ops.reference_sheet(arrays, panels, size, SHEET_BACKGROUND, out_bytes=True)
    return Image.fromarray(out.cpu().numpy(), mode="RGB")


def _cells(arrays, cell_size, gap, columns, scale_of):
    rows = int(math.ceil(len(arrays) / columns))
    boxes = []
    for i, a in enumerate(arrays):
        w, h = _shrunk(a, scale_of(a))
        boxes.append(((i % columns) * (cell_size + gap) + (cell_size - w) // 2, (i // columns) * (cell_size + gap) + (cell_size - h) // 2, w, h))
    return boxes, (columns * cell_size + gap * (columns - 1), rows * cell_size + gap * (rows - 1))


def combine_subject_location_images(subject_image, location_image):
    """subject and location side by side, each at most 640 pixels high, 24 pixels apart, centred vertically"""
    arrays = [_rgb(subject_image), _rgb(location_image)]
    sizes = [_shrunk(a, min(1.0, 640 / max(1, a.shape[0]))) for a in arrays]
    gap, height = 24, max(s[1] for s in sizes)
    boxes = [(0, (height - sizes[0][1]) // 2, *sizes[0]), (sizes[0][0] + gap, (height - sizes[1][1]) // 2, *sizes[1])]
    return _sheet(arrays, boxes, (sizes[0][0] + sizes[1][0] + gap, height))


def combine_flux_ingredient_images(images):
    """a near-square grid of cells (384 pixels for up to four pictures, else 256), 24 pixels apart; pictures are never enlarged"""
    if not images:
        raise ValueError("At least one image ingredient is required.")
    arrays = [_rgb(i) for i in images]
    cell = 384 if len(arrays) <= 4 else 256
    columns = 1 if len(arrays) == 1 else int(math.ceil(math.sqrt(len(arrays))))
    boxes, size = _cells(arrays, cell, 24, columns, lambda a: min(1.0, cell / max(1, a.shape[1]), cell / max(1, a.shape[0])))
    return _sheet(arrays, boxes, size)


def combine_story_reference_batch(images, cell_size=512):
    """the first four pictures in cells of ``cell_size`` (two columns, one for a single picture), 16 pixels apart; pictures fill their cell"""
    if not images:
        raise ValueError("At least one Story reference image is required.")
    arrays = [_rgb(i) for i in list(images[:4])]
    boxes, size = _cells(arrays, cell_size, 16, 1 if len(arrays) == 1 else 2, lambda a: min(cell_size / max(1, a.shape[1]), cell_size / max(1, a.shape[0])))
    return _sheet(arrays, boxes, size)

"""VRGDG_LTXICIngredientsGrid of the reference (VRGDG_LTXICIngredientsGrid.py) on the GPU: up to 24 IMAGE inputs quantised to bytes, shrunk
with Pillow's LANCZOS and pasted as panels -- eight layouts, two fit modes, rounded corners -- onto a coloured canvas, returned / 255.

The node keeps the reference's name, ``INPUT_TYPES``, return types, ``FUNCTION``, ``CATEGORY`` and error text, and has mappings of its own
(register them as INTEGRATION.md shows).  The layout arithmetic (``parse_color``, ``layout_rects``, ``aspect_row_rects``,
``panel_rectangles``) is host code in Python doubles, held to the reference by tests/golden/sheet.json: the normalised rectangles equal the
reference's as floats, exactly.  The pixels are ``ops.reference_sheet`` (csrc/vrg_sheet.hip): byte for byte what Pillow gives.

CPU tensors (what ComfyUI hands over) are uploaded frame by frame -- only the frames that are shown, ``[:1]`` of each input under
``first_image_only`` -- and the sheet comes back as the reference returns it: a CPU fp32 ``[1, H, W, 3]``.  Device tensors stay where they
are and give a device tensor.  Inputs are never written.
"""
from __future__ import annotations

import math

import torch

from . import ops
from ._devices import materialise

NAMED_COLORS = {"black": "#000000", "white": "#ffffff", "gray": "#808080", "grey": "#808080", "neutral_gray": "#b8b8b8",
                "neutral_grey": "#b8b8b8"}
ASPECT_LIMITS = (0.05, 20.0)
STORY_RECTS = ((0.0, 0.0, 0.235, 0.52), (0.235, 0.0, 0.385, 0.52), (0.62, 0.0, 0.38, 0.52), (0.0, 0.52, 0.37, 0.23), (0.37, 0.52, 0.63, 0.23),
               (0.0, 0.75, 0.37, 0.25), (0.37, 0.75, 0.63, 0.25))


def _clamped(value, lo, hi):
    return min(hi, max(lo, int(value)))


def parse_color(value, fallback):
    """(R, G, B) of a colour name, ``#rgb`` or ``#rrggbb``; anything else gives the fallback (and black if that is no colour either)"""
    text = str(value or "").strip() or fallback
    text = NAMED_COLORS.get(text.lower(), text)
    digits = text[1:] if text.startswith("#") else text
    if len(digits) == 3:
        digits = "".join(2 * ch for ch in digits)
    if len(digits) != 6:
        digits = fallback.lstrip("#")
    try:
        return tuple(int(digits[i:i + 2], 16) for i in (0, 2, 4))
    except ValueError:
        return parse_color(fallback, "#000000")


def grid_rects(count, columns=None):
    """a uniform grid in row-major order; without ``columns`` as many as a 16:9 sheet of squares would take"""
    if count <= 0:
        return []
    if not columns or columns <= 0:
        columns = int(math.ceil(math.sqrt(count * 16 / 9)))
    columns = max(1, min(count, int(columns)))
    rows = int(math.ceil(count / columns))
    return [((i % columns) / columns, (i // columns) / rows, 1 / columns, 1 / rows) for i in range(count)]


def _row(n, y, height):
    return [(i / n, y, 1 / n, height) for i in range(n)]


def layout_rects(preset, count, columns):
    """the normalised (x, y, w, h) of ``count`` panels under one of the presets other than ``aspect_rows``"""
    if count <= 0:
        return []
    if preset == "horizontal_strip":
        return [(i / count, 0.0, 1 / count, 1.0) for i in range(count)]
    if preset == "vertical_strip":
        return [(0.0, i / count, 1.0, 1 / count) for i in range(count)]
    if preset == "auto_ltx" and count >= 5:
        preset = "six_panel_story" if count in (6, 7) else "three_row_reference"
    if preset == "six_panel_story" and count >= 6:
        if count <= 7:
            return list(STORY_RECTS[:count])
        preset = "three_row_reference"
    if preset == "three_row_reference" and count >= 5:
        if count <= 6:
            top = count // 2
            return _row(top, 0.0, 0.42) + _row(count - top - 1, 0.42, 0.28) + [(0.0, 0.70, 1.0, 0.30)]
        top = min(3, count)
        mid = min(3, count - top)
        return _row(top, 0.0, 0.40) + _row(mid, 0.40, 0.28) + _row(count - top - mid, 0.68, 0.32)
    if preset == "wide_bottom" and count >= 3:
        above = count - 1
        band = 0.68 if above > 4 else 0.56
        rects = [(x, y * band, w, h * band) for x, y, w, h in grid_rects(above, columns if columns > 0 else None)]
        return (rects + [(0.0, band, 1.0, 1.0 - band)])[:count]
    return grid_rects(count, columns if columns > 0 else None)


def _compositions(total, parts):
    """every way to write ``total`` as ``parts`` positive integers, in lexicographic order"""
    if parts <= 1:
        yield [total]
    elif parts >= total:
        yield [1] * total
    else:
        stack = [([], total)]
        while stack:
            head, left = stack.pop()
            remaining_parts = parts - len(head)
            if remaining_parts == 1:
                yield head + [left]
                continue
            for first in range(left - remaining_parts + 1, 0, -1):             # pushed high to low, so popped low to high
                stack.append((head + [first], left - first))


def aspect_row_rects(aspects, canvas_width, canvas_height):
    """``aspect_rows``: rows of panels whose widths follow the pictures' aspects (``aspects``: width / height per picture, limited to
    0.05 .. 20): of all splits into at most four rows the one that fills the canvas best"""
    count = len(aspects)
    if count <= 0:
        return []
    if count == 1:
        return [(0.0, 0.0, 1.0, 1.0)]
    target = max(0.05, canvas_width / max(1, canvas_height))
    best = None
    for rows in range(1, min(count, 4) + 1):
        for split in _compositions(count, rows):
            sums, heights, at = [], [], 0
            for n in split:
                sums.append(sum(aspects[at:at + n]))
                heights.append(target / max(0.05, sums[-1]))
                at += n
            total = sum(heights)
            score = (total - 1.0) * 10.0 + rows * 0.05 if total > 1.02 else (1.0 - total) + rows * 0.035
            score += (max(heights) - min(heights)) * 0.08
            if best is None or score < best[0]:
                best = (score, split, heights, sums, total)
    _, split, heights, sums, total = best
    gap = 0.0
    y = max(0.0, (1.0 - total) / 2.0) if total <= 1.0 else 0.0
    if total < 0.98 and len(split) > 1:
        gap = (1.0 - total) / (len(split) + 1)
        y = gap
    rects, at = [], 0
    for n, height, row_sum in zip(split, heights, sums):
        if total > 1.0:
            height = height / total
        x = max(0.0, (1.0 - height * row_sum / target) / 2.0)
        for _ in range(n):
            width = height * aspects[at] / target
            rects.append((x, y, width, height))
            x += width
            at += 1
        y += height + gap
    return rects


def picture_aspect(width, height):
    if width <= 0 or height <= 0:
        return 1.0
    return max(ASPECT_LIMITS[0], min(ASPECT_LIMITS[1], width / height))


def panel_rectangles(rects, width, height, padding, gutter):
    """(left, top, panel_width, panel_height) on a ``width`` x ``height`` canvas of normalised rects, inset by half the gutter"""
    usable_w, usable_h = max(1, width - 2 * padding), max(1, height - 2 * padding)
    inset = gutter // 2
    out = []
    for x, y, w, h in rects:
        left = padding + int(round(x * usable_w)) + inset
        top = padding + int(round(y * usable_h)) + inset
        right = padding + int(round((x + w) * usable_w)) - inset
        bottom = padding + int(round((y + h) * usable_h)) - inset
        out.append((left, top, max(1, right - left), max(1, bottom - top)))
    return out


def _frames(value, batch_mode):
    """the [H, W, C] frames of one IMAGE input that the sheet shows"""
    if value is None or not isinstance(value, torch.Tensor):
        return []
    t = materialise(value).detach()
    if t.ndim == 3:
        t = t.unsqueeze(0)
    if t.ndim != 4 or int(t.shape[0]) <= 0:
        return []
    if batch_mode == "first_image_only":
        t = t[:1]
    if int(t.shape[-1]) == 2 or min(int(t.shape[1]), int(t.shape[2]), int(t.shape[3])) < 1:
        raise ValueError(f"VRGDG LTX IC Ingredients Grid: an image of shape {tuple(t.shape[1:])} cannot be shown")
    return [t[i] for i in range(int(t.shape[0]))]


class VRGDG_LTXICIngredientsGrid:
    MAX_IMAGES = 24
    LAYOUTS = ["auto_ltx", "aspect_rows", "six_panel_story", "three_row_reference", "wide_bottom", "uniform_grid", "horizontal_strip",
               "vertical_strip"]
    FIT_MODES = ["contain_pad", "cover_crop"]
    BATCH_MODES = ["first_image_only", "all_images"]

    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "image_count": ("INT", {"default": 6, "min": 1, "max": cls.MAX_IMAGES, "step": 1,
                                        "tooltip": "How many dynamic image inputs to show and compose."}),
                "layout": (cls.LAYOUTS, {"default": "auto_ltx"}),
                "output_width": ("INT", {"default": 768, "min": 64, "max": 8192, "step": 8}),
                "output_height": ("INT", {"default": 448, "min": 64, "max": 8192, "step": 8}),
                "columns": ("INT", {"default": 0, "min": 0, "max": 12, "step": 1,
                                    "tooltip": "Uniform grid columns. Use 0 for auto. Some presets ignore this."}),
                "gutter": ("INT", {"default": 4, "min": 0, "max": 128, "step": 1}),
                "outer_padding": ("INT", {"default": 4, "min": 0, "max": 128, "step": 1}),
                "corner_radius": ("INT", {"default": 3, "min": 0, "max": 96, "step": 1}),
                "fit_mode": (cls.FIT_MODES, {"default": "contain_pad"}),
                "batch_mode": (cls.BATCH_MODES, {"default": "first_image_only"}),
                "background_color": ("STRING", {"default": "#000000", "multiline": False}),
                "cell_background_color": ("STRING", {"default": "#b8b8b8", "multiline": False}),
            },
            "optional": {f"image{i}": ("IMAGE", {"forceInput": True, "tooltip": f"Ingredient image {i}."}) for i in range(1, cls.MAX_IMAGES + 1)},
        }

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("reference_sheet",)
    FUNCTION = "build"
    CATEGORY = "VRGDG/LTX"
    DESCRIPTION = "Builds an LTX IC-LoRA Ingredients-style reference sheet from dynamic image inputs."

    def build(self, image_count, layout, output_width, output_height, columns, gutter, outer_padding, corner_radius, fit_mode, batch_mode,
              background_color, cell_background_color, **kwargs):
        frames = []
        for i in range(1, _clamped(image_count, 1, self.MAX_IMAGES) + 1):
            frames.extend(_frames(kwargs.get(f"image{i}"), batch_mode))
        if not frames:
            raise ValueError("VRGDG LTX IC Ingredients Grid needs at least one connected image input.")
        width, height = _clamped(output_width, 64, 8192), _clamped(output_height, 64, 8192)
        gutter, padding = _clamped(gutter, 0, 128), _clamped(outer_padding, 0, 128)
        radius, columns = _clamped(corner_radius, 0, 96), _clamped(columns, 0, 12)
        background = parse_color(background_color, "#000000")
        cell = parse_color(cell_background_color, "#b8b8b8")
        if layout == "aspect_rows":
            rects = aspect_row_rects([picture_aspect(int(f.shape[1]), int(f.shape[0])) for f in frames], width, height)
        else:
            rects = layout_rects(layout, len(frames), columns)
        fit = "cover_crop" if fit_mode == "cover_crop" else "contain_pad"
        panels = [ops.SheetPanel(i, rect, fit, cell, radius) for i, rect in enumerate(panel_rectangles(rects, width, height, padding, gutter))]
        on_device = all(f.is_cuda for f in frames)
        sheet = ops.reference_sheet(frames, panels, (width, height), background).unsqueeze(0)
        return (sheet if on_device else sheet.cpu(),)


NODE_CLASS_MAPPINGS = {"VRGDG_LTXICIngredientsGrid": VRGDG_LTXICIngredientsGrid}
NODE_DISPLAY_NAME_MAPPINGS = {"VRGDG_LTXICIngredientsGrid": "VRGDG LTX IC Ingredients Grid"}

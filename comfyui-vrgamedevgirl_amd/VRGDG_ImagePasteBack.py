"""Image Paste Back (Feathered) on the MI355X: the node of the reference's VRGDG_ImagePasteBack.py with the same names, signatures, widget
specs and messages; the pixels come from csrc/vrg_composite.hip (ops.composite_frames).

What is here: `_batch_item`, `_soft_blend_mask`, `_match_color` and `VRGDG_ImagePasteBack`.  The node's per-frame loop of about twenty eager
ops with a host synchronisation per frame is two small measuring launches and one pass over the output; whether the colour match applies
(at least 16 pixels under the alpha) is decided on the device.  A CPU batch of originals (what ComfyUI hands a node) streams through the host-fed
pipeline of _devices in pieces, a single image is uploaded whole; device tensors are processed where they are.  Inputs are never written.

What is NOT here: `VRGDG_ModernFaceCrop` (cv2 face detection), and the registration in the package's
NODE_CLASS_MAPPINGS: INTEGRATION.md shows the two lines that merge this module's mapping.  The node is eager: it is not part of the deferred
graph fusion of nodes.py.

Refused with a ValueError, because the reference mishandles rather than defines them: a negative x / y in CROP_DATA (the reference falls into
Python's negative slicing) and channel counts other than 3 or 4.
"""
from __future__ import annotations

import torch

from . import ops
from ._devices import compute_device, intermediate_device, stream_frames_with_masks


def _batch_item(tensor, index):
    return tensor[min(index, tensor.shape[0] - 1)]


def _on_compute_device(t, like=None):
    """float32 on the GPU: where `like` lives if that is a GPU, else the compute device"""
    dev = like.device if like is not None and like.is_cuda else compute_device()
    return t.to(device=dev, dtype=torch.float32)


def _soft_blend_mask(height, width, inset, feather, shape, device, dtype):
    """The [height, width] feather mask, evaluated by the composite kernel (an all-zero paste); lives on the GPU whatever `device` says."""
    dev = torch.device(device) if device is not None and torch.device(device).type == "cuda" else compute_device()
    with torch.cuda.device(dev):
        zeros = torch.zeros((1, int(height), int(width), 3), dtype=torch.float32, device=dev)
        crop = torch.zeros((1, 1, 1, 3), dtype=torch.float32, device=dev)
        rule = ops.CompositeRule("ellipse" if shape == "ellipse" else "rectangle", feather=feather, inset=inset)
        entries = ops.paste_back_entries(1, 1, 0, (0, 0, int(width), int(height)))
        return ops.composite_frames(zeros, crop, entries, rule, 0.0)[1][0].to(dtype)


def _match_color(source, target, alpha, strength):
    """`source` shifted towards the mean colour of `target` where alpha > 0.25, measured by the composite's statistics kernel; the decision
    (at least 16 selected pixels) stays on the device.  [h, w, c] tensors and an [h, w, 1] alpha in [0, 1]; device tensors out."""
    if strength <= 0:
        return source
    src = _on_compute_device(source, source)
    with torch.cuda.device(src.device):
        tgt, a = target.to(src.device, torch.float32), alpha.to(src.device, torch.float32)
        h, w = int(src.shape[0]), int(src.shape[1])
        # the alpha travels as the user mask of an all-ones rectangle rule of the same size (both resamplings are the identity there)
        rule = ops.CompositeRule("rectangle", feather=0, inset=0)
        entries = ops.paste_back_entries(1, 1, 1, (0, 0, w, h))
        rec = ops.composite_stats(tgt[None].contiguous(), src[None].contiguous(), entries, rule, strength, user_mask=a[None, ..., 0].contiguous())
        shifted = torch.clamp(src + rec["shift"][0, :src.shape[2]], 0.0, 1.0)
        return torch.where(rec["matched"][0] != 0, shifted, src)


def _crop_corners(crop_data):
    """(x, y, right, bottom) of a WAS-style CROP_DATA pair (size, box); the node's three messages for what is not one."""
    if not crop_data:                                       # False (no face found upstream), None, empty
        raise ValueError("No valid CROP_DATA. Connect Image Crop Face's CROP_DATA output.")
    corners = None
    if isinstance(crop_data, (tuple, list)) and len(crop_data) == 2:
        try:
            corners = tuple(int(value) for value in crop_data[1])
        except (TypeError, ValueError):
            corners = None
    if corners is None or len(corners) != 4:
        raise ValueError("Unsupported CROP_DATA format; connect WAS Image Crop Face directly.")
    if corners[2] <= corners[0] or corners[3] <= corners[1]:
        raise ValueError(f"Invalid crop rectangle in CROP_DATA: {crop_data[1]!r}")
    return corners


class VRGDG_ImagePasteBack:
    """Resize and softly composite an enhanced crop into its original rectangle."""

    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "original_image": ("IMAGE",),
                "enhanced_crop": ("IMAGE",),
                "crop_data": ("CROP_DATA",),
                "inset_padding": ("INT", {"default": 8, "min": 0, "max": 1024, "step": 1}),
                "feather_strength": ("INT", {"default": 24, "min": 0, "max": 1024, "step": 1}),
                "blend_shape": (["ellipse", "rectangle"], {"default": "ellipse"}),
                "color_match": ("FLOAT", {"default": 0.65, "min": 0.0, "max": 1.0, "step": 0.05}),
            },
            "optional": {"mask": ("MASK",)},
        }

    RETURN_TYPES = ("IMAGE", "MASK")
    RETURN_NAMES = ("image", "blend_mask")
    FUNCTION = "paste_back"
    CATEGORY = "VRGameDevGirl/Image"
    DESCRIPTION = (
        "Pastes an enhanced crop back using WAS Image Crop Face CROP_DATA, then "
        "blends the edge with padding and feathering."
    )

    def paste_back(self, original_image, enhanced_crop, crop_data,
                   inset_padding, feather_strength, blend_shape, color_match, mask=None):
        corners = _crop_corners(crop_data)
        rule = ops.CompositeRule("ellipse" if blend_shape == "ellipse" else "rectangle", feather=feather_strength, inset=inset_padding)
        ops.composite_channels(rule, original_image.shape[3], enhanced_crop.shape[3])
        n_originals, n_crops, n_masks = int(original_image.shape[0]), int(enhanced_crop.shape[0]), int(mask.shape[0]) if mask is not None else 0
        entries = ops.paste_back_entries(n_originals, n_crops, n_masks, corners)
        if original_image.is_cuda:
            with torch.cuda.device(original_image.device):
                return ops.composite_frames(original_image.float(), enhanced_crop.to(original_image.device, torch.float32), entries, rule,
                                            color_match, user_mask=None if mask is None else mask.to(original_image.device, torch.float32))
        ops.composite_table(entries, rule, color_match, original_image.shape[1], original_image.shape[2])    # refuses before anything is uploaded
        dev = compute_device()
        with torch.cuda.device(dev):
            crops = enhanced_crop.to(dev, torch.float32)
            user_mask = mask.to(dev, torch.float32) if mask is not None else None
            if len(entries) == n_originals > 1 and intermediate_device().type == "cpu":
                # a batch of originals, one output frame each: they stream through the staging pipeline in pieces, crops and masks wait on the GPU
                def piece(gpu_originals, first_frame):
                    rows = [dict(entry, original=i) for i, entry in enumerate(entries[first_frame:first_frame + int(gpu_originals.shape[0])])]
                    return ops.composite_frames(gpu_originals, crops, rows, rule, color_match, user_mask=user_mask)

                image, blend_mask = stream_frames_with_masks(original_image.float(), piece)
                return (image, blend_mask)
            # a single image, or one original under several crops (more output frames than originals): uploaded whole
            image, blend_mask = ops.composite_frames(original_image.to(dev, torch.float32), crops, entries, rule, color_match, user_mask=user_mask)
        return (image.to(intermediate_device()), blend_mask.to(intermediate_device()))


NODE_CLASS_MAPPINGS = {
    "VRGDG_ImagePasteBack": VRGDG_ImagePasteBack,
}
NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDG_ImagePasteBack": "VRGDG Image Paste Back (Feathered)",
}

"""VRGDG_MultiReferenceConditioning, VRGDG_MultiReferenceConditioningFromPaths and VRGDG_ImageBatchMultiFromPaths of the reference
(VRGDG_GeneralNodes2.py:3801-4145) on the GPU: up to 50 reference pictures of unrelated sizes, each scaled to a megapixel budget, VAE-encoded
and appended to both conditionings as a reference latent; and picture lists joined into one IMAGE batch of the first picture's shape.

The reference resamples picture by picture on the CPU (``F.interpolate``, or a Pillow round trip for lanczos), uploads each result for the
encoder and resizes everything a second time for the IMAGE output.  Here ``ops.scale_reference_images`` scales all pictures of a call in
one launch (csrc/vrg_refbatch.hip) -- CPU pictures go up together, once -- the encoder reads the device tensors, and
``ops.batch_reference_images`` writes the whole batch in one more launch.  The nodes keep the reference's names, ``INPUT_TYPES``, return
types, ``FUNCTION``, ``CATEGORY``, ``DESCRIPTION`` and error texts.

Three seams are module attributes a caller may replace.  ``conditioning_appender``: ComfyUI's
``node_helpers.conditioning_set_values(..., append=True)``, imported when it is first called.  ``image_loader``: the host decode of one file
to RGB bytes (``Image.open``, ``exif_transpose``, ``convert("RGB")``); the bytes go to the device and become fp32 there
(``ops.reference_bytes_to_images``).  ``path_roots``: the directories a relative path is looked up in, ComfyUI's ``folder_paths``.  So this
module imports without ``comfy``, ``node_helpers`` and ``folder_paths``.  It has mappings of its own (register them as INTEGRATION.md shows).
"""
from __future__ import annotations

import json
import os

import numpy as np

from . import ops
from ._devices import intermediate_device

MAX_IMAGES = 50


def conditioning_appender(conditioning, latent):
    """``conditioning`` with the reference latent appended: ``node_helpers.conditioning_set_values``"""
    import node_helpers
    return node_helpers.conditioning_set_values(conditioning, {"reference_latents": [latent["samples"]]}, append=True)


def image_loader(path) -> np.ndarray:
    """the picture file at ``path`` as uint8 ``[height, width, 3]``, upright: the host decode"""
    from PIL import Image, ImageOps
    with Image.open(path) as image:
        return np.asarray(ImageOps.exif_transpose(image).convert("RGB"))


def path_roots() -> list:
    """the directories a relative path is looked up in after the working directory: ComfyUI's input, output and temp directories"""
    import folder_paths
    roots = [folder_paths.get_input_directory(), folder_paths.get_output_directory()]
    temp = getattr(folder_paths, "get_temp_directory", None)
    if callable(temp):
        roots.append(temp())
    return roots


def _unquoted(item) -> str:
    return str(item or "").strip().strip('"').strip("'")


def _parse_image_paths(raw) -> list:
    """The paths of a text box.  Accepted: one path per line; a JSON list of paths, or of objects that name theirs under "path", "file" or
    "image"; a JSON object with a list under "image_paths" or "images", or else its values.  Quotes and blanks around a path are dropped,
    empty entries skipped; text that is not JSON, or JSON of another kind, is read line by line."""
    text = str(raw or "").strip()
    if not text:
        return []
    try:
        parsed = json.loads(text)
    except Exception:
        parsed = None
    if isinstance(parsed, dict):
        listed = next((parsed[k] for k in ("image_paths", "images") if isinstance(parsed.get(k), list)), None)
        entries = listed if listed is not None else list(parsed.values())
    elif isinstance(parsed, list):
        entries = parsed
    else:
        entries = text.replace("\r", "\n").split("\n")
    paths = []
    for entry in entries:
        if isinstance(entry, dict):
            entry = entry.get("path") or entry.get("file") or entry.get("image") or ""
        path = _unquoted(entry)
        if path:
            paths.append(path)
    return paths


def _resolve_image_path(raw_path) -> str:
    """the existing file ``raw_path`` names: absolute as it is; relative in the working directory, then in ``path_roots()``"""
    text = _unquoted(raw_path)
    if not text:
        raise FileNotFoundError("Reference image path was empty.")
    candidates = [text] if os.path.isabs(text) else [text] + [os.path.join(root, text) for root in path_roots()]
    for candidate in candidates:
        full = os.path.normpath(os.path.abspath(candidate))
        if os.path.isfile(full):
            return full
    raise FileNotFoundError(f"Reference image was not found: {text}")


def _load_pictures(paths) -> list:
    """every file decoded on the host, all bytes uploaded together, ``[1, H, W, 3]`` fp32 on the device"""
    return ops.reference_bytes_to_images([image_loader(_resolve_image_path(p)) for p in paths])


def _encode_and_append(positive, negative, vae, pictures, upscale_method, megapixels, resolution_steps):
    scaled = ops.scale_reference_images(pictures, upscale_method, megapixels, resolution_steps)
    for picture in scaled:
        latent = {"samples": vae.encode(picture)}
        positive = conditioning_appender(positive, latent)
        negative = conditioning_appender(negative, latent)
    return positive, negative, scaled


def _scale_widgets(methods):
    return {
        "upscale_method": (list(methods), {"default": "nearest-exact"}),
        "megapixels": ("FLOAT", {"default": 1.0, "min": 0.01, "max": 16.0, "step": 0.01}),
        "resolution_steps": ("INT", {"default": 1, "min": 1, "max": 256, "step": 1}),
    }


class VRGDG_MultiReferenceConditioning:
    upscale_methods = list(ops.REFBATCH_METHODS)
    MAX_IMAGES = MAX_IMAGES

    @classmethod
    def INPUT_TYPES(cls):
        required = {
            "positive": ("CONDITIONING",),
            "negative": ("CONDITIONING",),
            "vae": ("VAE",),
            "image_count": ("INT", {"default": 4, "min": 1, "max": cls.MAX_IMAGES, "step": 1,
                                    "tooltip": "How many image inputs to show and process."}),
        }
        required.update(_scale_widgets(cls.upscale_methods))
        return {"required": required,
                "optional": {f"image{i}": ("IMAGE", {"tooltip": f"Optional reference image {i}."}) for i in range(1, cls.MAX_IMAGES + 1)}}

    RETURN_TYPES = ("CONDITIONING", "CONDITIONING", "IMAGE")
    RETURN_NAMES = ("positive", "negative", "IMAGE")
    FUNCTION = "apply"
    CATEGORY = "VRGDG/Conditioning"
    DESCRIPTION = (
        "Dynamically scales each connected reference image, VAE encodes it, "
        "and appends the resulting reference latent to positive and negative conditioning."
    )

    @staticmethod
    def _batch_for_image_output(images):
        if not images:
            raise ValueError("VRGDG Multi Reference Conditioning needs at least one connected image input.")
        return ops.batch_reference_images(images, "bilinear")

    def apply(self, positive, negative, vae, image_count, upscale_method, megapixels, resolution_steps, **kwargs):
        count = max(1, min(self.MAX_IMAGES, int(image_count)))
        pictures = [kwargs[f"image{i}"] for i in range(1, count + 1) if kwargs.get(f"image{i}") is not None]
        if not pictures:
            return self._batch_for_image_output(pictures)
        positive, negative, scaled = _encode_and_append(positive, negative, vae, pictures, upscale_method, megapixels, resolution_steps)
        return (positive, negative, self._batch_for_image_output(scaled).to(intermediate_device()))


class VRGDG_MultiReferenceConditioningFromPaths:
    upscale_methods = VRGDG_MultiReferenceConditioning.upscale_methods

    @classmethod
    def INPUT_TYPES(cls):
        required = {
            "positive": ("CONDITIONING",),
            "negative": ("CONDITIONING",),
            "vae": ("VAE",),
            "image_paths": ("STRING", {"default": "", "multiline": True,
                                       "tooltip": "Reference image paths from the UI. Use one path per line, or a JSON list of paths."}),
        }
        required.update(_scale_widgets(cls.upscale_methods))
        return {"required": required}

    RETURN_TYPES = ("CONDITIONING", "CONDITIONING", "IMAGE")
    RETURN_NAMES = ("positive", "negative", "IMAGE")
    FUNCTION = "apply"
    CATEGORY = "VRGDG/Conditioning"
    DESCRIPTION = (
        "UI-friendly multi-reference conditioning node. Takes image file paths, "
        "loads and scales each image, VAE encodes it, and appends reference latents."
    )

    _parse_image_paths = staticmethod(_parse_image_paths)
    _resolve_image_path = staticmethod(_resolve_image_path)

    def apply(self, positive, negative, vae, image_paths, upscale_method, megapixels, resolution_steps):
        paths = _parse_image_paths(image_paths)
        if not paths:
            raise ValueError("VRGDG UI Multi Reference Conditioning needs at least one image path.")
        positive, negative, scaled = _encode_and_append(positive, negative, vae, _load_pictures(paths), upscale_method, megapixels,
                                                        resolution_steps)
        return (positive, negative, VRGDG_MultiReferenceConditioning._batch_for_image_output(scaled).to(intermediate_device()))


class VRGDG_ImageBatchMultiFromPaths:
    upscale_methods = VRGDG_MultiReferenceConditioning.upscale_methods

    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "image_paths": ("STRING", {"default": "", "multiline": True,
                                           "tooltip": "Image paths from the UI. Use one path per line, a JSON list of paths, or an object "
                                                      "with image_paths/images."}),
                "upscale_method": (list(cls.upscale_methods), {"default": "bilinear"}),
            },
        }

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("images",)
    FUNCTION = "load_batch"
    CATEGORY = "VRGDG/Image"
    DESCRIPTION = (
        "UI-friendly Image Batch Multi node. Takes image file paths from a text box, "
        "loads each image, and returns one IMAGE batch without requiring dynamic noodle inputs."
    )

    def load_batch(self, image_paths, upscale_method):
        paths = _parse_image_paths(image_paths)
        if not paths:
            raise ValueError("VRGDG UI Image Batch Multi needs at least one image path.")
        return (ops.batch_reference_images(_load_pictures(paths), upscale_method).to(intermediate_device()),)


NODE_CLASS_MAPPINGS = {
    "VRGDG_MultiReferenceConditioning": VRGDG_MultiReferenceConditioning,
    "VRGDG_MultiReferenceConditioningFromPaths": VRGDG_MultiReferenceConditioningFromPaths,
    "VRGDG_ImageBatchMultiFromPaths": VRGDG_ImageBatchMultiFromPaths,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDG_MultiReferenceConditioning": "VRGDG Multi Reference Conditioning",
    "VRGDG_MultiReferenceConditioningFromPaths": "VRGDG UI Multi Reference Conditioning",
    "VRGDG_ImageBatchMultiFromPaths": "VRGDG UI Image Batch Multi",
}

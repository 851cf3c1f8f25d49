"""VRGDG_LTXMSRReferenceBuilder and VRGDG_LTX25MSRReferenceLoader of the reference (vrgdg_ltx_msr_reference_builder.py) on the GPU.

The builder stretches up to four subject stills and a background with cv2's byte Lanczos-4 to ``width`` x ``height`` and repeats them into
a 17 / 25 / 33 / 41-frame batch, returned / 255; the 2.5 loader returns every still on its own as a one-image batch / 255.  Both keep the
reference's names, ``INPUT_TYPES``, return types, ``FUNCTION``, ``CATEGORY`` and error texts, and the module has mappings of its own
(register them as INTEGRATION.md shows).  ``folder_paths`` is ComfyUI's and is imported where it is needed, so the module imports without it.

Files are decoded on the host as the reference decodes them (``Image.open``, ``ImageOps.exif_transpose``, ``convert("RGB")``); the decoded
bytes -- 3 B per pixel, never floats -- go to the device and ``ops.msr_reference_frames`` (csrc/vrg_msr.hip) filters every distinct picture
once and writes it to each of its frames.  The results come back as the reference returns them: CPU fp32 tensors.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _devices, ops

NONE_IMAGE = "(none)"
NEUTRAL_GRAY = 127


def _input_images():
    import folder_paths
    input_dir = folder_paths.get_input_directory()
    files = []
    if os.path.isdir(input_dir):
        files = [f for f in os.listdir(input_dir) if os.path.isfile(os.path.join(input_dir, f))]
        files = folder_paths.filter_files_content_types(files, ["image"])
    return [NONE_IMAGE] + sorted(files)


def _load_image_file(image_name):
    """the decoded [height, width, 3] bytes of one input file, or None for no file"""
    if not image_name or image_name == NONE_IMAGE:
        return None
    import folder_paths
    from PIL import Image, ImageOps
    img = ImageOps.exif_transpose(Image.open(folder_paths.get_annotated_filepath(image_name)))
    return np.array(img.convert("RGB"))


def _to_host(frames: torch.Tensor) -> torch.Tensor:
    """a device result as the CPU tensor the reference returns: into a page-locked buffer where it fits (_devices.PIN_LIMIT_BYTES)"""
    pinned, host = _devices._result_buffer(tuple(frames.shape), frames.dtype, frames.numel() * frames.element_size())
    host.copy_(frames, non_blocking=pinned)
    if pinned:
        torch.cuda.current_stream(frames.device).synchronize()
    return host


def _image_inputs(modes):
    images = _input_images()
    return {
        "subject_1": (images, {"image_upload": True}),
        "subject_2": (images, {"image_upload": True}),
        "subject_3": (images, {"image_upload": True}),
        "subject_4": (images, {"image_upload": True}),
        "background_image": (images, {"image_upload": True}),
        "background_mode": (modes, {"default": "use_uploaded_background"}),
        "width": ("INT", {"default": 736, "min": 32, "max": 8192, "step": 32}),
        "height": ("INT", {"default": 1280, "min": 32, "max": 8192, "step": 32}),
    }


class VRGDG_LTXMSRReferenceBuilder:
    STRENGTHS = ["auto - based on subject count", "17 - light", "25 - balanced", "33 - strong", "41 - strongest"]

    @classmethod
    def INPUT_TYPES(cls):
        required = _image_inputs(["use_uploaded_background", "neutral_placeholder_wip"])
        required["reference_strength"] = (list(cls.STRENGTHS), {"default": "auto - based on subject count"})
        return {"required": required}

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("output",)
    FUNCTION = "build_reference"
    CATEGORY = "VRGDG/LTX MSR"

    def build_reference(self, subject_1, subject_2, subject_3, subject_4, background_image, background_mode, width, height, reference_strength):
        subjects = [p for p in (_load_image_file(name) for name in (subject_1, subject_2, subject_3, subject_4)) if p is not None]
        if not subjects:
            raise ValueError("At least subject_1 must be set to an uploaded image.")
        if background_mode == "neutral_placeholder_wip":
            background = (NEUTRAL_GRAY, NEUTRAL_GRAY, NEUTRAL_GRAY)          # np.full(..., 127, uint8) / 255: float32(127) / float32(255)
        else:
            background = _load_image_file(background_image)
            if background is None:
                raise ValueError("background_image is required unless background_mode is neutral_placeholder_wip.")
        frame_count = self._resolve_frame_count(reference_strength, len(subjects))
        return (_to_host(ops.msr_reference_frames(subjects, (width, height), frame_count, background)),)

    @staticmethod
    def _resolve_frame_count(reference_strength, subject_count):
        for count in (17, 25, 33, 41):
            if str(reference_strength).startswith(str(count)):
                return count
        if subject_count <= 1:
            return 17
        if subject_count == 2:
            return 25
        if subject_count == 3:
            return 33
        return 41


class VRGDG_LTX25MSRReferenceLoader:
    """The stills of the LTX 2.5 guide: every reference is its own one-image batch at its own size (nothing is resized or repeated);
    ``width`` and ``height`` size the neutral placeholder only."""

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": _image_inputs(["use_uploaded_background", "neutral_placeholder_wip", "no_background"])}

    RETURN_TYPES = ("IMAGE", "IMAGE", "IMAGE", "IMAGE", "IMAGE")
    RETURN_NAMES = ("pic1", "pic2", "pic3", "pic4", "background")
    FUNCTION = "load_references"
    CATEGORY = "VRGDG/LTX MSR"
    DESCRIPTION = (
        "Loads up to four subjects and an optional background as separate still "
        "images for ComfyUI-LTX2.5-MSR Multi-Reference Guide."
    )

    def load_references(self, subject_1, subject_2, subject_3, subject_4, background_image, background_mode, width, height):
        subject = _load_image_file(subject_1)
        if subject is None:
            raise ValueError("subject_1 is required for LTX 2.5 MSR.")
        outputs = [_to_host(ops.bytes_to_image(subject))]
        for image_name in (subject_2, subject_3, subject_4):
            image = _load_image_file(image_name)
            outputs.append(_to_host(ops.bytes_to_image(image)) if image is not None else None)
        if background_mode == "neutral_placeholder_wip":
            # the Python double 127 / 255.0 rounded to fp32 -- the same float as the builder's float32(127) / float32(255)
            # (tests/test_msr_host.py::test_the_two_greys)
            background = torch.full((1, int(height), int(width), 3), NEUTRAL_GRAY / 255.0, dtype=torch.float32)
        elif background_mode == "no_background":
            background = None
        else:
            image = _load_image_file(background_image)
            if image is None:
                raise ValueError("background_image is required when background_mode is use_uploaded_background.")
            background = _to_host(ops.bytes_to_image(image))
        return (*outputs, background)


NODE_CLASS_MAPPINGS = {
    "VRGDG_LTXMSRReferenceBuilder": VRGDG_LTXMSRReferenceBuilder,
    "VRGDG_LTX25MSRReferenceLoader": VRGDG_LTX25MSRReferenceLoader,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDG_LTXMSRReferenceBuilder": "VRGDG LTX MSR Reference Builder",
    "VRGDG_LTX25MSRReferenceLoader": "VRGDG LTX 2.5 MSR Reference Loader",
}

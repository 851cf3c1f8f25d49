"""VRGDG_LTXFirstLastGuide of the reference (VRGDG_LTXFirstLastGuide.py) on the GPU: a continuous, low-strength temporal guide from two
user images.

The reference cross-fades the first frame of ``first_image`` into the first frame of ``last_image`` (centre-cropped and bilinearly resized
to the same size) over ``(latent_length - 1) * time_scale + 1`` frames on the CPU, concatenates them and hands the batch to the VAE
encoder.  Here the batch comes from ``ops.flf_guide_frames`` (csrc/vrg_flf.hip): two pictures go to the device, the frames are written in
HBM, next to the encoder that reads them.  The node keeps the reference's name, ``INPUT_TYPES``, return types, ``FUNCTION``, ``CATEGORY``,
``_curve`` and error texts; the latent and its ``noise_mask`` are assembled as the reference assembles them.

``guide_encoder`` is a seam and a module attribute a caller may replace: its default is ComfyUI's ``LTXVAddGuide.encode``, imported when
it is first called, so this module imports without ``comfy``, ``comfy_extras`` and ``folder_paths``.  The module has mappings of its
own (register them as INTEGRATION.md shows).  VRGDG_LTXFirstLastEndpointGuide of the same reference file moves latents only and is not here.
"""
from __future__ import annotations

import torch

from . import ops


def guide_encoder(vae, width, height, guide_video, formula):
    """(pixels, latent) of the guide batch: ``comfy_extras.nodes_lt.LTXVAddGuide.encode``"""
    from comfy_extras.nodes_lt import LTXVAddGuide
    return LTXVAddGuide.encode(vae, width, height, guide_video, formula)


class VRGDG_LTXFirstLastGuide:
    """Build a continuous, low-strength temporal guide from two user images."""

    @classmethod
    def INPUT_TYPES(cls):
        unit = {"min": 0.0, "max": 1.0, "step": 0.01}
        return {
            "required": {
                "positive": ("CONDITIONING",),
                "negative": ("CONDITIONING",),
                "vae": ("VAE",),
                "latent": ("LATENT",),
                "first_image": ("IMAGE",),
                "last_image": ("IMAGE",),
                "guide_strength": ("FLOAT", dict(unit, default=0.35)),
                "transition_start": ("FLOAT", dict(unit, default=0.05, max=0.95)),
                "transition_end": ("FLOAT", dict(unit, default=0.90, min=0.05)),
                "curve": (list(ops.FLF_CURVES), {"default": "smoothstep"}),
            }
        }

    RETURN_TYPES = ("CONDITIONING", "CONDITIONING", "LATENT")
    RETURN_NAMES = ("positive", "negative", "latent")
    FUNCTION = "add_first_last_guide"
    CATEGORY = "VRGDG/video/conditioning"

    _curve = staticmethod(ops.flf_curve)

    def add_first_last_guide(self, positive, negative, vae, latent, first_image, last_image, guide_strength=0.35, transition_start=0.05,
                             transition_end=0.90, curve="smoothstep"):
        samples = latent["samples"]
        latent_length = int(samples.shape[2])
        time_scale = int(vae.downscale_index_formula[0])
        frame_count = max(1, (latent_length - 1) * time_scale + 1)

        guide_video = ops.flf_guide_frames(first_image, last_image, frame_count, transition_start, transition_end, curve)
        # encoded straight into the existing latent timeline: one latent per time step, no keyframe per blended frame
        _, guide_latent = guide_encoder(vae, int(samples.shape[4]), int(samples.shape[3]), guide_video, vae.downscale_index_formula)
        if guide_latent.shape[2] != latent_length:
            raise ValueError(
                f"Temporal guide encoded to {guide_latent.shape[2]} latent frames; "
                f"the destination latent requires {latent_length}."
            )
        if guide_latent.shape[1] != samples.shape[1]:
            raise ValueError(
                f"Temporal guide has {guide_latent.shape[1]} channels; "
                f"the destination latent requires {samples.shape[1]}."
            )

        strength = max(0.0, min(1.0, float(guide_strength)))
        noise_mask = torch.full((samples.shape[0], 1, latent_length, 1, 1), 1.0 - strength, dtype=guide_latent.dtype,
                                device=guide_latent.device)
        output_latent = dict(latent)
        output_latent["samples"] = guide_latent
        output_latent["noise_mask"] = noise_mask
        return positive, negative, output_latent


NODE_CLASS_MAPPINGS = {
    "VRGDG_LTXFirstLastGuide": VRGDG_LTXFirstLastGuide,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDG_LTXFirstLastGuide": "VRGDG LTX First / Last Temporal Guide",
}

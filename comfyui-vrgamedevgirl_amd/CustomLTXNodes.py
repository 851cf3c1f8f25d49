"""VRGDG_LTXSigmaAdvancedGuider of the reference (CustomLTXNodes.py) with its guidance arithmetic on the GPU: one ManualSigmas-driven guider
with scheduled CFG or APG, STG and variance rescale for LTX models.

At every model evaluation of every sampler step the reference combines two or three full latents (positive, negative, perturbed) with some
25 eager torch kernels: the CFG-star projection, CFG or APG (momentum average, per-row norm threshold, a projection through fp64 copies of
whole latents), STG and two global standard deviations.  Here everything between the model evaluations is ONE ``ops.ltx_guidance`` call
(csrc/vrg_guidance.hip): fused launches with fp64 sums, no fp64 copy of a latent, the same bits on every run, no wait on the host.

Kept from the reference: the mapping key and display name, ``INPUT_TYPES``, ``RETURN_TYPES``, ``FUNCTION``, ``CATEGORY``, the error texts; the
host logic of the schedules (``_sigma_tensor``, ``_interpolation_factor``, ``_build_transition_values``, ``_runtime_schedule_offset``,
``_current_transition_index``, ``_schedule_index``); the guider's control flow -- the ``isclose`` gates on cfg, stg and rescale, the reset
of the running average when sigma rises, ``ptb_index`` / ``do_skip`` set in ``try`` / ``finally`` around the perturbed evaluation, the
``sampler_post_cfg_function`` hook dictionary with its keys.

Seams, module attributes a caller may replace, resolved when they are first used, so this module imports without ComfyUI:
``comfy_samplers()`` (``comfy.samplers``: ``CFGGuider``, ``calc_cond_batch``) and ``ltx_stg_module()`` (the ``stg`` module of
ComfyUI-LTXVideo: ``STGFlag``, ``STGGuider``, ``STGBlockWrapper``).  The three model evaluations stay calls of ``calc_cond_batch``.

The module has mappings of its own (register them as INTEGRATION.md shows).  Not here: VRGDG_LTXCFGSchedule and
VRGDG_LTXScheduledCFGGuider (they hand the arithmetic to ComfyUI's own ``sampling_function``) and VRGDG_LTXSigmaGuideRelease (it scales a
slice of a denoise mask and guide attention entries): no device arithmetic of their own to move.
"""
from __future__ import annotations

import importlib
import math

import torch

from . import ops


def comfy_samplers():
    """``comfy.samplers``, imported when the first guider is built"""
    import comfy.samplers
    return comfy.samplers


def ltx_stg_module():
    """The ``stg`` module of an installed ComfyUI-LTXVideo, looked for next to this package and under ``custom_nodes``"""
    package = __package__ or ""
    names = [f"{package.rsplit('.', 1)[0]}.ComfyUI-LTXVideo.stg"] if "." in package else []
    names += ["custom_nodes.ComfyUI-LTXVideo.stg", "ComfyUI-LTXVideo.stg"]
    failures = []
    for name in names:
        try:
            return importlib.import_module(name)
        except ImportError as error:            # (ModuleNotFoundError is one)
            failures.append(str(error))
    raise ImportError("VRGDG LTX Sigma Advanced Guider requires ComfyUI-LTXVideo. " + " | ".join(failures))


# ---- schedules: host logic, no device --------------------------------------------------------------------------------------------------------

def _sigma_tensor(sigmas) -> torch.Tensor:
    flat = torch.as_tensor(sigmas).detach().flatten().to(device="cpu", dtype=torch.float64)
    if flat.numel() < 2:
        raise ValueError("sigmas must contain at least two values")
    if not torch.isfinite(flat).all():
        raise ValueError("every sigma value must be finite")
    return flat


def _interpolation_factor(interpolation: str, amount: float) -> float:
    if interpolation == "linear":
        return amount
    if interpolation == "ease_in":
        return amount * amount
    if interpolation == "ease_out":
        return amount * (2.0 - amount)
    raise ValueError(f"Unsupported interpolation: {interpolation}")


def _build_transition_values(sigmas, value_start, value_end, interpolation, start_percent, end_percent, *, outside_value):
    """(sigmas as fp64, one value per sigma transition).  Inside the window [start_percent, end_percent] of the transitions the value ramps
    from ``value_start`` to ``value_end`` (rounded to 4 places); outside it is ``outside_value``, or with ``None`` the start value before
    and the end value after."""
    flat = _sigma_tensor(sigmas)
    if start_percent > end_percent:
        raise ValueError("start_percent must be less than or equal to end_percent")
    count = int(flat.numel()) - 1
    first = min(int(count * start_percent), count - 1)
    last = min(int(count * end_percent), count - 1)
    if outside_value is None:
        values = [float(value_start) if i <= last else float(value_end) for i in range(count)]
    else:
        values = [float(outside_value)] * count
    for i in range(first, last + 1):
        amount = (i - first) / (last - first) if last != first else 0.0
        values[i] = round(float(value_start + _interpolation_factor(interpolation, amount) * (value_end - value_start)), 4)
    return flat, tuple(values)


def _runtime_schedule_offset(expected_sigmas, runtime_sigmas) -> int:
    """Where the sampler's sigma range lies in the connected ManualSigmas (LTX's easy samplers split them into contiguous ranges)"""
    expected, runtime = _sigma_tensor(expected_sigmas), _sigma_tensor(runtime_sigmas)
    n = int(runtime.numel())
    for offset in range(int(expected.numel()) - n + 1):
        if torch.allclose(runtime, expected[offset:offset + n], rtol=1e-5, atol=1e-7):
            return offset
    raise ValueError("The sampler's sigma range is not part of the connected ManualSigmas. "
                     "Connect the same SIGMAS output to this node and the sampler.")


def _current_transition_index(sample_sigmas, timestep) -> int:
    """The transition a model evaluation at ``timestep`` belongs to: the one that starts at that sigma; else the first whose interval holds
    it (samplers evaluate between two sigmas); else the nearest start.  Compared on the CPU in fp64, wherever the timestep lives."""
    sigmas = _sigma_tensor(sample_sigmas)
    current = torch.as_tensor(timestep).detach().flatten()[0].to(device="cpu", dtype=torch.float64)
    starts = sigmas[:-1]
    exact = torch.isclose(starts, current, rtol=1e-5, atol=1e-7).nonzero()
    if exact.numel() > 0:
        return int(exact.flatten()[0].item())
    for i in range(int(sigmas.numel()) - 1):
        a, b = sigmas[i], sigmas[i + 1]
        if torch.minimum(a, b) <= current <= torch.maximum(a, b):
            return i
    return int(torch.argmin(torch.abs(starts - current)).item())


def _schedule_index(expected_sigmas, runtime_sigmas, timestep) -> int:
    return _runtime_schedule_offset(expected_sigmas, runtime_sigmas) + _current_transition_index(runtime_sigmas, timestep)


# ---- the guider ------------------------------------------------------------------------------------------------------------------------------

class _SigmaAdvancedGuidance:
    """The guider without its base: ``guider_class()`` puts it in front of the seam's ``CFGGuider``."""

    def __init__(self, model, sigmas, cfg_values, stg_values, rescale_values, stg_blocks, guidance_mode, cfg_star, apg_eta, apg_norm_threshold,
                 apg_momentum):
        stg = ltx_stg_module()
        model = model.clone()
        super().__init__(model)
        self.sigma_schedule = tuple(float(v) for v in _sigma_tensor(sigmas))
        self.cfg_values = tuple(float(v) for v in cfg_values)
        self.stg_values = tuple(float(v) for v in stg_values)
        self.rescale_values = tuple(float(v) for v in rescale_values)
        self.guidance_mode = guidance_mode
        self.cfg_star = bool(cfg_star)
        self.apg_eta = float(apg_eta)
        self.apg_norm_threshold = float(apg_norm_threshold)
        self.apg_momentum = float(apg_momentum)
        self.apg_running_average = None
        self.previous_sigma = None
        self.stg_flag = stg.STGFlag(do_skip=False, skip_layers=list(stg_blocks))
        blocks = stg.STGGuider.get_transformer_blocks(model)
        invalid_blocks = [index for index in stg_blocks if index < 0 or index >= len(blocks)]
        if invalid_blocks:
            raise ValueError(f"stg_blocks contains invalid indices {invalid_blocks}; this LTX model "
                             f"has {len(blocks)} transformer blocks")
        for index, block in enumerate(blocks):
            model.set_model_patch_replace(stg.STGBlockWrapper(block, self.stg_flag, index), "dit", "double_block", index)

    def set_conds(self, positive, negative):
        self.inner_set_conds({"positive": positive, "negative": negative})

    def _average_for(self, sigma):
        """The running average an APG step at ``sigma`` continues: forgotten when sigma rises (a new sampling run)"""
        sigma_value = float(torch.as_tensor(sigma).detach().flatten()[0])
        if self.previous_sigma is not None and sigma_value > self.previous_sigma + 1e-7:
            self.apg_running_average = None
        self.previous_sigma = sigma_value
        return self.apg_running_average

    def predict_noise(self, x, timestep, model_options=None, seed=None):
        if model_options is None:
            model_options = {}
        transformer_options = model_options.setdefault("transformer_options", {})
        runtime_sigmas = transformer_options.get("sample_sigmas")
        if runtime_sigmas is None:
            raise ValueError("LTX Sigma Advanced Guider could not find the sampler sigma schedule")
        index = _schedule_index(self.sigma_schedule, runtime_sigmas, timestep)
        cfg, stg_scale, rescale = self.cfg_values[index], self.stg_values[index], self.rescale_values[index]
        positive_cond, negative_cond = self.conds.get("positive"), self.conds.get("negative")
        evaluate = comfy_samplers().calc_cond_batch

        positive = evaluate(self.inner_model, [positive_cond], x, timestep, model_options)[0]
        negative = None
        if not math.isclose(cfg, 1.0):
            negative = evaluate(self.inner_model, [negative_cond], x, timestep, model_options)[0]
        apg = negative is not None and self.guidance_mode == "APG"
        average = self._average_for(timestep) if apg else None

        perturbed = None
        if not math.isclose(stg_scale, 0.0):
            try:
                transformer_options["ptb_index"] = 0
                self.stg_flag.do_skip = True
                perturbed = evaluate(self.inner_model, [positive_cond], x, timestep, model_options)[0]
            finally:
                self.stg_flag.do_skip = False
                transformer_options.pop("ptb_index", None)

        result = ops.ltx_guidance(positive, negative, perturbed, cfg=cfg, stg_scale=stg_scale, rescale=rescale, cfg_star=self.cfg_star,
                                  mode="APG" if apg else "CFG", eta=self.apg_eta, norm_threshold=self.apg_norm_threshold,
                                  momentum=self.apg_momentum, average=average, want_negative=self.cfg_star)
        if result.average is not None:
            self.apg_running_average = result.average
        guided = result.guided

        uncond_for_hook = result.negative if result.negative is not None else negative if negative is not None else positive
        perturbed_for_hook = perturbed if perturbed is not None else positive
        for function in model_options.get("sampler_post_cfg_function", []):
            guided = function({"denoised": guided, "cond": positive_cond, "uncond": negative_cond, "model": self.inner_model,
                               "uncond_denoised": uncond_for_hook, "cond_denoised": positive, "sigma": timestep,
                               "model_options": model_options, "input": x, "perturbed_cond": positive_cond,
                               "perturbed_cond_denoised": perturbed_for_hook})
        return guided


_GUIDER_CLASSES = {}


def guider_class():
    """``_LTXSigmaAdvancedGuider``: the guidance above as a subclass of the seam's ``CFGGuider`` (one class per base)"""
    base = comfy_samplers().CFGGuider
    if base not in _GUIDER_CLASSES:
        _GUIDER_CLASSES[base] = type("_LTXSigmaAdvancedGuider", (_SigmaAdvancedGuidance, base),
                                     {"__doc__": "ManualSigmas-driven CFG/APG + STG guider for current LTX models."})
    return _GUIDER_CLASSES[base]


class VRGDGLTXSigmaAdvancedGuider:
    @classmethod
    def INPUT_TYPES(cls):
        def number(default, low, high, step=0.01):
            return ("FLOAT", {"default": default, "min": low, "max": high, "step": step})
        return {
            "required": {
                "model": ("MODEL",),
                "positive": ("CONDITIONING",),
                "negative": ("CONDITIONING",),
                "sigmas": ("SIGMAS", {"tooltip": "Connect the same ManualSigmas used by the sampler."}),
                "cfg_start": number(4.0, 0.0, 100.0),
                "cfg_end": number(4.0, 0.0, 100.0),
                "stg_start": number(1.0, 0.0, 20.0),
                "stg_end": number(1.0, 0.0, 20.0),
                "rescale_start": number(0.7, 0.0, 1.0),
                "rescale_end": number(0.7, 0.0, 1.0),
                "interpolation": (["linear", "ease_in", "ease_out"],),
                "start_percent": number(0.0, 0.0, 1.0),
                "end_percent": number(1.0, 0.0, 1.0),
                "stg_blocks": ("STRING", {"default": "14, 19", "tooltip": "Comma-separated LTX transformer blocks to perturb."}),
                "guidance_mode": (["CFG", "APG"],),
                "cfg_star": ("BOOLEAN", {"default": False}),
                "apg_eta": number(1.0, -10.0, 10.0),
                "apg_norm_threshold": number(5.0, 0.0, 50.0, 0.1),
                "apg_momentum": number(0.0, -5.0, 1.0),
            }
        }

    RETURN_TYPES = ("GUIDER",)
    RETURN_NAMES = ("guider",)
    FUNCTION = "get_guider"
    CATEGORY = "VRGameDevGirl/LTX/Sampling"
    DESCRIPTION = ("One ManualSigmas-driven LTX guider with scheduled CFG/APG, STG, and "
                   "variance rescale. APG replaces the CFG vector when selected; it is not "
                   "stacked as a second guidance pass. Outside the active percentage range "
                   "CFG is 1 and STG/rescale are 0.")

    def get_guider(self, model, positive, negative, sigmas, cfg_start, cfg_end, stg_start, stg_end, rescale_start, rescale_end, interpolation,
                   start_percent, end_percent, stg_blocks, guidance_mode, cfg_star, apg_eta, apg_norm_threshold, apg_momentum):
        window = (interpolation, start_percent, end_percent)
        sigma_tensor, cfg_values = _build_transition_values(sigmas, cfg_start, cfg_end, *window, outside_value=1.0)
        _, stg_values = _build_transition_values(sigmas, stg_start, stg_end, *window, outside_value=0.0)
        _, rescale_values = _build_transition_values(sigmas, rescale_start, rescale_end, *window, outside_value=0.0)
        try:
            block_indices = [int(part.strip()) for part in stg_blocks.split(",") if part.strip()]
        except ValueError as error:
            raise ValueError("stg_blocks must be comma-separated integers") from error
        if not block_indices and any(not math.isclose(value, 0.0) for value in stg_values):
            raise ValueError("At least one stg_blocks index is required when STG is active")
        guider = guider_class()(model, sigma_tensor, cfg_values, stg_values, rescale_values, block_indices, guidance_mode, cfg_star, apg_eta,
                                apg_norm_threshold, apg_momentum)
        guider.set_conds(positive, negative)
        guider.raw_conds = (positive, negative)
        return (guider,)


NODE_CLASS_MAPPINGS = {
    "VRGDG_LTXSigmaAdvancedGuider": VRGDGLTXSigmaAdvancedGuider,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDG_LTXSigmaAdvancedGuider": "VRGDG LTX Sigma Advanced Guider",
}

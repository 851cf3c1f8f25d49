"""Per-batch effect helpers of the stand-alone video enhancer
(VRGDG_StandaloneVideoEnhancerNodes.py:233-308 of the reference): unsharp, then per-frame-seeded grain.
Per-frame seeding makes the result independent of batch boundaries and of how frames are sharded across GPUs
(the property the reference tests at tests/test_standalone_video_enhancer.py:39-61).  The loop's upscale
(``_resize_frames``: cv2's INTER_LANCZOS4 on the decoded bytes) runs on the GPU as well, fused into the effects
(``_enhance_decoded``), so that a 4K job uploads its source-size frames.  Job control, segment files and the ffmpeg mux
around these helpers are out of scope."""
from __future__ import annotations

import torch

from . import ops
from ._devices import resident


class DecodedFrames:
    """What this module's ``_frames_to_tensor`` hands to the render loop (reference :417-421:
    ``tensor = _frames_to_tensor(frames); enhanced, n = _process_with_retry(tensor, settings, i); _tensor_to_frames(enhanced)``):
    the decoded batch as ONE uint8 B,G,R tensor on the GPU, with the ``/ 255`` conversion DEFERRED.  ``_apply_effects_batch`` runs
    the whole loop body on it as one uint8 -> uint8 kernel (ops.sharpen_then_seeded_grain: 3 + 3 B/px instead of the 54 B/px of
    converter, fp32 effects, converter) and ``_tensor_to_frames`` only downloads the bytes; the results are byte-identical to the
    reference's fp32 route.  Anything else that wants the reference's fp32 tensor calls ``float_tensor()``."""

    def __init__(self, frames_u8: torch.Tensor):
        self.u8 = frames_u8

    def __len__(self):
        return int(self.u8.shape[0])

    def __getitem__(self, index):
        if not isinstance(index, slice):
            raise TypeError("DecodedFrames supports batch slices only")
        return DecodedFrames(self.u8[index])

    @property
    def shape(self):
        return self.u8.shape

    @property
    def is_cuda(self):
        return self.u8.is_cuda

    def float_tensor(self) -> torch.Tensor:
        """fp32 R,G,B [F,H,W,3] in [0,1]: ``np.stack(rgb).astype(float32) / 255.0`` (reference :311-316), on the GPU."""
        return ops.frames_u8_to_f32(self.u8)

    @staticmethod
    def cat(parts):
        return DecodedFrames(torch.cat([p.u8 for p in parts], dim=0))


def _apply_unsharp(images, strength, use_gpu):
    if strength <= 0:
        return images
    return ops.stencil3x3(images, "unsharp", strength, zero_border=bool(use_gpu))


def _apply_seeded_grain(images, intensity, saturation_mix, seed, frame_start):
    if intensity <= 0:
        return images
    return ops.film_grain_seeded_frames(images, intensity, saturation_mix, seed, frame_start)


def _apply_effects_batch(images, settings, frame_start=0):
    """sharpen (optional) then seeded grain (optional).  A CPU tensor comes back as a CPU tensor like in the
    reference; a GPU tensor (what this module's _frames_to_tensor produces) stays on the GPU so that the enhancer loop
    decode -> _frames_to_tensor -> _process_with_retry -> _tensor_to_frames crosses PCIe once each way, in uint8."""
    use_gpu_flag = bool(settings.get("use_gpu", True))
    if isinstance(images, DecodedFrames):
        # decoded uint8 frames: the conversions and both effects in one pass (or the converter route for what that kernel refuses)
        sharpen_on, grain_on = bool(settings.get("sharpen_enabled", True)), bool(settings.get("grain_enabled", False))
        out = ops.sharpen_then_seeded_grain(images.u8, float(settings.get("sharpen_strength", 0.5)) if sharpen_on else 0.0, use_gpu_flag,
                                            float(settings.get("grain_intensity", 0.04)) if grain_on else 0.0,
                                            float(settings.get("saturation_mix", 0.5)), int(settings.get("seed", 42)), int(frame_start))
        return DecodedFrames(out)
    batch = resident(images).to(torch.float32)
    sharpen, grain = bool(settings.get("sharpen_enabled", True)), bool(settings.get("grain_enabled", False))
    strength, intensity = float(settings.get("sharpen_strength", 0.5)), float(settings.get("grain_intensity", 0.04))
    if sharpen and grain and strength > 0 and intensity > 0:
        # both effects: one pass over the frames (the same bits as the two helpers below, one after the other)
        batch = ops.sharpen_then_seeded_grain(batch, strength, use_gpu_flag, intensity, float(settings.get("saturation_mix", 0.5)),
                                              int(settings.get("seed", 42)), int(frame_start))
    else:
        if sharpen:
            batch = _apply_unsharp(batch, strength, use_gpu_flag)
        if grain:
            batch = _apply_seeded_grain(batch, intensity, float(settings.get("saturation_mix", 0.5)), int(settings.get("seed", 42)),
                                        int(frame_start))
    return batch.detach() if images.is_cuda else batch.detach().cpu()


def _process_with_retry(images, settings, frame_start):
    """Halve the batch on device OOM (same contract as the reference: returns (frames, smallest batch used))."""
    try:
        return _apply_effects_batch(images, settings, frame_start), len(images)
    except RuntimeError as exc:
        if "out of memory" not in str(exc).lower() or len(images) <= 1:
            raise
        torch.cuda.empty_cache()
        mid = max(1, len(images) // 2)
        left, ls = _process_with_retry(images[:mid], settings, frame_start)
        right, rs = _process_with_retry(images[mid:], settings, frame_start + mid)
        if isinstance(left, DecodedFrames):
            return DecodedFrames.cat((left, right)), min(ls, rs)
        return torch.cat((left, right), dim=0), min(ls, rs)


_LONG_EDGE = {"2k": 2560, "3k": 3072, "4k": 3840}
_BATCH_BY_PIXELS = ((1280 * 720, 16), (1920 * 1080, 8), (2560 * 1440, 4), (3200 * 1800, 2))

# Which route _enhance_decoded takes when both are possible: the fused kernel (one launch, the upscaled frames stay in LDS) or the two
# launches (vrg_lanczos4_u8, then vrg_sharpen_grain_u8).  With grain on, the fused kernel draws each normal with a Philox call of its own
# where the two-launch route shares one call among four elements; profiles/lanczos.json has both timed, DESIGN.md section 3 the reasons.
FUSED_UPSCALE_WITH_GRAIN = False
FUSED_UPSCALE_WITHOUT_GRAIN = True


def _output_dimensions(width, height, upscale_resolution):
    """(width, height) of the rendered video: the long edge goes to 2560 / 3072 / 3840 for "2k" / "3k" / "4k" when the source is
    smaller, both sides rounded to even numbers; anything else, or a source already that large, keeps its size."""
    w, h = max(int(width), 1), max(int(height), 1)
    target = _LONG_EDGE.get(str(upscale_resolution or "original").strip().lower())
    long_edge = max(w, h)
    if target is None or long_edge >= target:
        return w, h
    factor = target / long_edge
    even = lambda v: max(2 * int(round(v * factor / 2.0)), 2)      # noqa: E731
    return even(w), even(h)


def _auto_batch_size(width, height):
    """Frames per batch when the settings leave it open: 16 up to 720p, halved per size class, 1 above 3200 x 1800."""
    pixels = max(int(width) * int(height), 1)
    for limit, batch in _BATCH_BY_PIXELS:
        if pixels <= limit:
            return batch
    return 1


def _resize_frames(frames, output_width, output_height):
    """``cv2.resize(frame, (w, h), interpolation=cv2.INTER_LANCZOS4)`` per frame on the GPU (ops.resize_frames_u8).  A list of BGR arrays
    comes back as a list of BGR arrays, a ``DecodedFrames`` as a ``DecodedFrames``; frames that already have the size are handed back
    as they are (the same objects), like in the reference."""
    w, h = max(int(output_width), 1), max(int(output_height), 1)
    if isinstance(frames, DecodedFrames):
        out = ops.resize_frames_u8(frames.u8, w, h)
        return frames if out is frames.u8 else DecodedFrames(out)
    frames = list(frames)
    todo = [i for i, f in enumerate(frames) if not (f.shape[1] == w and f.shape[0] == h)]
    if not todo:
        return frames
    from .VRGDG_LUTVideoTools import _stack_frames, _unstack_frames
    result = list(frames)
    by_shape = {}
    for i in todo:
        by_shape.setdefault(tuple(frames[i].shape), []).append(i)
    for indices in by_shape.values():
        resized = _unstack_frames(ops.resize_frames_u8(_stack_frames([frames[i] for i in indices]), w, h))
        for i, r in zip(indices, resized):
            result[i] = r
    return result


def _upscale_effects(frames_u8, output_width, output_height, settings, frame_start):
    sharpen_on, grain_on = bool(settings.get("sharpen_enabled", True)), bool(settings.get("grain_enabled", False))
    strength = float(settings.get("sharpen_strength", 0.5)) if sharpen_on else 0.0
    intensity = float(settings.get("grain_intensity", 0.04)) if grain_on else 0.0
    args = (strength, bool(settings.get("use_gpu", True)), intensity, float(settings.get("saturation_mix", 0.5)), int(settings.get("seed", 42)),
            int(frame_start))
    fused = FUSED_UPSCALE_WITH_GRAIN if intensity > 0 else FUSED_UPSCALE_WITHOUT_GRAIN
    if fused:
        return ops.upscale_sharpen_then_seeded_grain(frames_u8, output_width, output_height, *args)
    return ops.sharpen_then_seeded_grain(ops.resize_frames_u8(frames_u8, output_width, output_height), *args)


def _enhance_decoded(frames, output_width, output_height, settings, frame_start=0):
    """The render loop's ``frames = _resize_frames(frames, w, h); tensor = _frames_to_tensor(frames); enhanced, n = _process_with_retry(
    tensor, settings, i)`` (reference :415-417) on decoded frames -- a list of BGR arrays or a ``DecodedFrames``: the SOURCE-size bytes are
    uploaded, upscale and effects run on the GPU, the result is a ``DecodedFrames`` of the output size for ``_tensor_to_frames``.  On
    device OOM the batch is halved like in ``_process_with_retry`` (``.smallest_batch`` of the result is the smallest batch used)."""
    w, h = max(int(output_width), 1), max(int(output_height), 1)
    decoded = frames if isinstance(frames, DecodedFrames) else _frames_to_tensor(frames)

    def run(part, start):
        try:
            return DecodedFrames(_upscale_effects(part.u8, w, h, settings, start)), len(part)
        except RuntimeError as exc:
            if "out of memory" not in str(exc).lower() or len(part) <= 1:
                raise
            torch.cuda.empty_cache()
            mid = max(1, len(part) // 2)
            left, ls = run(part[:mid], start)
            right, rs = run(part[mid:], start + mid)
            return DecodedFrames.cat((left, right)), min(ls, rs)

    result, smallest = run(decoded, int(frame_start))
    result.smallest_batch = smallest
    return result


def _frames_to_tensor(frames):
    """BGR uint8 frames -> the batch on the GPU, 3 B/px over PCIe, as ``DecodedFrames`` (the ``/ 255`` of reference :311-316 happens
    inside the effects kernel; ``.float_tensor()`` is the reference's fp32 tensor)."""
    from .VRGDG_LUTVideoTools import _stack_frames
    return DecodedFrames(_stack_frames(frames))


def _tensor_to_frames(tensor):
    """fp32 RGB (or the DecodedFrames ``_apply_effects_batch`` returned) -> list of BGR uint8 frames (:319-324 of the reference)."""
    if isinstance(tensor, DecodedFrames):
        from .VRGDG_LUTVideoTools import _unstack_frames
        return _unstack_frames(tensor.u8)
    from .VRGDG_LUTVideoTools import _tensor_to_frames as impl
    return impl(tensor)

"""Stream-order probes: does every launch of a public call go to the CALLER's current stream?

The arithmetic of every operator is pinned elsewhere.  Here the expected value is the same call run once on the default stream and
synchronised -- a reference for ORDERING only.  The probe then repeats the call under a side stream so that a launch on any other stream
gives other bits, deterministically (`probe`):

  * a spin sits on the default stream; a launch that went there by accident runs behind it and the caller's stream reads an output
    nobody wrote (the output is poisoned first);
  * a spin sits on the caller's stream in front of the copy that makes the inputs valid; a launch that went anywhere else runs during
    that spin and reads the input poison (finite, inside the operators' domain: 0.25 for floats, 64 for bytes).

The caller's stream is one of torch's pool that was seen to run BESIDE the default stream (Spin.overlap): the runtime maps its streams
onto a few hardware queues, and two streams on one queue run in queue order whatever their own order says.
Whether a spin was still running when the call returned ("armed") is read from events, not from a clock.  A call that uploads its
records with the synchronous `_hip.upload_records` waits for the caller's stream on the host: it can only be armed against the
default stream and is listed in HOST_SYNCING with the line that waits.

The table CASES and the dict EXCLUDED are read without a GPU by tests/test_stream_table_host.py.
"""
import time
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

POISON_IN = {True: 0.25, False: 64}          # by is_floating_point: stale input
POISON_OUT = {True: 0.75, False: 192}        # an output nobody wrote
MARGIN = 4.0                                 # the caller-side spin outlasts the host side of the call this many times
FLOOR_SECONDS = 0.005                        # ... and the handful of torch calls the probe itself makes around it
TOTAL_SPIN_SECONDS = 0.5                     # both spins of one test together, at the most


@dataclass
class Case:
    name: str
    build: Callable                 # build(ops, dev) -> (inputs: list of device tensors, call(inputs, out) -> tensor | tuple of tensors)
    covers: tuple                   # the functions that hand the stream to the library on this call's path (bare: of ops.py; else module.name)
    out: bool = False               # the call takes out=: the probe passes a poisoned one
    reset: Optional[Callable] = None        # reset(ops): forget cached tables, so that the call is a FIRST use (uploads under the caller's stream)


def _rand(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def _bytes(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def _cube(n, seed):
    return {"size": n, "lut": _rand((n, n, n, 3), seed), "domain_min": torch.zeros(3), "domain_max": torch.ones(3)}


POINT = (2, 37, 344, 3)             # the smallest frame the fused sharpen + grain kernel takes, two frames, odd height
ADJUST_ALL = {"temperature": -12.5, "tint": 8, "saturation": 14, "exposure": -9, "contrast": 11, "highlights": -22, "shadows": 17, "whites": 6,
              "blacks": -4, "sharpen": 33, "clarity": 21, "vignette": 28, "fade": 9}


# ---- pointwise and fused ----------------------------------------------------------------------------------------------------------------------

def _film_grain(ops, dev):
    def call(inp, out):
        torch.manual_seed(5)
        return ops.film_grain(inp[0], 0.04, 0.5, chunk_frames=1, out=out)
    return [_rand(POINT, 1).to(dev)], call


def _film_grain_oversize(ops, dev):
    """The route of an RNG chunk that torch itself splits (above rng.MAX_CHUNK_NUMEL = 2^29 elements: 2 GB a frame batch) at the small
    shape: the limit is lowered for the call, so the chunk is cut into four leaves that are not frame aligned -- the leaf-by-leaf noise
    launches and the injected-noise grain run as they do for a real oversize chunk (their bits are then not torch.randn's; the expected
    value here is the same call on the default stream)."""
    from comfyui_vrgamedevgirl_amd import rng

    def call(inp, out):
        limit = rng.MAX_CHUNK_NUMEL
        rng.MAX_CHUNK_NUMEL = 20000
        try:
            torch.manual_seed(6)
            return ops.film_grain(inp[0], 0.04, 0.5, chunk_frames=0)
        finally:
            rng.MAX_CHUNK_NUMEL = limit
    return [_rand(POINT, 3).to(dev)], call


def _seeded(ops, dev):
    return [_rand(POINT, 2).to(dev)], lambda inp, out: ops.film_grain_seeded_frames(inp[0], 0.05, 0.4, 1234, 17)


def _injected(ops, dev):
    g = torch.Generator().manual_seed(4)
    return [_rand(POINT, 3).to(dev), torch.randn(POINT, generator=g).to(dev)], lambda inp, out: ops.film_grain_injected(inp[0], inp[1], 0.04, 0.5)


def _lut3d(n):
    def build(ops, dev):
        lut = ops.upload_lut(_cube(n, 10 + n), dev)
        return [_rand(POINT, 5).to(dev)], lambda inp, out: ops.lut3d(inp[0], lut, 6.5, out=out)
    return build


def _lut3d_fresh(ops, dev):
    cube = _cube(17, 27)
    return [_rand(POINT, 5).to(dev)], lambda inp, out: ops.lut3d(inp[0], ops.upload_lut(cube, dev), 10.0)


def _lut_ffmpeg(ops, dev):
    lut = ops.upload_lut(_cube(17, 28), dev)
    return [_bytes(POINT, 6).to(dev)], lambda inp, out: ops.lut3d_ffmpeg_u8(inp[0], lut)


def _stencil(zero):
    def build(ops, dev):
        return [_rand(POINT, 7).to(dev)], lambda inp, out: ops.stencil3x3(inp[0], "unsharp", 0.6, zero, out=out)
    return build


def _sharpen_grain(u8):
    def build(ops, dev):
        x = _bytes(POINT, 8) if u8 else _rand(POINT, 8)
        return [x.to(dev)], lambda inp, out: ops.sharpen_then_seeded_grain(inp[0], 0.6, False, 0.05, 0.4, 1234, 17)
    return build


def _adjust(u8):
    def build(ops, dev):
        from comfyui_vrgamedevgirl_amd import VRGDG_LUTVideoTools as LVT
        terms = ops.adjust_terms(LVT._normalize_adjust_settings(ADJUST_ALL))
        x = _bytes(POINT, 9) if u8 else _rand(POINT, 9, -0.1, 1.1)
        return [x.to(dev)], lambda inp, out: ops.adjust(inp[0], terms, out=out)
    return build


def _u8_to_f32(ops, dev):
    return [_bytes(POINT, 11).to(dev)], lambda inp, out: ops.frames_u8_to_f32(inp[0])


def _f32_to_u8(ops, dev):
    return [_rand(POINT, 12, -0.1, 1.1).to(dev)], lambda inp, out: ops.f32_to_frames_u8(inp[0])


def _chain(variant, colormatch):
    def build(ops, dev):
        lut = ops.upload_lut(_cube(17, 29), dev)
        ref_ms = ops.reference_stats(_rand((1, 64, 80, 3), 13).to(dev)) if colormatch else None
        torch.cuda.synchronize()
        spec = ops.ChainSpec(grain=(0.04, 0.5, 2), lut=(lut, 10.0), colormatch=(ref_ms, 0.9) if colormatch else None,
                             sharpen=("unsharp", 0.5, False), variant=variant)

        def call(inp, out):
            torch.manual_seed(7)
            return ops.fused_chain(inp[0], spec, out=out)
        return [_rand(POINT, 14).to(dev)], call
    return build


# ---- colour match -----------------------------------------------------------------------------------------------------------------------------

CM, CM_REF = (3, 45, 51, 3), (1, 64, 80, 3)


def _lab_stats(ops, dev):
    return [_rand(CM, 20).to(dev)], lambda inp, out: ops.finalize_stats(ops.lab_stats(inp[0]))


def _lab_stats_device(ops, dev):
    return [_rand(CM, 21, -30.0, 70.0).to(dev)], lambda inp, out: ops.lab_stats_device(inp[0], 2)


def _chain_stats(ops, dev):
    lut = ops.upload_lut(_cube(17, 30), dev)

    def call(inp, out):
        torch.manual_seed(8)
        lab = torch.empty_like(inp[0])
        return ops.chain_stats(inp[0], ops.ChainSpec(grain=(0.06, 0.3, 2), lut=(lut, 10.0)), lab_out=lab), lab
    return [_rand(CM, 22).to(dev)], call


def _reference_stats(ops, dev):
    return [_rand(CM_REF, 23).to(dev)], lambda inp, out: ops.reference_stats(inp[0])


def _apply(ops, dev):
    x = _rand(CM, 24).to(dev)
    ims = ops.finalize_stats(ops.lab_stats(x))
    rms = ops.finalize_stats(ops.lab_stats(_rand(CM_REF, 25).to(dev)))
    torch.cuda.synchronize()
    return [x, ims, rms], lambda inp, out: ops.colormatch_apply(inp[0], inp[1], inp[2], 0.6)


def _color_match(stats):
    def build(ops, dev):
        return [_rand(CM, 26).to(dev), _rand(CM_REF, 27).to(dev)], lambda inp, out: ops.color_match(inp[0], inp[1], 0.8, cm_stats=stats, cache_lab=False)
    return build


def _color_match_async(ops, dev):
    def call(inp, out):
        ref_ms, event = ops.reference_stats_async(inp[1])            # on the pack's side stream, ordered after the caller's
        return ops.color_match(inp[0], None, 0.8, ref_ms=ref_ms, ref_event=event), ref_ms
    return [_rand(CM, 28).to(dev), _rand(CM_REF, 29).to(dev)], call


def _stats_selfcheck(ops, dev):
    return [], lambda inp, out: torch.tensor([ops.device_stats_selfcheck(dev, force=True)], device=dev)


# ---- resamplers with cached tables ------------------------------------------------------------------------------------------------------------

def _forget_tables(ops):
    ops._lanczos_tables.clear()
    ops._area_tables.clear()
    ops._grid_tables.clear()
    ops._warp_tables.clear()


def _lanczos(ops, dev):
    return [_bytes((2, 54, 96, 3), 30).to(dev)], lambda inp, out: ops.resize_frames_u8(inp[0], 192, 108)


def _upscale(ops, dev):
    return [_bytes((2, 54, 96, 3), 31).to(dev)], lambda inp, out: ops.upscale_sharpen_then_seeded_grain(inp[0], 192, 108, 0.6, True, 0.05, 0.35, 42, 5)


def _cut(ops, dev):
    def call(inp, out):
        thumbs = ops.cut_thumbnails(inp[0], out=out)
        hist = ops.cut_histograms(thumbs)
        return thumbs, hist, ops.cut_pair_sums(thumbs, hist)
    return [_rand((3, 70, 90, 3), 32, -0.1, 1.1).to(dev)], call


def _warp_affine(ops, dev):
    t = np.array([[1.04, -0.1, 3.3], [0.1, 1.04, -2.7]], dtype=np.float32)
    return [_bytes((3, 40, 56, 3), 33).to(dev)], lambda inp, out: ops.warp_affine_u8(inp[0], [t, None, t], 48, 36)


def _grid(ops, dev):
    return ([_rand((2, 40, 64, 3), 34).to(dev), _rand((1, 33, 47, 4), 35).to(dev), _rand((2, 16, 24, 3), 36).to(dev)],
            lambda inp, out: ops.video_grid(list(inp), 32, 24, 2))


def _grid_bytes(ops, dev):
    index = [[0, 1, 1], [-1, 0, 0]]
    return [_bytes((2, 40, 64, 3), 37).to(dev), _bytes((1, 33, 47, 3), 38).to(dev)], lambda inp, out: ops.video_grid_bytes(list(inp), index, 32, 24, 2)


def _msr(ops, dev):
    return ([_bytes((37, 53, 3), 39).to(dev), _bytes((64, 48, 3), 40).to(dev)],
            lambda inp, out: ops.msr_reference_frames(list(inp), (64, 96), 5, background=(127, 127, 127)))


# ---- record-driven calls ----------------------------------------------------------------------------------------------------------------------

STRETCH, LETTERBOX, BICUBIC = "Stretch to dimensions", "Fit with letterbox (preserve all)", "Bicubic (recommended)"


def _resize(ops, dev):
    g = ops.resize_geometry(45, 51, 64, 40, LETTERBOX)
    return [_rand((2, 45, 51, 4), 50).to(dev)], lambda inp, out: ops.resize_geometry_frames(inp[0], g, BICUBIC)


def _prepare(ops, dev):
    g = ops.resize_geometry(45, 51, 64, 40, STRETCH)
    return [_rand((3, 45, 51, 3), 51).to(dev)], lambda inp, out: ops.prepare_frames(inp[0], g, BICUBIC, [2, 0, 2])


def _restore(ops, dev):
    return ([_rand((2, 34, 60, 3), 52).to(dev), _rand((3, 81, 145, 4), 53).to(dev)],
            lambda inp, out: ops.restore_frames(inp[0], inp[1], 145, 81, LETTERBOX, BICUBIC, 0.7, out=out))


def _crop(ops, dev):
    entries = [{"box": (10, 8, 60, 50)}, {"box": None}, {"box": (0, 0, 90, 70)}]

    def call(inp, out):
        return ops.crop_frames(inp[0], ops.crop_sequence_plan(entries, 3, 70, 90), size=(64, 48))
    return [_rand((3, 70, 90, 3), 54).to(dev)], call


def _composite_rows():
    return [{"original": i, "crop": i, "box": (10 + i, 8, 90 + i, 80), "strength": 0.9} for i in range(3)]


def _composite(ops, dev):
    rule = ops.CompositeRule("radial", feather=7)

    def call(inp, out):
        rec = ops.composite_stats(inp[0], inp[1], _composite_rows(), rule, 0.65)
        image, mask = ops.composite_frames(inp[0], inp[1], _composite_rows(), rule, 0.65)
        return image, mask, rec["count"], rec["shift"]
    return [_rand((3, 90, 120, 3), 55).to(dev), _rand((3, 32, 32, 3), 56).to(dev)], call


def _aligned(ops, dev):
    ident = np.array([[1, 0, 0.5], [0, 1, 0]], dtype=np.float32)
    return ([_rand((3, 90, 120, 3), 57).to(dev), _rand((3, 32, 32, 3), 58).to(dev)],
            lambda inp, out: ops.aligned_composite_frames(inp[0], inp[1], _composite_rows(), 5, [None, ident, None]))


def _face_bytes(ops, dev):
    def call(inp, out):
        faces = ops.face_bytes(inp[1], _composite_rows(), 90, 120, originals=inp[0])
        thumbs, _index = ops.face_thumbs(faces)
        return faces.generated, faces.source, thumbs
    return [_rand((3, 90, 120, 3), 59).to(dev), _rand((3, 32, 32, 3), 60).to(dev)], call


def _detect(ops, dev):
    rows = [(0, -1, 0, 0, 64, 48), (1, 0, 8, 4, 40, 44)]
    inv = [[0.98, 0.17, -3.0, -0.17, 0.98, 5.0]]

    def call(inp, out):
        return ops.detect_blobs(inp[0], rows, inv), ops.warp_linear_bytes(inp[0], [(0, 0), (1, -1)], inv)
    return [_rand((2, 48, 64, 3), 61).to(dev)], call


def _sheet(ops, dev):
    panels = [ops.SheetPanel(0, (0, 0, 53, 37)), ops.SheetPanel(1, (60, 4, 30, 40))]

    def call(inp, out):
        return (ops.reference_sheet(list(inp), panels, (96, 48), (9, 9, 9)), ops.reference_sheet(list(inp), panels, (96, 48), (9, 9, 9), out_bytes=True))
    return [_rand((37, 53, 3), 62).to(dev), _rand((64, 40, 3), 63).to(dev)], call


def _flf(ops, dev):
    return [_rand((1, 40, 56, 3), 64).to(dev), _rand((1, 50, 90, 3), 65).to(dev)], lambda inp, out: ops.flf_guide_frames(inp[0], inp[1], 9)


def _refbatch(ops, dev):
    def call(inp, out):
        scaled = ops.scale_reference_images(list(inp), "bicubic", 0.002, 4)
        return (*scaled, ops.batch_reference_images(list(inp), "bilinear"), ops.batch_reference_images(list(inp), "lanczos"))
    return [_rand((1, 33, 29, 3), 66).to(dev), _rand((1, 20, 37, 3), 67).to(dev)], call


def _refbatch_bytes(ops, dev):
    return [_bytes((16, 16, 3), 68).to(dev), _bytes((7, 5, 3), 69).to(dev)], lambda inp, out: tuple(ops.reference_bytes_to_images(list(inp)))


def _assemble(ops, dev):
    plan = [(0, 0), (0, 2), (1, 0), (0, 1)]

    def call(inp, out):
        data, clean = ops.assemble_labelled_bytes(list(inp), plan, clean_out=True)
        return ops.assemble_frames(list(inp), plan), data, clean
    return [_rand((3, 16, 24, 3), 70).to(dev), _rand((1, 16, 24, 3), 71).to(dev)], call


def _anchor_load(ops, dev):
    return [_bytes((37, 53, 3), 72).to(dev), _bytes((64, 40, 3), 73).to(dev)], lambda inp, out: ops.anchor_frames(list(inp))


def _anchor_store(ops, dev):
    return [_rand((2, 37, 53, 3), 74, -0.1, 1.1).to(dev)], lambda inp, out: ops.anchor_store_bytes(inp[0], bgr=True, out=out)


# ---- calls of the node modules that ops has no entry for ----------------------------------------------------------------------------------------

FF_BOXES = [(10, 8, 74, 72), None, (0, 0, 120, 90)]          # (left, top, right, bottom) per frame of 120 x 90
FF_STRENGTHS = [0.9, 1.0, 0.8]


def _ff_crop(ops, dev):
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix as FF
    return [_bytes((3, 90, 120, 3), 80).to(dev)], lambda inp, out: FF.crop_frames(inp[0], FF_BOXES, 64)


def _ff_composite(ops, dev):
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix as FF
    return ([_bytes((3, 90, 120, 3), 81).to(dev), _bytes((2, 64, 64, 3), 82).to(dev)],
            lambda inp, out: FF.composite_frames(inp[0], inp[1], FF_BOXES, FF_STRENGTHS, 12, 0.5))


def _ff_packed(ops, dev):
    """frames on the host: only the boxes cross the bus, in and out (no device input to poison: the outputs and the flags are probed)"""
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix as FF
    originals, enhanced = _bytes((3, 90, 120, 3), 83), _bytes((2, 64, 64, 3), 84)

    def call(inp, out):
        crops = FF.crop_frames_packed(originals, FF_BOXES, 64)
        boxes = FF.composite_boxes_packed(originals, enhanced, FF_BOXES, FF_STRENGTHS, 12, 0.5)
        return crops, torch.from_numpy(np.concatenate([b.reshape(-1) for b in boxes]))
    return [], call


def _far_resize(ops, dev):
    from comfyui_vrgamedevgirl_amd import far_face_repair as FR
    return [_bytes((37, 53, 3), 85).to(dev), _bytes((5, 9, 3), 86).to(dev)], lambda inp, out: FR.pil_lanczos_resize(list(inp), (40, 30))


def _far_composite(ops, dev):
    from comfyui_vrgamedevgirl_amd import far_face_repair as FR
    masks = [_bytes((33, 29), 89).numpy(), _bytes((20, 20), 90).numpy()]

    def call(inp, out):
        fresh = FR.composite_frames(inp[0], [inp[1], inp[2]], FF_BOXES, 6, True)                  # fresh soft ellipses, colour match
        saved = FR.composite_frames(inp[0], [inp[1], inp[2]], FF_BOXES, -1, True, masks)          # the saved masks, resized
        return fresh, saved
    return [_bytes((3, 90, 120, 3), 87).to(dev), _bytes((48, 40, 3), 88).to(dev), _bytes((100, 130, 3), 91).to(dev)], call


def _contact_sheet(ops, dev):
    from comfyui_vrgamedevgirl_amd import far_face_repair as FR
    return ([_bytes((48, 64, 3), 92).to(dev), _bytes((48, 64, 3), 93).to(dev), _bytes((40, 70, 3), 94).to(dev)],
            lambda inp, out: FR.contact_sheet([inp[0], inp[1]], [inp[2], None], 24, 2, 60))


def _channel_sums(ops, dev):
    from comfyui_vrgamedevgirl_amd import VRGDG_WorkflowRunnerNodes as WR
    return [_bytes(POINT, 95).to(dev)], lambda inp, out: WR._channel_sums(inp[0])


CASES = [
    Case("film_grain", _film_grain, ("_grain_call",), out=True),
    Case("film_grain_oversize", _film_grain_oversize, ("_film_grain_oversize",)),
    Case("film_grain_seeded_frames", _seeded, ("_grain_call",)),
    Case("film_grain_injected", _injected, ("film_grain_injected",)),
    Case("lut3d_17", _lut3d(17), ("lut3d",), out=True),
    Case("lut3d_33", _lut3d(33), ("lut3d",), out=True),
    Case("lut3d_fresh_upload", _lut3d_fresh, ("upload_lut", "lut3d")),
    Case("lut3d_ffmpeg_u8", _lut_ffmpeg, ("lut3d_ffmpeg_u8",)),
    Case("stencil3x3_replicate", _stencil(False), ("stencil3x3",), out=True),
    Case("stencil3x3_zero", _stencil(True), ("stencil3x3",), out=True),
    Case("sharpen_then_seeded_grain_f32", _sharpen_grain(False), ("sharpen_then_seeded_grain",)),
    Case("sharpen_then_seeded_grain_u8", _sharpen_grain(True), ("_sharpen_then_seeded_grain_u8",)),
    Case("adjust_f32", _adjust(False), ("adjust",), out=True),
    Case("adjust_u8", _adjust(True), ("adjust",), out=True),
    Case("frames_u8_to_f32", _u8_to_f32, ("frames_u8_to_f32",)),
    Case("f32_to_frames_u8", _f32_to_u8, ("f32_to_frames_u8",)),
    *[Case(f"fused_chain_v{v}{'_cm' if cm else ''}", _chain(v, cm), ("fused_chain",) + (("lab_stats_device",) if cm else ()), out=True)
      for v in (0, 1, 2) for cm in (False, True)],
    Case("lab_stats_finalize", _lab_stats, ("lab_stats", "finalize_stats")),
    Case("lab_stats_device", _lab_stats_device, ("lab_stats_device",)),
    Case("chain_stats", _chain_stats, ("chain_stats",)),
    Case("reference_stats", _reference_stats, ("reference_stats", "lab_stats_device")),
    Case("colormatch_apply", _apply, ("colormatch_apply",)),
    Case("color_match_device", _color_match("device"), ("fused_chain", "reference_stats", "lab_stats_device")),
    Case("color_match_fp64", _color_match("fp64"), ("lab_stats", "finalize_stats", "colormatch_apply")),
    Case("color_match_async_reference", _color_match_async, ("reference_stats", "fused_chain")),
    Case("device_stats_selfcheck", _stats_selfcheck, ("device_stats_selfcheck",)),
    Case("resize_frames_u8", _lanczos, ("resize_frames_u8",)),
    Case("resize_frames_u8[first]", _lanczos, ("resize_frames_u8",), reset=_forget_tables),
    Case("upscale_sharpen_then_seeded_grain", _upscale, ("upscale_sharpen_then_seeded_grain",)),
    Case("upscale_sharpen_then_seeded_grain[first]", _upscale, ("upscale_sharpen_then_seeded_grain",), reset=_forget_tables),
    Case("cut_score", _cut, ("cut_thumbnails", "cut_histograms", "cut_pair_sums"), out=True),
    Case("cut_score[first]", _cut, ("cut_thumbnails", "cut_histograms", "cut_pair_sums"), reset=_forget_tables),
    Case("warp_affine_u8", _warp_affine, ("warp_affine_u8",)),
    Case("warp_affine_u8[first]", _warp_affine, ("warp_affine_u8",), reset=_forget_tables),
    Case("video_grid", _grid, ("_grid_launch",)),
    Case("video_grid[first]", _grid, ("_grid_launch",), reset=_forget_tables),
    Case("video_grid_bytes", _grid_bytes, ("_grid_launch",)),
    Case("msr_reference_frames", _msr, ("msr_reference_frames",)),
    Case("resize_geometry_frames", _resize, ("resize_geometry_frames",)),
    Case("prepare_frames", _prepare, ("prepare_frames",)),
    Case("restore_frames", _restore, ("restore_frames",), out=True),
    Case("crop_frames", _crop, ("crop_resize",)),
    Case("composite_stats_and_frames", _composite, ("_composite_measure", "composite_frames")),
    Case("aligned_composite_frames", _aligned, ("aligned_composite_frames", "face_bytes")),
    Case("face_bytes_and_thumbs", _face_bytes, ("face_bytes", "_face_thumbs")),
    Case("detect_blobs_and_warp", _detect, ("detect_blobs", "warp_linear_bytes")),
    Case("reference_sheet", _sheet, ("reference_sheet",)),
    Case("flf_guide_frames", _flf, ("flf_guide_frames",)),
    Case("reference_images", _refbatch, ("_refbatch_launch",)),
    Case("reference_bytes_to_images", _refbatch_bytes, ("_refbatch_launch",)),
    Case("assemble", _assemble, ("assemble_frames", "assemble_labelled_bytes")),
    Case("anchor_frames", _anchor_load, ("anchor_frames",)),
    Case("anchor_store_bytes", _anchor_store, ("anchor_store_bytes",), out=True),
    Case("facefix_builder_crop", _ff_crop, ("VRGDG_FaceFix.crop_frames",)),
    Case("facefix_builder_composite", _ff_composite, ("VRGDG_FaceFix._run_masks", "VRGDG_FaceFix.CompositePlan.run_resize_stats",
                                                      "VRGDG_FaceFix.CompositePlan.run_composite")),
    Case("facefix_builder_packed", _ff_packed, ("VRGDG_FaceFix.crop_frames_packed", "VRGDG_FaceFix.composite_boxes_packed", "VRGDG_FaceFix._run_masks")),
    Case("far_face_resize", _far_resize, ("far_face_repair.ResizePlan.run",)),
    Case("far_face_composite", _far_composite, ("far_face_repair.ResizePlan.run", "far_face_repair.MaskPlan.run", "far_face_repair.CompositePlan.run_means",
                                                "far_face_repair.CompositePlan.run_paste")),
    Case("contact_sheet", _contact_sheet, ("far_face_repair.ThumbPlan.run_rows", "far_face_repair.ThumbPlan.run_compose")),
    Case("u8_channel_sums", _channel_sums, ("VRGDG_WorkflowRunnerNodes._channel_sums",)),
]

#: the modules whose functions and methods hand _hip.current_stream() to the library; names of `ops` stand bare in `covers`, the others as
#: module.function or module.Class.method
STREAM_MODULES = ("ops", "VRGDG_FaceFix", "far_face_repair", "VRGDG_WorkflowRunnerNodes")

#: calls that wait for the caller's stream on the host, and where: they are armed against the default stream only
HOST_SYNCING = {
    "lut3d_fresh_upload": "ops.py upload_lut: lut_data['lut'].to(device) is a synchronous upload",
    "device_stats_selfcheck": "ops.py device_stats_selfcheck: torch.equal(got, want) reads a flag on the host",
    "resize_frames_u8[first]": "ops.py _uploaded: _hip.upload_records(build(), device) on a cache miss",
    "upscale_sharpen_then_seeded_grain[first]": "ops.py _uploaded: _hip.upload_records(build(), device) on a cache miss",
    "cut_score[first]": "ops.py _uploaded: _hip.upload_records(build(), device) on a cache miss",
    "warp_affine_u8": "ops.py warp_affine_u8: rec = _hip.upload_records(table, x.device, F)",
    "warp_affine_u8[first]": "ops.py _uploaded: _hip.upload_records(build(), device) on a cache miss, then warp_affine_u8's records",
    "video_grid": "ops.py _grid_launch: dev_desc = _hip.upload_records(desc, out.device)",
    "video_grid[first]": "ops.py _uploaded: _hip.upload_records(build(), device) on a cache miss, then _grid_launch's records",
    "video_grid_bytes": "ops.py _grid_launch: dev_desc = _hip.upload_records(desc, out.device)",
    "msr_reference_frames": "ops.py msr_reference_frames: d = _hip.upload_records(desc, dev)",
    "prepare_frames": "ops.py prepare_frames: torch.tensor(listed, dtype=torch.int32).to(x.device)",
    "crop_frames": "ops.py crop_resize: dev_table = _hip.upload_records(table, source.device)",
    "composite_stats_and_frames": "ops.py _composite_prepare: dev_table = _hip.upload_records(table, o.device, ...)",
    "aligned_composite_frames": "ops.py _composite_prepare / face_bytes / aligned_composite_frames: _hip.upload_records",
    "face_bytes_and_thumbs": "ops.py face_bytes: dev_table = _hip.upload_records(...); _face_thumbs: upload_records(..., out=records)",
    "detect_blobs_and_warp": "ops.py detect_blobs / warp_linear_bytes: torch.from_numpy(t.copy()).to(dev) and launch(): _hip.upload_records",
    "reference_sheet": "ops.py reference_sheet: d = _hip.upload_records(part, dev) / (rec, dev)",
    "flf_guide_frames": "ops.py flf_guide_frames: wd = torch.from_numpy(weights).to(dev)",
    "reference_images": "ops.py _refbatch_launch: table = _hip.upload_records(desc, dev)",
    "reference_bytes_to_images": "ops.py _refbatch_launch: table = _hip.upload_records(desc, dev)",
    "assemble": "ops.py _assemble_prepare: table = _hip.upload_records(rows, dev)",
    "anchor_frames": "ops.py anchor_frames: table = _hip.upload_records(desc, dev, trailing=(tables,))",
    "facefix_builder_crop": "VRGDG_FaceFix.py crop_frames: taps, dev_desc = _upload(table, x.device), _upload(desc, x.device)",
    "facefix_builder_composite": "VRGDG_FaceFix.py CompositePlan.__init__: self.taps, self.desc = _upload(...); _run_masks: _upload(spans, device)",
    "facefix_builder_packed": "VRGDG_FaceFix.py crop_frames_packed / composite_boxes_packed: _upload(...), _packed.py upload_with_prefix(...) and download(out), which waits for the stream",
    "far_face_resize": "far_face_repair.py ResizePlan.__init__: self.tables = _upload(...), self.desc = _upload(desc, device)",
    "far_face_composite": "far_face_repair.py CompositePlan / ResizePlan / MaskPlan: _upload(...) of their records",
    "contact_sheet": "far_face_repair.py ThumbPlan.__init__: _upload(...) of the entries and tables",
}

#: functions of ops.py that hand _hip.current_stream() to the library and are NOT probed; only calls without a caller-produced device input
EXCLUDED = {
    "torch_stream_noise": "test / debug entry: fills a fresh tensor from a host descriptor, no device input",
    "toolchain_selfcheck": "probes the compiler's output on tensors it makes itself and reads them back; no device input",
}
MAY_BE_EXCLUDED = {"torch_stream_noise", "toolchain_selfcheck"}      # with the HipEvent methods and the debug-library probes (not module-level functions of ops.py)


def covered() -> set:
    return {name for case in CASES for name in case.covers}


# ---- the probe ----------------------------------------------------------------------------------------------------------------------------------

def flat(result):
    if isinstance(result, torch.Tensor):
        return [result]
    return [t for t in result if t is not None]


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit for bit (so NaN by position and payload, -0.0 apart from 0.0), compared on the device"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return bool(torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)))


class Spin:
    """torch.cuda._sleep cycles per second, from the slope of two spins timed by events"""

    def __init__(self):
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        c1, c2 = 1_000_000, 5_000_000
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        torch.cuda._sleep(c1)
        e[1].record()
        torch.cuda._sleep(c2)
        e[2].record()
        torch.cuda.synchronize()
        self.ms = (e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]))
        self.cycles = (c1, c2)
        slope = (self.ms[1] - self.ms[0]) / (c2 - c1)                 # ms per cycle
        assert slope > 0, f"torch.cuda._sleep does not spin: {self.ms} ms for {self.cycles} cycles"
        self.hz = 1000.0 / slope

    def __str__(self):
        return f"_sleep: {self.cycles[0]} cycles {self.ms[0]:.3f} ms, {self.cycles[1]} cycles {self.ms[1]:.3f} ms -> {self.hz / 1e6:.1f} MHz"

    def queue(self, seconds: float):
        torch.cuda._sleep(int(seconds * self.hz))

    def overlap(self, a, b, seconds=0.003) -> bool:
        """Do spins on streams `a` and `b` run side by side?  The runtime spreads its streams over a few hardware queues (4 by default); two
        streams on one queue run one after the other whatever their order says, which hides every ordering mistake between them and keeps a
        call that waits for its own stream on the host behind the other stream's spin.  Timed on the GPU by events: both spins start
        behind a gate (a short spin on the default stream), so the host's own pace while it queues them does not count."""
        default = torch.cuda.default_stream()
        best = float("inf")
        for _ in range(2):
            torch.cuda.synchronize()
            gate, end_a, end_b = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            self.queue(0.002)
            gate.record(default)
            for stream, end in ((a, end_a), (b, end_b)):
                stream.wait_event(gate)
                with torch.cuda.stream(stream):
                    self.queue(seconds)
                    end.record(stream)
            torch.cuda.synchronize()
            best = min(best, max(gate.elapsed_time(end_a), gate.elapsed_time(end_b)) / 1e3)
        return best < 1.6 * seconds

    def streams(self, n: int) -> list:
        """`n` new streams that overlap the default stream and one another (see overlap)"""
        chosen, default = [], torch.cuda.default_stream()
        for _ in range(32):                      # torch hands out its pool of 32 streams in turn
            s = torch.cuda.Stream()
            if all(self.overlap(s, other) for other in [default] + chosen):
                chosen.append(s)
                if len(chosen) == n:
                    return chosen
        raise AssertionError(f"COULD NOT ARM, nothing about the package was tested: only {len(chosen)} of the {n} streams wanted were seen to run "
                             "beside the default stream and one another (32 streams of torch's pool tried; is the GPU shared or "
                             "GPU_MAX_HW_QUEUES below 2?)")

    @property
    def side(self):
        if getattr(self, "_side", None) is None:
            self._side = self.streams(1)[0]
        return self._side


def _poison(t: torch.Tensor, table) -> torch.Tensor:
    return torch.full_like(t, table[t.is_floating_point()])


def probe(ops, case: Case, inputs, call, spin: Spin) -> dict:
    """Steps 1-5 of the module docstring.  Returns the flags and figures; asserts nothing."""
    dev = torch.device("cuda", torch.cuda.current_device())
    assert torch.cuda.current_stream() == torch.cuda.default_stream()

    def run(inp, out):
        if case.reset is not None:
            case.reset(ops)
        return flat(call(inp, out))

    # 1. the expected bits: the same call on the default stream (once to warm caches and self-checks, once timed on the host)
    run(inputs, None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = run(inputs, None)
    host_seconds = time.perf_counter() - t0
    torch.cuda.synchronize()
    assert all(w.data_ptr() != x.data_ptr() for w in want for x in inputs), "the call hands an input back: nothing to probe"
    # 2. poisoned inputs, a poisoned out
    x2 = [_poison(x, POISON_IN) for x in inputs]
    out = _poison(want[0], POISON_OUT) if case.out else None
    early_seconds = min(max(MARGIN * host_seconds, FLOOR_SECONDS), TOTAL_SPIN_SECONDS / 3.0)
    late_seconds = 2.0 * early_seconds           # a call that waits for its own stream on the host still returns under it
    early, late = torch.cuda.Event(), torch.cuda.Event()
    side = spin.side                             # a stream of torch's pool that runs beside the default stream (Spin.overlap)
    with torch.cuda.stream(side):                # a dry run fills this stream's pool of the allocator: no hipMalloc while the spins run
        dry = run(inputs, None)
    side.synchronize()
    del dry
    torch.cuda.synchronize()
    # 3. the default stream is busy: a launch that went there leaves the caller an unwritten output.  The caller's spin is queued FIRST:
    # where the runtime puts both streams on one hardware queue the spins run one after the other, and a call that waits for its own
    # stream on the host must still return under the default stream's spin
    with torch.cuda.stream(side):
        spin.queue(early_seconds)
    spin.queue(late_seconds)
    late.record()
    # 4. the caller's stream: (spin,) inputs made valid, the call
    with torch.cuda.stream(side):
        for a, b in zip(x2, inputs):
            a.copy_(b)
        if out is None:
            for w in want:                # fill and free blocks of the outputs' sizes in this stream's pool: a fresh output starts as poison
                junk = _poison(w, POISON_OUT)
                del junk
        early.record()
        got = run(x2, out)
        armed_early, armed_late = not early.query(), not late.query()
        seen = [g.clone() for g in got]
    # 5.
    side.synchronize()
    torch.cuda.synchronize()
    return {"host_ms": host_seconds * 1e3, "early_ms": early_seconds * 1e3, "late_ms": late_seconds * 1e3,
            "armed_early": armed_early, "armed_late": armed_late,
            "outputs": len(want) == len(seen) and [same_bits(s, w) for s, w in zip(seen, want)],
            "inputs_kept": [same_bits(a, b) for a, b in zip(x2, inputs)]}

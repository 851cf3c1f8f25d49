"""Pass 2 of the headline chain keeps the NaN patches of its clamps behind a scalar branch on a wave-wide ballot (clamp01_3<true>,
csrc/vrg_pixel_math.hpp): a wave whose pixels are all finite skips them, a wave that sees one NaN runs them; pass 1 takes the same decision
with selects.  These tests steer it both ways -- per wave of pass 1 (k_produce_lab<3,false,false>: the grain clamp) and per row step of pass 2
(k_apply_march<COLORMATCH|FROM_LAB>: the Lab -> RGB clip and the unsharp clamp) -- and hold the fused headline chain (device statistics,
cm_chunk 1), bit for bit and NaN position for NaN position, to

  * the stand-alone operator sequence film_grain -> lut3d -> color_match -> stencil3x3 (kernels this change does not touch), every case, both
    arithmetic policies;
  * oracle/chain_oracle.headline_chain (the check bench.verify_output makes), every case whose FRAMES hold no NaN: the restated LUT indexes
    with the pixel value and raises on a NaN (the kernels use cell 0 there: a NaN pixel takes pass 1's patched side at the grain clamp and
    leaves the cube finite), so a NaN frame has no oracle to be held to; pass 2's patched side is steered by the NaN reference.  +Inf, 1e35 and
    denormals leave grain's clamp as 1 / 1 / ~0 and go through it; a NaN in the REFERENCE frame only reaches the statistics and goes through too.

Frames: 4 x 66 x 130 (two strips x three segments of pass 2, 25,740 elements per frame > PR_RUN + 3: the shared-Philox pass 1, GENERAL = false)
and 4 x 48 x 64 (the GENERAL form of pass 2, which keeps the flattened selects)."""
import pytest
import torch

from oracle import restated as R

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SHAPES = {"strips": (4, 66, 130), "general": (4, 48, 64)}


def _poke(x, kind):
    """the issue's frame cases; x: [4, H, W, 3] uniform frames (modified in place)"""
    F, H, W, _ = x.shape
    if kind == "finite":
        pass
    elif kind == "specials":                         # one NaN, one +Inf, one 1e35, one denormal in otherwise finite frames
        x[0, H // 2, W // 3, 1] = NAN
        x[1, 5, 7, 0] = INF
        x[2, H - 2, W - 3, 2] = 1e35
        x[3, 11, 13, 1] = 1e-40
    elif kind == "specials_no_nan":                  # the same without the NaN: the oracle can follow
        x[1, 5, 7, 0] = INF
        x[2, H - 2, W - 3, 2] = 1e35
        x[3, 11, 13, 1] = 1e-40
    elif kind == "halo_priming":                     # a strip's halo columns (x = 61 / 62) on a segment's priming rows (y = 59 / 60)
        x[1, min(59, H - 1), min(61, W - 1), 0] = NAN
        x[2, min(60, H - 1), min(62, W - 1), 2] = NAN
    elif kind == "first_pixel":                      # the chunk's first pixel: the one idle lanes of pass 1 re-read
        x[0, 0, 0, 1] = NAN
    elif kind == "run_end":                          # the last sub-range of a Philox run and the two elements past it
        flat = x.view(-1)
        for e in (PR_RUN - 700, PR_RUN - 1, PR_RUN, PR_RUN + 1, flat.numel() - 2):
            flat[e] = NAN
    elif kind == "constant":                         # a frame whose Lab std is 0
        x[2] = 0.37
    else:
        raise ValueError(kind)
    return x


PR_RUN = 768 * 8       # elements per sibling run of a pass-1 workgroup: 8 sub-ranges of 768 (csrc/vrg_produce_body.hpp)


FRAME_KINDS = ["finite", "specials", "specials_no_nan", "halo_priming", "first_pixel", "run_end", "constant"]
ORACLE_KINDS = {"finite", "specials_no_nan", "constant"}


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def lut(ops, dev):
    import os
    from comfyui_vrgamedevgirl_amd import VRGDG_IV_Adjustments as iv
    data = R.parse_cube_file(os.path.join(iv.LUTS_DIR, "AMD_TealOrange_33.cube"))
    return data, ops.upload_lut(data, dev)


def _same(a, b):
    a, b = a.cpu(), b.cpu()
    return bool((torch.isnan(a) == torch.isnan(b)).all()) and bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def _inputs(shape, kind, ref_nan, dev):
    F, H, W = SHAPES[shape]
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = _poke(torch.rand((F, H, W, 3), generator=g), kind)
    ref = torch.rand((1, H, W, 3), generator=g)
    if ref_nan:
        ref[0, H // 3, W // 2, 2] = NAN
    return x.to(dev), ref.to(dev)


@pytest.mark.parametrize("ref_nan", [False, True])
@pytest.mark.parametrize("kind", FRAME_KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("math", ["device", "fast"])
def test_headline_chain_equals_the_operator_sequence(ops, dev, lut, math, shape, kind, ref_nan):
    _, dlut = lut
    x, ref = _inputs(shape, kind, ref_nan, dev)
    ref_ms = ops.reference_stats(ref, cm_math=math)
    spec = ops.ChainSpec(grain=(0.04, 0.5, 4), lut=(dlut, 10.0), colormatch=(ref_ms, 1.0), sharpen=("unsharp", 0.5, False), cm_math=math, cm_chunk=1)
    fused = ops.fused_chain(x, spec, generator=torch.Generator(device=dev).manual_seed(5))
    y = ops.film_grain(x, 0.04, 0.5, chunk_frames=4, generator=torch.Generator(device=dev).manual_seed(5))
    y = ops.lut3d(y, dlut, 10.0)
    y = ops.color_match(y, ref, 1.0, ref_ms=ref_ms, cm_math=math, cm_chunk=1)
    y = ops.stencil3x3(y, "unsharp", 0.5, False)
    assert _same(fused, y), (math, shape, kind, ref_nan, int((fused.cpu().view(torch.int32) != y.cpu().view(torch.int32)).sum()))
    if kind == "finite" and not ref_nan:
        assert not bool(torch.isnan(fused).any())
    if ref_nan:                                        # NaN reference statistics: every row step of pass 2 takes the patched side
        assert bool(torch.isnan(fused).all())


@pytest.mark.parametrize("ref_nan", [False, True])
@pytest.mark.parametrize("kind", sorted(ORACLE_KINDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_headline_chain_equals_the_oracle(ops, dev, lut, shape, kind, ref_nan):
    from oracle import chain_oracle as CO
    data, dlut = lut
    x, ref = _inputs(shape, kind, ref_nan, dev)
    F, H, W = SHAPES[shape]
    stream = ops.rng.reserve(4 * H * W * 3, 8, dev, torch.Generator(device=dev).manual_seed(42))
    ref_ms = ops.reference_stats(ref)
    spec = ops.ChainSpec(grain=(0.04, 0.5, 4), lut=(dlut, 10.0), colormatch=(ref_ms, 1.0), sharpen=("unsharp", 0.5, False), cm_chunk=1)
    out = ops.fused_chain(x, spec, plans=(ops.NoisePlan(4, stream, chunk0=3), None, 1))
    want = CO.headline_chain(x.cpu(), dev, stages=("grain", "lut", "colormatch", "sharpen"), stream=stream, chunk0=3, chunk_frames=4,
                             lut_cpu=data, reference_dev=ref, cm_batch=1)
    assert _same(out, want), (shape, kind, ref_nan)

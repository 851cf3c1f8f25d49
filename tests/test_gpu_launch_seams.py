"""Every entry point that launches "one record per blockIdx.y / blockIdx.z" splits a call into launches of at most 32768 records
(`launch_chunks`, csrc/vrg_common.hpp) and has to advance by hand everything its chunk lambda indexes by record: source and destination
pointers, descriptor and index tables, scratch, statistics rows, the Philox chunk index, the `f % ref_frames` mapping.  A forgotten
`+ f0` redoes records 0..2 or writes them to the wrong place, and no size below 32769 records shows it.

The tests of this file run each such entry point over 32768 + 3 records (or the next count its alignment accepts).  Every record's content
depends on its index (32768 % 7 == 1, so records 32768.. are not records 0..), all records are compared, against the reference and with
the comparison of the entry point's own GPU test, and where the wrapper takes an `out` it is a slice of a larger buffer whose guard frames
must come back untouched.  SEAMS lists every chunked launch of csrc/ with the test that crosses its seam."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import restated as R
import crop_support as CS
import prepare_support as PS
import resize_support as RS
import stencil_support as SS
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu

LAUNCH = 32768                           # LAUNCH_RECORDS of csrc/vrg_common.hpp
N = LAUNCH + 3
K = 7                                    # distinct base records; record i uses base i % 7 or (i * 5) % 7
GUARD = 7.25
GUARD_U8 = 0x5A
ULP1 = 2.0 ** -23
CM_E2E_DEVICE_ULP = 32                   # tests/test_gpu_parity.py:410, the budget of test_colour_match_end_to_end_ulp_budget_vs_device_oracle

#: (source of the chunked launch, what it launches, the test that crosses its 32768-record seam -- or why none can[, launch_chunks call
#: sites the row stands for, 1 if not given])
SEAMS = (
    ("vrg_stencil.hip k_stencil3x3 (launch_chunks)", "generic stencil route: C not 3 / 4, or RGBA off the 16-byte grid",
     "test_gpu_launch_seams::test_generic_stencil_past_one_launch"),
    ("vrg_stencil.hip launch_stencil_flat (own loop)", "flat march: splits at 2^30 / (strips x segments) frames", "out of reach: 2^30 waves"),
    ("vrg_adjust.hip launch_adjust (launch_chunks)", "vrg_adjust_f32 / _u8: point, clarity 3 / 9, sharpen, both through the tmp ring",
     "test_gpu_launch_seams::test_adjust_past_one_launch"),
    ("vrg_adjust.hip vrg_u8_channel_sums (one launch, refuses > 65535 frames)", "opening colour match sums",
     "test_gpu_launch_seams::test_channel_sums_of_more_frames_than_one_launch_takes"),
    ("vrg_pointwise.hip vrg_colormatch_apply_f32 (launch_chunks, aligned to ref_frames)", "colour-match apply pass",
     "test_gpu_launch_seams::test_colour_match_apply_past_one_launch"),
    ("vrg_chain.hip launch_stats (launch_chunks, aligned to the noise chunk)", "pass 1: Lab image and fp64 statistics",
     "test_gpu_launch_seams::test_chain_statistics_past_one_launch, test_fused_chain_past_one_launch"),
    ("vrg_chain.hip launch_chain, point-wise route (own loop, aligned to noise chunk and ref_frames)", "fused chain without a stencil",
     "test_gpu_launch_seams::test_fused_chain_past_one_launch[*-pointwise], test_fused_chain_with_three_reference_frames_past_one_launch, "
     "test_fused_chain_with_both_alignments_past_one_launch"),
    ("vrg_chain.hip launch_chain, tile route (own loop)", "fused chain with a stencil: splits at 2^23 / tiles per frame", "out of reach: 2^23 tiles"),
    ("vrg_apply_march.hip launch_apply_march_t (own loop)", "pass 2 march: splits at 2^30 / (strips x segments) frames", "out of reach: 2^30 waves"),
    ("vrg_march.hip launch_march (own loop over noise chunks)", "grain -> (LUT) -> sharpen march: one launch per run of whole noise chunks",
     "test_gpu_parity::test_fused_chain_across_several_philox_groups (no 32768 seam: the grid is one-dimensional)"),
    ("vrg_resize.hip (launch_chunks)", "frame resize / restore", "test_gpu_launch_seams::test_resize_and_restore_past_one_launch"),
    ("vrg_crop.hip (launch_chunks)", "crop sequence", "test_gpu_launch_seams::test_crop_sequence_past_one_launch"),
    ("vrg_prepare.hip (launch_chunks)", "Prepare, with and without an index table", "test_gpu_launch_seams::test_prepare_past_one_launch"),
    ("vrg_thumb.hip vrg_thumb_rows_u8 (launch_chunks)", "contact-sheet / Pillow thumbnails: one entry per blockIdx.z",
     "test_gpu_launch_seams::test_pillow_thumbnails_past_one_launch"),
    ("vrg_thumbs.hip vrg_face_thumbs_u8 (launch_chunks)", "landmark input: 320 x 320 thumbnails of the face bytes",
     "test_gpu_launch_seams::test_landmark_input_past_one_launch"),
    ("vrg_sheet.hip sheet_rows_launch (launch_chunks)", "reference sheet panels", "test_gpu_launch_seams::test_sheet_panels_past_one_launch"),
    ("vrg_msr.hip vrg_msr_frames_f32 (launch_chunks)", "MSR frames", "test_gpu_launch_seams::test_msr_frames_past_one_launch"),
    ("vrg_composite.hip vrg_composite_stats_f32 (launch_chunks)", "n_match statistics rows",
     "test_gpu_launch_seams::test_composite_statistics_past_one_launch"),
    ("vrg_composite.hip vrg_face_bytes_u8 (launch_chunks)", "face bytes", "test_gpu_launch_seams::test_face_bytes_past_one_launch"),
    ("vrg_composite.hip vrg_warp_affine_u8 (launch_chunks)", "byte Lanczos-4 affine warp",
     "test_gpu_launch_seams::test_warp_affine_past_one_launch"),
    ("vrg_probe.hip (own loop)", "debug probes of libvrgdg_hip_debug.so: not a product entry point", "not a product path"),
    ("vrg_farface.hip (launch_chunks)", "far-face resize records and masks", "test_gpu_byte_movers::test_*_past_one_launch", 2),
    ("vrg_facefix.hip (launch_chunks)", "builder crops, masks, resize statistics", "test_gpu_byte_movers::test_*_past_one_launch", 3),
    ("vrg_grid.hip (launch_chunks)", "video grid", "test_gpu_grid::test_chunked_launch"),
    ("vrg_assemble.hip (launch_chunks)", "music-video assembly", "test_gpu_assemble::test_more_frames_than_one_launch_takes"),
)


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _rand(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _guarded(n, tail, dtype, dev, shift=0):
    """-> (buffer, out): `out` is a contiguous [n, *tail] view of a buffer filled with the guard value, one frame (plus `shift` elements:
    off the 16-byte grid) into it and one frame (less `shift`) short of its end"""
    fe = int(np.prod(tail))
    fill = GUARD_U8 if dtype == torch.uint8 else GUARD
    raw = torch.full(((n + 2) * fe,), fill, dtype=dtype, device=dev)
    return raw, raw[fe + shift:fe + shift + n * fe].view(n, *tail)


def _guards_intact(raw, out):
    fill = GUARD_U8 if raw.dtype == torch.uint8 else GUARD
    first = (out.data_ptr() - raw.data_ptr()) // raw.element_size()
    return bool((raw[:first] == fill).all()) and bool((raw[first + out.numel():] == fill).all())


def _same_bits(got, want, what):
    """all records, bit for bit (NaN equals NaN of the same payload); names the first differing record"""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = {4: torch.int32, 8: torch.int64, 1: torch.uint8}[got.element_size()]
    bad = (got.view(view) != want.view(view)).reshape(got.shape[0], -1).any(dim=1)
    if bool(bad.any()):
        first = int(torch.nonzero(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {got.shape[0]} records differ, the first is record {first}: got {got[first].flatten()[:6].tolist()} "
                    f"want {want[first].flatten()[:6].tolist()}")


def _differs_past_the_seam(want):
    """the expected record 32768 is not the expected record 0 (nor 32769 record 1, 32770 record 2): redoing the first records would fail"""
    want = want.detach().cpu()
    for i in range(want.shape[0] - LAUNCH):
        assert not torch.equal(want[LAUNCH + i], want[i]), i


def test_the_table_names_a_test_for_every_chunked_launch():
    """every `launch_chunks(` call site of csrc/ is counted by a row of SEAMS, every row names a test that exists or says why no test can
    cross its seam ("out of reach: ...", "not a product path")"""
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    sites = {}
    for name in sorted(os.listdir(os.path.join(PKG_DIR, "csrc"))):
        if name.endswith(".hip"):
            with open(os.path.join(PKG_DIR, "csrc", name), encoding="utf-8") as fh:
                n = len(re.findall(r"\blaunch_chunks\(", fh.read()))
            if n:
                sites[name] = n
    rows = {}
    for row in SEAMS:
        if "(launch_chunks" in row[0]:
            name = row[0].split(" ")[0]
            rows[name] = rows.get(name, 0) + (row[3] if len(row) > 3 else 1)
    assert sites and rows == sites, (rows, sites)
    for row in SEAMS:
        test = row[2]
        if "::" not in test:
            assert test.startswith("out of reach: ") or test == "not a product path", row
            continue
        module = test.split("::")[0]
        with open(os.path.join(here, module + ".py"), encoding="utf-8") as fh:
            text = fh.read()
        for part in test.split("::", 1)[1].split(","):
            fn = part.strip().split("[")[0].split(" ")[0].replace("test_gpu_launch_seams::", "")
            if "*" in fn:
                a, b = fn.split("*", 1)
                assert any(line.startswith("def " + a) and b in line for line in text.splitlines()), test
            else:
                assert f"def {fn}(" in text, test


# ------------------------------------------------------------------------------------------------
# the stand-alone stencil: only its generic route puts frames on blockIdx.y
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,shift", [((3, 5, 1), 0), ((2, 2, 4), 1)], ids=["3x5x1", "2x2x4-off-grid"])
def test_generic_stencil_past_one_launch(ops, dev, shape, shift):
    """k_stencil3x3 over 32771 frames: one channel (on the grid), and RGBA frames whose output is one float off the 16-byte grid (what keeps
    them from the flat march).  The oracle and the pairing of tests/test_gpu_stencil.py (stencil_support.expected), bit for bit."""
    base = _rand((K, *shape), 5101, -0.1, 1.1)
    which = (torch.arange(N) * 5) % K
    x = base[which].contiguous().to(dev)
    assert SS.route(N, *shape, aligned=shift == 0).route == "generic"
    for op, strength, zero in (("unsharp", 0.5, False), ("laplacian", 0.8, True), ("sobel", 0.8, False)):
        want = SS.expected(base, op, strength, zero)[which]
        _differs_past_the_seam(want)
        raw, out = _guarded(N, shape, torch.float32, dev, shift)
        assert not shift or out.data_ptr() % 16 == 4
        got = ops.stencil3x3(x, op, strength, zero, out=out)
        assert got.data_ptr() == out.data_ptr()
        _same_bits(got, want, f"{op} zero={zero} {shape}")
        assert _guards_intact(raw, out), (op, shape)
    assert torch.equal(x.cpu(), base[which])


# ------------------------------------------------------------------------------------------------
# the 13-slider Adjust
# ------------------------------------------------------------------------------------------------
def _adjust_want(x, settings):
    """tests/test_gpu_parity.py, _adjust_want: the reference on the CPU, the vignette distance with the correctly rounded sqrt"""
    norm = R.normalize_adjust_settings(settings)
    if norm["enabled"] and norm["vignette"] > 0.0:
        return R.adjust_tensor(x, settings, ieee_sqrt=True).contiguous()
    return R.adjust_tensor(x, settings).contiguous()


ADJUST_SEAMS = [
    ((1, 1), {"exposure": 20, "temperature": 60, "blacks": 50, "fade": 30}, "point"),
    ((2, 2), {"sharpen": 100, "whites": -35, "tint": 44}, "sharpen"),
    ((3, 3), {"clarity": 55, "vignette": 80}, "clarity3"),                 # the smallest frame whose box is 3 (k_adjust_box_small)
    ((3, 3), {"clarity": 55, "sharpen": 25, "exposure": 20}, "both3"),     # ... and through the tmp ring
    ((9, 9), {"clarity": -40, "temperature": 60}, "clarity9"),             # the smallest frame whose box is 9 (k_adjust_box<9>)
    ((9, 9), {"clarity": 55, "sharpen": 25, "vignette": 80, "fade": 30}, "both9"),
]


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("hw,settings,name", ADJUST_SEAMS, ids=[c[2] for c in ADJUST_SEAMS])
def test_adjust_past_one_launch(ops, pkg, dev, hw, settings, name, u8):
    """vrg_adjust_f32 / vrg_adjust_u8 over 32771 frames, every route of launch_adjust; bit for bit / byte for byte against the oracle of
    test_adjust_kernels_vs_oracle_across_tiles and test_adjust_u8_equals_convert_adjust_convert (tests/test_gpu_parity.py)."""
    from comfyui_vrgamedevgirl_amd import VRGDG_LUTVideoTools as LVT
    shape = (*hw, 3)
    which = torch.arange(N) % K
    terms = ops.adjust_terms(LVT._normalize_adjust_settings(settings))
    if u8:
        g = torch.Generator().manual_seed(5200 + hw[0])
        base = torch.randint(0, 256, (K, *shape), generator=g, dtype=torch.uint8)
        want = torch.from_numpy(np.stack(R.tensor_to_frames(_adjust_want(R.frames_to_tensor(list(base.numpy())), settings))))
    else:
        base = _rand((K, *shape), 5200 + hw[0], -0.1, 1.1)
        want = _adjust_want(base, settings)
    want = want[which]
    _differs_past_the_seam(want)
    x = base[which].contiguous().to(dev)
    raw, out = _guarded(N, shape, base.dtype, dev)
    ws_raw, ws = _guarded(N, shape, torch.float32, dev)
    got = ops.adjust(x, terms, out=out, workspace=ws)
    assert got.data_ptr() == out.data_ptr()
    _same_bits(got, want, f"adjust {name} {'u8' if u8 else 'f32'}")
    assert _guards_intact(raw, out) and _guards_intact(ws_raw, ws), name
    assert torch.equal(x.cpu(), base[which])


def test_channel_sums_of_more_frames_than_one_launch_takes(pkg, dev):
    """vrg_u8_channel_sums takes at most 65535 frames a call (blockIdx.y): the Python caller splits, and every frame's sums are numpy's"""
    from comfyui_vrgamedevgirl_amd import VRGDG_WorkflowRunnerNodes as WR
    n = 65536 + 1
    g = torch.Generator().manual_seed(5300)
    frames = torch.randint(0, 256, (n, 1, 1, 3), generator=g, dtype=torch.uint8)
    got = WR._channel_sums(frames.to(dev))
    a = frames.numpy().reshape(n, -1, 3).astype(np.uint64)
    want = np.stack([a.sum(axis=1), (a * a).sum(axis=1)], axis=-1).astype(np.int64)          # test_u8_channel_sums_are_exact
    assert got.shape == (n, 3, 2) and got.dtype == torch.int64
    bad = np.flatnonzero((got.cpu().numpy() != want).reshape(n, -1).any(axis=1))
    assert bad.size == 0, (bad.size, int(bad[0]))
    assert not np.array_equal(want[65535], want[0]) and not np.array_equal(want[65536], want[1])


# ------------------------------------------------------------------------------------------------
# colour match: the apply pass, whose reference statistics repeat every R frames
# ------------------------------------------------------------------------------------------------
def _spread_frames(n, seed):
    """[n, 2, 2, 3] frames whose four pixels lie far apart in Lab (reddish, greenish, bluish, grey; +- 0.1 at random): no frame's
    statistics are degenerate, so that the ulp budgets of the large frames of tests/test_gpu_parity.py hold for four pixels"""
    corners = torch.tensor([[0.8, 0.2, 0.2], [0.2, 0.7, 0.25], [0.25, 0.2, 0.8], [0.5, 0.5, 0.5]]).view(1, 2, 2, 3)
    return (corners + _rand((n, 2, 2, 3), seed, -0.1, 0.1)).contiguous()


def _lab_nchw(x_dev):
    return R.kornia_rgb_to_lab(x_dev.permute(0, 3, 1, 2))


@pytest.mark.parametrize("Rn", [3, 5])
def test_colour_match_apply_past_one_launch(ops, dev, Rn):
    """ops.colormatch_apply with R = 3 and 5 reference frames over the next multiple of R above 32768 frames of 2 x 2, img_ms and ref_ms rows
    that differ per frame: bit-equal to the device oracle of test_colour_match_apply_bit_equal_device_oracle_with_injected_statistics
    (R.color_match_apply evaluated by torch on this GPU, frame f against reference frame f % R), and equal to the call made in two pieces.
    (Before launch_chunks took an alignment the second launch started at frame 32768, not a multiple of R: VRG_ERR_UNSUPPORTED.)"""
    F = -(-(LAUNCH + 1) // Rn) * Rn
    assert F > LAUNCH and F % Rn == 0 and F - Rn <= LAUNCH and LAUNCH % Rn != 0
    k = 0.8
    x = _spread_frames(F, 5400 + Rn).to(dev)
    ims = torch.stack([_rand((F, 3), 5410 + Rn, -20.0, 60.0), _rand((F, 3), 5420 + Rn, 2.0, 30.0)], dim=-1).contiguous().to(dev)
    rms = torch.stack([_rand((Rn, 3), 5430 + Rn, -20.0, 60.0), _rand((Rn, 3), 5440 + Rn, 2.0, 30.0)], dim=-1).contiguous().to(dev)
    rep = rms.repeat(F // Rn, 1, 1)                                                       # frame f -> reference frame f % R
    want = R.color_match_apply(_lab_nchw(x), ims[..., 0].view(F, 3, 1, 1), ims[..., 1].view(F, 3, 1, 1), rep[..., 0].view(F, 3, 1, 1),
                               rep[..., 1].view(F, 3, 1, 1), k).clamp(0, 1).permute(0, 2, 3, 1).contiguous()
    _differs_past_the_seam(want)
    got = ops.colormatch_apply(x, ims, rms, k, cm_math="device")
    _same_bits(got, want, f"colour-match apply, R = {Rn}")
    cut = 32766 - 32766 % Rn                                                               # two pieces, each a whole number of rounds of R
    pieces = torch.cat([ops.colormatch_apply(x[:cut], ims[:cut], rms, k, cm_math="device"),
                        ops.colormatch_apply(x[cut:], ims[cut:], rms, k, cm_math="device")])
    _same_bits(got, pieces, f"colour-match apply in one call and in two, R = {Rn}")


# ------------------------------------------------------------------------------------------------
# the fused chain and its statistics pass with a grain batch size of 3: noise chunks that no power of two holds
# ------------------------------------------------------------------------------------------------
GRAIN = (0.06, 0.3, 3)
F_GRAIN = LAUNCH + 3                     # plan_noise: a main segment of 10923 chunks = 32769 frames, and a tail of 2


@functools.lru_cache(maxsize=None)
def _identity_lut(device_index):
    from comfyui_vrgamedevgirl_amd import VRGDG_IV_Adjustments as iv
    from comfyui_vrgamedevgirl_amd import ops as _ops
    data = R.parse_cube_file(os.path.join(iv.LUTS_DIR, "AMD_Identity_17.cube"))
    return data, _ops.upload_lut(data, torch.device("cuda", device_index))


def _device_noise(frames, step, tail, dev):
    """the N(0,1) tensors the reference's chunk loop draws on this GPU, one torch.randn per `step` frames, from the current generator state"""
    return torch.cat([torch.randn((min(step, frames - i), *tail), device=dev) for i in range(0, frames, step)]).cpu()


def _grain_lut_oracle(x, data, dev, seed):
    """grain (batch size 3) -> identity cube at full strength on the CPU, with the very noise torch draws on the device: the pairing of
    test_fused_chain_equals_sequential_operators_and_oracle (tests/test_gpu_parity.py)"""
    torch.manual_seed(seed)
    noise = _device_noise(x.shape[0], GRAIN[2], tuple(x.shape[1:]), dev)
    o = R.fast_film_grain(x, GRAIN[0], GRAIN[1], GRAIN[2], noise_fn=lambda i, shp: noise[i:i + shp[0]])
    return R.apply_lut_with_strength(o, data, 10.0)


def test_chain_statistics_past_one_launch(ops, dev):
    """ops.chain_stats, grain batch size 3 -> LUT over 32771 frames of 2 x 2 (launch_stats: the general kernel, tiny frames).  The Lab image is
    bit-equal to the device oracle's Lab of the oracle's grain -> LUT image (test_lab_image_of_the_statistics_pass_bit_equal_device_oracle); the
    statistics rows against the fp64 statistics of that Lab image within the bounds of test_shared_philox_statistics_pass (n exact, mean
    1e-12, M2 1e-11, each relative to 1 + |value|).  And the whole call equals the call on frames [0, 32766) and [32766, 32771).
    (Before launch_chunks took an alignment: VRG_ERR_UNSUPPORTED, 32768 is not a multiple of 3.)  chain_stats is the fp64 pass alone: it has no
    colour-match stage and reads neither cm_stats nor cm_chunk, so there is one case."""
    F = F_GRAIN
    data, dlut = _identity_lut(dev.index)
    x = _spread_frames(F, 5500)
    xd = x.to(dev)
    spec = ops.ChainSpec(grain=GRAIN, lut=(dlut, 10.0))
    y = _grain_lut_oracle(x, data, dev, 31)
    lab_want = _lab_nchw(y.to(dev)).permute(0, 2, 3, 1).contiguous()
    _differs_past_the_seam(lab_want)
    torch.manual_seed(31)
    plans = ops.plan_noise(F, 12, GRAIN[2], dev)
    assert plans[0].chunk_frames == 3 and plans[2] == 10923 and plans[1].chunk_frames == 2
    raw, lab = _guarded(F, (2, 2, 3), torch.float32, dev)
    stats = ops.chain_stats(xd, spec, plans=plans, lab_out=lab)
    _same_bits(lab, lab_want, "Lab image of pass 1")
    assert _guards_intact(raw, lab)
    l64 = lab_want.double().cpu().reshape(F, 4, 3)
    mean64 = l64.mean(dim=1)
    m2_64 = ((l64 - mean64[:, None]) ** 2).sum(dim=1)
    s = stats.cpu()
    assert torch.equal(s[..., 0], torch.full((F, 3), 4.0, dtype=torch.float64))
    bad = ((s[..., 1] - mean64).abs() > 1e-12 * (1 + mean64.abs())) | ((s[..., 2] - m2_64).abs() > 1e-11 * (1 + m2_64.abs()))
    assert not bool(bad.any()), (int(bad.any(dim=1).sum()), int(torch.nonzero(bad.any(dim=1))[0]))
    assert not torch.equal(mean64[LAUNCH], mean64[0])
    cut = 32766
    lab2 = torch.empty_like(xd)
    halves = torch.cat([ops.chain_stats(xd[:cut], spec, plans=ops.slice_plans(plans, 0, cut), lab_out=lab2[:cut]),
                        ops.chain_stats(xd[cut:], spec, plans=ops.slice_plans(plans, cut, F - cut), lab_out=lab2[cut:])])
    _same_bits(stats, halves, "statistics in one call and in two")
    _same_bits(lab, lab2, "Lab image in one call and in two")


@pytest.mark.parametrize("sharpen", [("unsharp", 0.5, False), None], ids=["tile", "pointwise"])
@pytest.mark.parametrize("cm_stats", ["fp64", "device"])
def test_fused_chain_past_one_launch(ops, dev, cm_stats, sharpen):
    """ops.fused_chain, grain batch size 3 -> identity 17 cube -> colour match (-> unsharp) over 32771 frames of 2 x 2: pass 1 through
    launch_stats in two launches of whole noise chunks, pass 2 through launch_chain's tile route (one launch) or, without the stencil, its
    point-wise route (two launches: the statistics rows of the second start at frame 32768).  Against the oracle composition of
    test_fused_chain_with_colour_match (tests/test_gpu_parity.py): the colour match of the reference evaluated by torch on the device in one
    calls of 32766 frames and the rest (the node's batch_size; cm_chunk says the same to the chain: torch's reductions give bits that depend
    on the shape of the call, ops.lab_stats_device) -- bit for bit with the device statistics, within CM_E2E_DEVICE_ULP (twice that behind the
    unsharp at 0.5, as there) with the fp64 statistics.  With both, the whole call also equals the call on frames [0, 32766) and
    [32766, 32771), whose statistics calls are those two."""
    F = F_GRAIN
    data, dlut = _identity_lut(dev.index)
    x = _spread_frames(F, 5600)
    ref = _rand((1, 30, 30, 3), 5601)
    xd, refd = x.to(dev), ref.to(dev)
    k = 0.9
    o = _grain_lut_oracle(x, data, dev, 41)
    cut = 32766                                      # the reference's batch_size: calls of 32766 and 5 frames, for the oracle, the chain and its pieces
    o = R.color_match(o.to(dev), refd, k, cut).cpu()
    if sharpen:
        o = R.unsharp(o, sharpen[1], sharpen[2])
    _differs_past_the_seam(o)
    ref_ms = ops.reference_stats(refd, cm_stats=cm_stats)
    spec = ops.ChainSpec(grain=GRAIN, lut=(dlut, 10.0), colormatch=(ref_ms, k), sharpen=sharpen, cm_stats=cm_stats, cm_chunk=cut)
    torch.manual_seed(41)
    plans = ops.plan_noise(F, 12, GRAIN[2], dev)
    raw, out = _guarded(F, (2, 2, 3), torch.float32, dev)
    got = ops.fused_chain(xd, spec, plans=plans, out=out)
    assert got.data_ptr() == out.data_ptr() and _guards_intact(raw, out)
    if cm_stats == "device":
        _same_bits(got, o, "grain -> LUT -> colour match (-> unsharp) vs the oracle, device statistics")
    else:
        d = (got.double().cpu() - o.double()).abs().reshape(F, -1).max(dim=1).values / ULP1
        print(f"fused chain, fp64 statistics, sharpen={sharpen}: max {float(d.max()):.2f} ulp(1.0) at frame {int(d.argmax())}")
        budget = CM_E2E_DEVICE_ULP * (2 if sharpen else 1)
        assert float(d.max()) <= budget, (float(d.max()), int(d.argmax()), int((d > budget).sum()))
    halves = torch.cat([ops.fused_chain(xd[:cut], spec, plans=ops.slice_plans(plans, 0, cut)),
                        ops.fused_chain(xd[cut:], spec, plans=ops.slice_plans(plans, cut, F - cut))])
    _same_bits(got, halves, "the chain in one call and in two")
    if cm_stats == "fp64":
        _same_bits(ops.fused_chain(xd, spec, plans=plans, cache_lab=False), got, "recomputing form (grain in pass 2)")


@pytest.mark.parametrize("cm_stats", ["fp64", "device"])
def test_fused_chain_with_three_reference_frames_past_one_launch(ops, dev, cm_stats):
    """No grain, colour match against R = 3 reference frames, no stencil, 32772 frames of 2 x 2: launch_chain's point-wise route in launches of
    32766 frames (its other alignment).  The oracle: the reference's colour match in calls of 3 frames (frame f against reference frame
    f % 3), its element-wise path evaluated by torch on the device over all frames at once with the statistics of each frame
    (R.color_match_apply, as in test_colour_match_apply_bit_equal_device_oracle_with_injected_statistics): with the fp64 statistics our own
    finalised rows go in (what is under test is the apply pass and the rows' offsets: bit for bit), with the device statistics torch's
    reductions over calls of 3 frames."""
    F = LAUNCH + 4
    assert F % 3 == 0
    k = 0.6
    x = _spread_frames(F, 5700)
    ref = _rand((3, 8, 8, 3), 5701)
    xd, refd = x.to(dev), ref.to(dev)
    ref_ms = ops.reference_stats(refd, cm_stats=cm_stats)
    lab = _lab_nchw(xd)
    if cm_stats == "fp64":
        ims = ops.finalize_stats(ops.lab_stats(xd))
        l64 = lab.double().permute(0, 2, 3, 1).reshape(F, 4, 3)
        sd64 = l64.std(dim=1, unbiased=True) + float(np.float32(1e-5))
        assert float(((ims[..., 0].double() - l64.mean(dim=1)).abs() / (l64.mean(dim=1).abs() * ULP1)).max()) <= 0.5      # tests/test_gpu_parity.py:804
        assert float(((ims[..., 1].double() - sd64).abs() / (sd64 * ULP1)).max()) <= 1.0
    else:
        calls = [R.lab_stats(lab[i:i + 3]) for i in range(0, F, 3)]                        # tests/test_gpu_parity.py, _stats_per_frame
        ims = torch.cat([torch.stack([mu.flatten(1), sd.flatten(1)], dim=-1) for mu, sd in calls]).contiguous()
    rep = ref_ms.repeat(F // 3, 1, 1)
    want = R.color_match_apply(lab, ims[..., 0].reshape(F, 3, 1, 1), ims[..., 1].reshape(F, 3, 1, 1), rep[..., 0].reshape(F, 3, 1, 1),
                               rep[..., 1].reshape(F, 3, 1, 1), k).clamp(0, 1).permute(0, 2, 3, 1).contiguous()
    _differs_past_the_seam(want)
    spec = ops.ChainSpec(colormatch=(ref_ms, k), cm_stats=cm_stats, cm_chunk=3)
    raw, out = _guarded(F, (2, 2, 3), torch.float32, dev)
    got = ops.fused_chain(xd, spec, out=out)
    _same_bits(got, want, f"colour match against three reference frames, {cm_stats} statistics")
    assert _guards_intact(raw, out)
    _same_bits(ops.fused_chain(xd, spec, cache_lab=False), want, "recomputing form")


# ------------------------------------------------------------------------------------------------
# frame resize / restore, Prepare and the crop sequence: torch itself, run live on seven base frames, is the reference
# ------------------------------------------------------------------------------------------------
RESIZE_SHAPE, RESIZE_TARGET = (K, 2, 3, 3), (2, 3)            # 2 rows x 3 columns -> 3 rows x 2 columns, a stretch
RESTORE_ORIGINALS = (K, 3, 2, 4)                              # RGBA originals: the fourth channel is clamped and kept
RESIZE_CASES = ([RS.fit_case(5800, RESIZE_SHAPE, RESIZE_TARGET, RS.STRETCH, m) for m in (RS.BICUBIC, RS.BILINEAR)] +
                [RS.restore_case(5800, RESIZE_SHAPE, 5801, RESTORE_ORIGINALS, RS.STRETCH, m, 0.65, K) for m in (RS.BICUBIC, RS.BILINEAR)])


@pytest.fixture(scope="module")
def torch_live(tmp_path_factory):
    """torch's own result of RESIZE_CASES, from one child process (resize_support.torch_results); shared, never written"""
    return RS.torch_results(RESIZE_CASES, tmp_path_factory.mktemp("seams_torch"))


@pytest.mark.parametrize("ci", [0, 1], ids=["bicubic", "bilinear"])
def test_resize_and_restore_past_one_launch(ops, dev, torch_live, ci):
    """ops.resize_frames and ops.restore_frames over 32771 frames (k_resize_bicubic and k_resize_direct, each with and without the blend
    over the originals, whose pointer the chunk advances too): no differing element against torch run live, the comparison of
    tests/test_gpu_resize_torch.py (resize_support.mismatches)."""
    which = torch.arange(N) % K
    method = RESIZE_CASES[ci]["method"]
    (base,) = torch_live.inputs(ci)
    want = torch.from_numpy(torch_live[ci])[which]
    _differs_past_the_seam(want)
    x = base[which].contiguous().to(dev)
    raw, out = _guarded(N, (3, 2, 3), torch.float32, dev)
    got = ops.resize_frames(x, RESIZE_TARGET[0], RESIZE_TARGET[1], RS.STRETCH, method, out=out)
    assert RS.mismatches(got.cpu().numpy(), want.numpy()) == 0
    _same_bits(got, want, f"resize {method}")
    assert _guards_intact(raw, out)
    work, originals = torch_live.inputs(ci + 2)
    want = torch.from_numpy(torch_live[ci + 2])[which]
    _differs_past_the_seam(want)
    o = originals[which].contiguous().to(dev)
    raw, out = _guarded(N, (3, 2, 4), torch.float32, dev)
    got = ops.restore_frames(x, o, 2, 3, RS.STRETCH, method, 0.65, out=out)
    assert torch.equal(work, base)
    _same_bits(got, want, f"restore {method}")
    assert _guards_intact(raw, out) and torch.equal(o.cpu(), originals[which])


@pytest.mark.parametrize("ci", [0, 1], ids=["bicubic", "bilinear"])
@pytest.mark.parametrize("indexed", [True, False], ids=["index-table", "in-order"])
def test_prepare_past_one_launch(ops, dev, torch_live, ci, indexed):
    """ops.prepare_frames to 32771 output frames, through an index table whose entries vary with the output frame ((i * 5) % 7 of seven
    source frames) and without one (32771 source frames); the staged bicubic and the direct kernel.  fp32: no differing element against torch
    run live; bytes: numpy's (x * 255).round() of that (prepare_support.quantise, test_special_values_reach_the_bytes)."""
    method = RESIZE_CASES[ci]["method"]
    (base,) = torch_live.inputs(ci)
    which = (torch.arange(N) * 5) % K if indexed else torch.arange(N) % K
    want = torch.from_numpy(torch_live[ci])[which]
    _differs_past_the_seam(want)
    g = ops.resize_geometry(2, 3, RESIZE_TARGET[0], RESIZE_TARGET[1], RS.STRETCH)
    if indexed:
        f32, u8 = ops.prepare_frames(base.to(dev), g, method, [int(i) for i in which])
    else:
        f32, u8 = ops.prepare_frames(base[which].contiguous().to(dev), g, method)
    _same_bits(f32, want, f"prepare {method} fp32")
    _same_bits(u8, torch.from_numpy(PS.quantise(want.numpy())), f"prepare {method} bytes")


def test_crop_sequence_past_one_launch(ops, dev, tmp_path):
    """ops.crop_resize, 32771 records over one 6 x 7 RGBA frame: seven boxes (2 x 2 to 5 x 4, at different places), record i takes box
    (i * 5) % 7, work frames of 3 x 2.  No differing element against the host arithmetic of tests/test_gpu_crop.py (crop_support.host_crop)."""
    hm = CS.build_host_lib(tmp_path)
    frame = CS.make_frames((1, 6, 7, 4), 5900)
    boxes = [(0, 0, 2, 2), (1, 2, 6, 6), (3, 1, 7, 4), (2, 0, 5, 5), (0, 3, 4, 6), (4, 2, 7, 6), (1, 1, 3, 5)]
    records = np.array([((t * 7 + l) * 4, 7 * 4, 4, r - l, b - t) for l, t, r, b in boxes], dtype=np.int64)
    which = (np.arange(N) * 5) % K
    want = torch.from_numpy(CS.host_crop(hm, frame, records, (3, 2)))[torch.from_numpy(which)]
    _differs_past_the_seam(want)
    x = torch.from_numpy(frame).to(dev)
    raw, out = _guarded(N, (3, 2, 3), torch.float32, dev)
    got = ops.crop_resize(x, records[which], (3, 2), out=out)
    assert CS.mismatches(got.cpu().numpy(), want.numpy()) == 0
    _same_bits(got, want, "crop records")
    assert _guards_intact(raw, out) and np.array_equal(x.cpu().numpy(), frame)


# ------------------------------------------------------------------------------------------------
# the landmark-aligned composite's launchers: byte warp, face bytes, composite statistics, landmark input
# ------------------------------------------------------------------------------------------------
def _np_rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _rows_differ_past_the_seam(want):
    for i in range(len(want) - LAUNCH):
        assert not np.array_equal(want[LAUNCH + i], want[i]), i


def _first_bad(got, want):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))
    return (int(bad.size), int(bad[0])) if bad.size else None


def test_warp_affine_past_one_launch(ops, dev):
    """ops.warp_affine_u8 over 32771 frames of 4 x 5 -> 3 x 2: frame i is base frame i % 7 under transform (i * 5) % 7 of seven (the warp
    records vary with the frame).  Byte for byte against the restatement of tests/test_gpu_landmark.py (warp_support.restated)."""
    import warp_support as WS
    base = _np_rng(6000).integers(0, 256, (K, 4, 5, 3), dtype=np.uint8)
    transforms = [WS.similarity(1.0 + 0.07 * j, 9.0 * j - 20.0, 0.3 * j, -0.2 * j, (2.0, 1.5)) for j in range(K)]
    which = np.arange(N) % K
    want7 = np.stack([WS.restated(base[j], transforms[(j * 5) % K], 3, 2) for j in range(K)])
    want = want7[which]
    _rows_differ_past_the_seam(want)
    x = torch.from_numpy(base[which]).to(dev)
    got = ops.warp_affine_u8(x, [transforms[(int(i) * 5) % K] for i in range(N)], 3, 2)
    assert _first_bad(got.cpu().numpy(), want) is None
    assert np.array_equal(x.cpu().numpy(), base[which])


def _face_rows(n):
    """entry i: original i % 7, crop (i * 5) % 7, a box of 2 x 2 .. 3 x 3 whose place and size go with i % 7"""
    boxes = [(0, 0, 2, 2), (1, 1, 4, 3), (2, 0, 4, 3), (0, 1, 3, 4), (1, 0, 3, 2), (2, 2, 4, 4), (0, 0, 3, 3)]
    return [{"original": i % K, "crop": (i * 5) % K, "box": boxes[i % K]} for i in range(n)]


def test_face_bytes_past_one_launch(ops, dev, tmp_path):
    """ops.face_bytes over 32771 entries on seven 4 x 4 RGBA originals and seven 3 x 3 crops.  As test_face_bytes_equal_the_restatement
    (tests/test_gpu_landmark.py): source = warp_support.quantise(original under the box); generated = quantise of the clamped bicubic face.
    That test reads the face where the opaque composite's alpha is 1; boxes this small have no such pixel, so the face of the seven distinct
    entries comes from the host arithmetic of the composite (composite_support.HostCall.box, the yardstick of tests/test_gpu_composite.py)."""
    import composite_support as CPS
    import warp_support as WS
    originals = torch.from_numpy(_np_rng(6100).random((K, 4, 4, 4), dtype=np.float32) * 1.3 - 0.15).to(dev)
    work = torch.from_numpy(_np_rng(6101).random((K, 3, 3, 3), dtype=np.float32) * 1.2 - 0.1).to(dev)
    rows = _face_rows(N)
    faces = ops.face_bytes(work, rows, 4, 4, originals=originals)
    gen, src = faces.generated.cpu().numpy(), faces.source.cpu().numpy()
    o = originals.cpu().numpy()
    call = CPS.HostCall(CPS.build_host_lib(tmp_path), ops, o, work.cpu().numpy(), rows[:K], ops.CompositeRule("opaque", feather=0), 0.0)
    want_src, want_gen = [], []
    for j in range(K):
        l, t, r, b = rows[j]["box"]
        want_src.append(WS.quantise(o[j, t:b, l:r, :3]))
        want_gen.append(WS.quantise(np.clip(call.box(j)[1][..., :3], 0.0, 1.0)))
    assert not np.array_equal(want_gen[LAUNCH % K], want_gen[0]) and not np.array_equal(want_src[LAUNCH % K], want_src[0])
    assert faces.offsets[LAUNCH] > faces.offsets[LAUNCH - 1] > 0 and len(gen) >= faces.offsets[N - 1] + 27
    bad = [f for f in range(N) if not (np.array_equal(faces.image(gen, f), want_gen[f % K]) and np.array_equal(faces.image(src, f), want_src[f % K]))]
    assert not bad, (len(bad), bad[0])


def test_landmark_input_past_one_launch(ops, dev):
    """ops.face_thumbs of 32771 generated faces (vrg_face_thumbs_u8): every 320 x 320 thumbnail against landmark_input_support.restated of its
    face bytes, byte for byte, as test_face_thumbs_of_face_bytes (tests/test_gpu_landmark_input.py).  The thumbnail size is fixed, so the output
    is 32771 x 307200 bytes (10 GB): it stays on the device and is compared there, in pieces."""
    import landmark_input_support as L
    work = torch.from_numpy(_np_rng(6201).random((K, 3, 3, 3), dtype=np.float32) * 1.2 - 0.1).to(dev)
    faces = ops.face_bytes(work, _face_rows(N), 4, 4)
    gen = faces.generated.cpu().numpy()
    want7 = np.stack([L.restated(faces.image(gen, j)) for j in range(K)]).reshape(K, -1)
    assert len({w.tobytes() for w in want7}) == K
    thumbs, index = ops.face_thumbs(faces, ("generated",))
    assert index == list(range(N)) and tuple(thumbs.shape) == (N, 1, L.SIDE, L.SIDE, 3)
    want_dev = torch.from_numpy(want7).to(dev)
    flat = thumbs.view(N, -1)
    for f0 in range(0, N, 1024):
        f1 = min(N, f0 + 1024)
        same = (flat[f0:f1] == want_dev[torch.arange(f0, f1, device=dev) % K]).all(dim=1)
        assert bool(same.all()), f0 + int(torch.nonzero(~same)[0])
    del thumbs, flat
    torch.cuda.empty_cache()


def test_composite_statistics_past_one_launch(ops, dev, tmp_path):
    """ops.composite_stats with 32771 frames to measure (n_match past one launch: the list of frames and the scratch advance): entry i pastes
    crop (i * 5) % 7 into a 12 x 12 box of original i % 7 placed by i % 7, radial rule, colour match 0.65.  Every record equals
    composite_support.HostCall.truth_stats of the seven distinct entries, as in test_nodes_on_the_fixture (tests/test_gpu_composite.py)."""
    import composite_support as CPS
    hm = CPS.build_host_lib(tmp_path)
    originals = _rand((K, 16, 16, 3), 6300, -0.1, 1.1)
    crops = _rand((K, 4, 4, 3), 6301, -0.1, 1.1)
    entries = [{"original": i % K, "crop": (i * 5) % K, "box": (i % K % 3, i % K // 3, i % K % 3 + 12, i % K // 3 + 12), "strength": 1.0} for i in range(N)]
    rule = ops.CompositeRule("radial", feather=2)
    truth = CPS.HostCall(hm, ops, originals.numpy(), crops.numpy(), entries[:K], rule, 0.65).truth_stats()[:K]
    assert truth[:, 1].sum() >= 4 and len({t.tobytes() for t in truth}) == K
    rec = ops.composite_stats(originals.to(dev), crops.to(dev), entries, rule, 0.65)
    got = np.zeros((N, CPS.STATS_WORDS), dtype=np.uint32)
    f32 = got.view(np.float32)
    got[:, 0], got[:, 1] = rec["count"].cpu().numpy(), rec["matched"].cpu().numpy()
    f32[:, 2:6], f32[:, 6:10], f32[:, 10:14] = rec["crop_mean"].cpu().numpy(), rec["original_mean"].cpu().numpy(), rec["shift"].cpu().numpy()
    assert _first_bad(got, truth[np.arange(N) % K]) is None


# ------------------------------------------------------------------------------------------------
# Pillow thumbnails, reference sheet panels, MSR frames
# ------------------------------------------------------------------------------------------------
def test_pillow_thumbnails_past_one_launch(pkg, dev):
    """far_face_repair.pil_thumbnail of a batch of 32771 images of 5 x 6 asked for (3, 3) (vrg_thumb_rows_u8: one entry per blockIdx.z, then
    the compose pass): every thumbnail is Pillow's own Image.thumbnail(..., BICUBIC, reducing_gap=2.0), as test_thumbnails_equal_pillow."""
    from PIL import Image
    from comfyui_vrgamedevgirl_amd import far_face_repair as ffr
    base = _np_rng(6400).integers(0, 256, (K, 5, 6, 3), dtype=np.uint8)
    want7 = []
    for j in range(K):
        im = Image.fromarray(base[j], "RGB")
        im.thumbnail((3, 3), Image.Resampling.BICUBIC, reducing_gap=2.0)
        want7.append(np.asarray(im))
    want7 = np.stack(want7)
    which = (np.arange(N) * 5) % K
    _rows_differ_past_the_seam(want7[which])
    x = torch.from_numpy(base[which]).to(dev)
    got = ffr.pil_thumbnail(x, (3, 3))
    assert tuple(got.shape) == (N, *want7.shape[1:])
    assert _first_bad(got.cpu().numpy(), want7[which]) is None
    assert np.array_equal(x.cpu().numpy(), base[which])


def test_sheet_panels_past_one_launch(ops, dev):
    """ops.reference_sheet with 32771 panels of 2 x 2 on a 514 x 256 canvas, panel i showing source (i * 5) % 7 of seven byte pictures of
    different sizes (resized, contained or cropped by i % 3): byte for byte Pillow's own sheet (sheet_support.pillow_sheet, the yardstick of
    tests/test_gpu_sheet.py).  The cells left over keep the background."""
    import sheet_support as SH
    sizes = [(3, 5), (5, 3), (4, 4), (2, 2), (6, 2), (3, 3), (2, 7)]
    sources = [_np_rng(6500 + j).integers(0, 256, (h, w, 3), dtype=np.uint8) for j, (h, w) in enumerate(sizes)]
    fits = ("resize", "contain_pad", "cover_crop")
    panels = [SH.P((i * 5) % K, ((i % 257) * 2, (i // 257) * 2, 2, 2), fits[i % 3], (40, 90, 200)) for i in range(N)]
    want = SH.pillow_sheet(sources, panels, (514, 256), (10, 20, 30))
    assert not np.array_equal(want[(LAUNCH // 257) * 2:(LAUNCH // 257) * 2 + 2, (LAUNCH % 257) * 2:(LAUNCH % 257) * 2 + 2], want[:2, :2])
    got = ops.reference_sheet([torch.from_numpy(s).to(dev) for s in sources], [ops.SheetPanel(**p) for p in panels], (514, 256), (10, 20, 30),
                              out_bytes=True)
    bad = np.argwhere((got.cpu().numpy() != want).any(axis=2))
    assert len(bad) == 0, (len(bad), tuple(bad[0]))


def test_msr_frames_past_one_launch(ops, dev):
    """ops.msr_reference_frames of 32771 pictures, one frame each (one descriptor per blockIdx.y): picture i is base picture (i * 5) % 7 of
    seven sizes, one of them the output size (taken unfiltered), stretched to 3 x 2.  Bit for bit msr_support.expected_frames, the expectation
    of test_launch_equals_the_restatement (tests/test_gpu_msr.py)."""
    import msr_support as M
    sizes = [(3, 5), (5, 3), (2, 3), (4, 4), (6, 2), (3, 3), (2, 7)]
    base = [_np_rng(6600 + j).integers(0, 256, (h, w, 3), dtype=np.uint8) for j, (h, w) in enumerate(sizes)]
    want7 = M.expected_frames(base, (3, 2), [1] * K)
    which = (np.arange(N) * 5) % K
    _rows_differ_past_the_seam(want7[which])
    on_dev = [torch.from_numpy(b).to(dev) for b in base]
    got = ops.msr_reference_frames([on_dev[j] for j in which], (3, 2), N)
    assert tuple(got.shape) == (N, 2, 3, 3)
    assert _first_bad(got.cpu().numpy().view(np.uint32), want7[which].view(np.uint32)) is None


def test_fused_chain_with_both_alignments_past_one_launch(ops, dev):
    """Grain batch size 3 and R = 4 reference frames together, 32772 frames of 2 x 2, no stencil, pass 2 recomputing the grain
    (cache_lab=False): launch_chain's launches hold whole noise chunks AND whole rounds of the reference (32760 frames, a multiple of 12).
    The oracle: the grain -> LUT image of the oracle, its Lab image by torch on the device, per-frame statistics in float64 rounded once
    (what the fp64 statistics are), the reference's apply formulas with frame f against reference frame f % 4; within CM_E2E_DEVICE_ULP, the
    budget of the fp64-statistics variant.  The Lab-caching form gives the same bits (test_fused_chain_with_colour_match)."""
    F, Rn, k = LAUNCH + 4, 4, 0.7
    assert F % 3 == 0 and F % Rn == 0
    data, dlut = _identity_lut(dev.index)
    x = _spread_frames(F, 5750)
    ref_ms = ops.reference_stats(_rand((Rn, 8, 8, 3), 5751).to(dev), cm_stats="fp64")
    y = _grain_lut_oracle(x, data, dev, 51)
    lab = _lab_nchw(y.to(dev))
    l64 = lab.double().reshape(F, 3, 4)
    ims = torch.stack([l64.mean(dim=2), l64.std(dim=2, unbiased=True) + float(np.float32(1e-5))], dim=-1).float()
    rep = ref_ms.repeat(F // Rn, 1, 1)
    want = R.color_match_apply(lab, ims[..., 0].reshape(F, 3, 1, 1), ims[..., 1].reshape(F, 3, 1, 1), rep[..., 0].reshape(F, 3, 1, 1),
                               rep[..., 1].reshape(F, 3, 1, 1), k).clamp(0, 1).permute(0, 2, 3, 1).contiguous()
    _differs_past_the_seam(want)
    spec = ops.ChainSpec(grain=GRAIN, lut=(dlut, 10.0), colormatch=(ref_ms, k), cm_stats="fp64")
    torch.manual_seed(51)
    plans = ops.plan_noise(F, 12, GRAIN[2], dev)
    assert plans[1] is None and plans[2] * 3 == F
    raw, out = _guarded(F, (2, 2, 3), torch.float32, dev)
    got = ops.fused_chain(x.to(dev), spec, plans=plans, out=out, cache_lab=False)
    assert _guards_intact(raw, out)
    d = (got.double() - want.double()).abs().reshape(F, -1).max(dim=1).values / ULP1
    print(f"fused chain, grain 3 and R = 4: max {float(d.max()):.2f} ulp(1.0) at frame {int(d.argmax())}")
    assert float(d.max()) <= CM_E2E_DEVICE_ULP, (float(d.max()), int(d.argmax()), int((d > CM_E2E_DEVICE_ULP).sum()))
    _same_bits(ops.fused_chain(x.to(dev), spec, plans=plans), got, "Lab-caching form")

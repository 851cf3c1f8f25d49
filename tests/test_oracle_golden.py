"""The CPU oracle (oracle/restated.py) against fixtures produced by the REFERENCE's own code
(oracle/make_golden.py): bit-for-bit."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import restated as R
from oracle import reference_loader as RL
from conftest import GOLDEN


def _npz(name):
    return np.load(os.path.join(GOLDEN, name))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_grain_noise_injected_cases():
    z = _npz("grain.npz")
    x = _t(z["x"])
    for tag in ("default", "strong_colour", "mono_all", "workflow_widgets"):
        I, s, bs = float(z[f"{tag}.I"]), float(z[f"{tag}.s"]), int(z[f"{tag}.bs"])
        noise = _t(z[f"{tag}.noise"])
        out = R.fast_film_grain(x, I, s, bs, noise_fn=lambda i, shape: noise[i:i + shape[0]])
        assert torch.equal(out, _t(z[f"{tag}.out"])), tag


def test_grain_cpu_generator_paths():
    z = _npz("grain.npz")
    x = _t(z["x"])
    assert torch.equal(R.film_grain_tensor(x, 0.04, 0.5, 7), _t(z["route_seed7.out"]))
    assert torch.equal(R.film_grain_tensor(x, 7.0, -3.0, 11), _t(z["route_clamped.out"]))
    fr = torch.full((4, 12, 16, 3), 0.5)
    out = R.seeded_grain(R.unsharp(fr, 0.5, False), 0.04, 0.5, 42, 100)
    assert torch.equal(out, _t(z["effects_batch.out"]))


def test_seeded_grain_is_batch_boundary_invariant():
    # the property the reference's own test pins (tests/test_standalone_video_enhancer.py:39-61)
    fr = torch.full((4, 12, 16, 3), 0.5)
    whole = R.seeded_grain(fr, 0.04, 0.5, 42, 100)
    split = torch.cat((R.seeded_grain(fr[:2], 0.04, 0.5, 42, 100), R.seeded_grain(fr[2:], 0.04, 0.5, 42, 102)))
    assert torch.equal(whole, split)


@pytest.mark.parametrize("tag,fname", [("a", "synthetic_17.cube"), ("b", "synthetic_domain_9.cube")])
def test_lut_parse_and_apply(tag, fname):
    z = _npz("lut.npz")
    lut = R.parse_cube_file(os.path.join(GOLDEN, fname))
    assert torch.equal(lut["lut"], _t(z[f"{tag}.lut"]))
    assert torch.equal(lut["domain_min"], _t(z[f"{tag}.dmin"]))
    assert torch.equal(lut["domain_max"], _t(z[f"{tag}.dmax"]))
    img, img4 = _t(z[f"{tag}.img"]), _t(z[f"{tag}.img4"])
    for s in (10.0, 3.3, 0.0, 25.0):
        assert torch.equal(R.apply_lut_with_strength(img, lut, s), _t(z[f"{tag}.out.s{s}"])), s
    assert torch.equal(R.apply_lut_with_strength(img4, lut, 10.0), _t(z[f"{tag}.out4.s10.0"]))
    assert torch.equal(R.apply_lut_with_strength(img, lut, 6.5), _t(z[f"{tag}.route.s6.5"]))


def test_cube_parser_errors(tmp_path):
    p = tmp_path / "bad1.cube"
    p.write_text("LUT_1D_SIZE 4\n0 0 0\n")
    with pytest.raises(ValueError):
        R.parse_cube_file(str(p))
    p.write_text("0 0 0\n")
    with pytest.raises(ValueError):
        R.parse_cube_file(str(p))
    p.write_text("LUT_3D_SIZE 2\n0 0 0\n")
    with pytest.raises(ValueError):
        R.parse_cube_file(str(p))


def test_stencils():
    z = _npz("stencil.npz")
    for tag in ("rand", "odd", "one", "row", "col", "c4", "const"):
        x = _t(z[f"{tag}.x"])
        for s in (0.5, 3.75):
            for gpu in (False, True):
                got = R.unsharp(x, s, gpu).contiguous()
                assert torch.equal(got, _t(z[f"{tag}.unsharp.{s}.{int(gpu)}"])), (tag, s, gpu)
        for gpu in (False, True):
            if gpu and x.shape[-1] != 3:
                continue
            assert torch.equal(R.laplacian(x, 0.8, gpu).contiguous(), _t(z[f"{tag}.laplacian.0.8.{int(gpu)}"])), (tag, gpu)
            assert torch.equal(R.sobel(x, 0.8, gpu).contiguous(), _t(z[f"{tag}.sobel.0.8.{int(gpu)}"])), (tag, gpu)
    x = _t(z["rand.x"])
    assert torch.equal(R.unsharp(x, 0.9, False), _t(z["enh.unsharp_cpu"]))
    assert torch.equal(R.unsharp(x, 0.9, True).contiguous(), _t(z["enh.unsharp_gpuflag"]))


def _unit_ulps(a, b):
    """largest distance in units of ulp(1.0) = 2^-23 of the [0, 1] outputs (north_star's "within 1 ulp fp32 per channel")"""
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / 2.0 ** -23) if a.size else 0.0


def test_zero_border_raster_restatement_matches_conv2d_to_an_ulp():
    """The explicit (kh, kw)-raster order the HIP kernels use against whatever order torch's conv2d took when the reference generated the
    fixtures (`use_gpu=True` run on the CPU: nodes.py:244-289, 324-384).  laplacian: BIT-EQUAL on every fixture (round 5 allowed 5e-7 =
    4 ulp(1.0): a regression of three ulp would have passed); sobel: within ONE ulp(1.0) (2 of 351 elements of `rand` differ, by exactly that)."""
    z = _npz("stencil.npz")
    for tag in ("rand", "odd", "one", "row", "col", "const"):
        x = _t(z[f"{tag}.x"])
        assert torch.equal(R.laplacian_zero_raster(x, 0.8), _t(z[f"{tag}.laplacian.0.8.1"])), tag
        assert _unit_ulps(R.sobel_zero_raster(x, 0.8).numpy(), z[f"{tag}.sobel.0.8.1"]) <= 1.0, tag


def test_zero_border_forms_on_a_1080p_frame_against_reference_rows():
    """tests/golden/stencil_1080p_rows.npz: twelve rows (the four border rows among them) of the reference's `use_gpu=True` unsharp / laplacian /
    sobel outputs for a seeded 1080p frame, produced by the reference itself on the CPU (oracle/make_golden.py).  unsharp (avg_pool2d) and
    laplacian (conv2d): bit-equal; sobel: 45 of 69,120 sampled elements differ, by at most one ulp(1.0) -- no summation
    order of the six taps (all 720 x 42 permutations x trees were tried) brings that to zero: the difference is not in the order."""
    z = _npz("stencil_1080p_rows.npz")
    g = torch.Generator().manual_seed(int(z["seed"]))
    x = torch.rand(tuple(int(v) for v in z["shape"]), generator=g) * float(z["affine"][0]) + float(z["affine"][1])
    rows = z["rows"]
    assert np.array_equal(R.unsharp(x, 0.5, True).contiguous().numpy()[0, rows], z["unsharp.0.5.1"])
    assert np.array_equal(R.laplacian_zero_raster(x, 0.8).numpy()[0, rows], z["laplacian.0.8.1"])
    sob = R.sobel_zero_raster(x, 0.8).numpy()[0, rows]
    assert _unit_ulps(sob, z["sobel.0.8.1"]) <= 1.0 and int((sob != z["sobel.0.8.1"]).sum()) <= 69


def test_colour_match_control_flow():
    z = _npz("colormatch.npz")
    x, ref1, ref4 = _t(z["x"]), _t(z["ref1"]), _t(z["ref4"])
    assert torch.equal(R.color_match(x, ref1, 1.0, 1), _t(z["out.ref1.k1.bs1"]))
    assert torch.equal(R.color_match(x, ref1, 0.35, 3), _t(z["out.ref1.k0.35.bs3"]))
    assert torch.equal(R.color_match(x, ref4, 0.8, 4), _t(z["out.ref4.k0.8.bs4"]))


def _lab_probe_images():
    """The colour-match probe set: video-like frames, the sRGB / Lab branch points and their float neighbours, 0, 1, tiny values."""
    g = torch.Generator().manual_seed(11)
    smooth = torch.rand(2, 3, 24, 32, generator=g)
    low = torch.rand(1, 3, 24, 32, generator=g) * 0.06                       # around the 0.04045 sRGB knee and the 0.008856 Lab knee
    specials = torch.tensor([0.0, 1.0, 0.04045, 0.040450003, 0.04044999, 0.0031308, 0.008856, 1e-6, 1e-3, 0.5, 0.999999, 0.2068966],
                            dtype=torch.float32)
    grid = torch.stack(torch.meshgrid(specials, specials, specials, indexing="ij"), 0).reshape(1, 3, 12 * 12, 12)
    return [smooth, low, grid]


@pytest.mark.skipif(RL.installed_kornia() is None, reason="kornia is not installed: the restated Lab transforms stay unpinned (DESIGN.md section 4)")
def test_restated_lab_equals_installed_kornia():
    """The pin of SURVEY.md section 8 row a8: wherever the reference's own dependency exists, the restated transforms are held to it
    bit for bit on the CPU -- forward, inverse (on in- and out-of-gamut Lab values) and through the reference's match_color."""
    kc, version = RL.installed_kornia()
    for img in _lab_probe_images():
        lab_k, lab_r = kc.rgb_to_lab(img), R.kornia_rgb_to_lab(img)
        assert torch.equal(lab_k, lab_r), f"rgb_to_lab: restatement vs kornia {version}"
        for scale in (1.0, 1.3):                                               # 1.3: pushes a / b out of gamut (negative linear RGB, clip)
            assert torch.equal(kc.lab_to_rgb(lab_k * scale), R.kornia_lab_to_rgb(lab_k * scale)), f"lab_to_rgb: restatement vs kornia {version}"
            assert torch.equal(kc.lab_to_rgb(lab_k * scale, clip=False), R.kornia_lab_to_rgb(lab_k * scale, clip=False))
    with open(os.path.join(GOLDEN, "provenance.json")) as fh:
        made_with = json.load(fh)["colormatch.npz"]["kornia.color"]
    if made_with.startswith("kornia"):                                         # fixtures regenerated on a box with kornia: they ARE kornia's
        test_colour_match_control_flow()


def test_golden_provenance_names_the_lab_source():
    with open(os.path.join(GOLDEN, "provenance.json")) as fh:
        src = json.load(fh)["colormatch.npz"]["kornia.color"]
    assert src.startswith("kornia ") or src.startswith("restated"), src


def test_lab_restated_self_consistency():
    # kornia is absent (parity unpinned): check the published algorithm's invariants instead
    g = torch.Generator().manual_seed(5)
    rgb = torch.rand(2, 3, 16, 16, generator=g)
    lab = R.kornia_rgb_to_lab(rgb)
    back = R.kornia_lab_to_rgb(lab)
    assert (back - rgb).abs().max() < 2e-5
    white = R.kornia_rgb_to_lab(torch.ones(1, 3, 1, 1))
    assert abs(white[0, 0, 0, 0].item() - 100.0) < 1e-3 and white[0, 1:].abs().max() < 1e-2
    assert R.kornia_rgb_to_lab(torch.zeros(1, 3, 1, 1)).abs().max() == 0


def test_shipped_lut_assets_by_digest(tmp_path):
    """The reference's 12 shipped cube files (tests/golden/reference_luts/, gzip of the files as shipped) against the recorded digests."""
    import gzip
    with open(os.path.join(GOLDEN, "shipped_lut_digests.json")) as fh:
        meta = json.load(fh)
    g = torch.Generator().manual_seed(meta["probe_seed"])
    probe = torch.rand(*meta["probe_shape"], generator=g) * meta["probe_affine"][0] + meta["probe_affine"][1]
    assert len(meta["luts"]) == 12
    for name, want in meta["luts"].items():
        path = tmp_path / name
        with gzip.open(os.path.join(GOLDEN, "reference_luts", name + ".gz"), "rb") as fh:
            path.write_bytes(fh.read())
        lut = R.parse_cube_file(str(path))
        assert lut["size"] == want["size"]
        assert hashlib.sha256(lut["lut"].numpy().tobytes()).hexdigest() == want["lut_sha256"], name
        out = R.apply_cube_lut(probe, lut["lut"], lut["domain_min"], lut["domain_max"])
        assert hashlib.sha256(out.numpy().tobytes()).hexdigest() == want["out_sha256"], name


def _reference_nodes():
    """tests/golden/reference_nodes.*: what the reference's node classes returned on these tests' seeded inputs (oracle/make_golden.py)."""
    with open(os.path.join(GOLDEN, "reference_nodes.json")) as fh:
        return _npz("reference_nodes.npz"), json.load(fh)


def test_restatement_against_live_reference_random_shapes():
    """The three sharpen nodes of the reference on random shapes, recorded from a live run of its node classes."""
    z, _ = _reference_nodes()
    for i in range(3):
        x = _t(z[f"sharpen{i}.x"])
        for s, gpu in ((0.5, False), (2.5, True)):
            assert torch.equal(R.unsharp(x, s, gpu).contiguous(), _t(z[f"sharpen{i}.unsharp.{s}.{int(gpu)}"])), (i, s, gpu)
            assert torch.equal(R.laplacian(x, s, gpu).contiguous(), _t(z[f"sharpen{i}.laplacian.{s}.{int(gpu)}"])), (i, s, gpu)
            assert torch.equal(R.sobel(x, s, gpu).contiguous(), _t(z[f"sharpen{i}.sobel.{s}.{int(gpu)}"])), (i, s, gpu)


# ------------------------------------------------------------------ 13-slider Adjust (section 8f rank 2)

def _adjust_cases():
    with open(os.path.join(GOLDEN, "adjust_cases.json")) as fh:
        return json.load(fh)


def test_adjust_restatement_against_reference_fixtures():
    z = _npz("adjust.npz")
    meta = _adjust_cases()
    for tag in meta["shapes"]:
        x = _t(z[f"{tag}.x"])
        for name, settings in meta["cases"].items():
            got = R.adjust_tensor(x, settings).contiguous().numpy()
            assert np.array_equal(got, z[f"{tag}.{name}"]), (tag, name)


def test_adjust_normalization_against_reference_fixture():
    with open(os.path.join(GOLDEN, "adjust_normalized.json")) as fh:
        want = json.load(fh)
    for name, settings in _adjust_cases()["cases"].items():
        assert R.normalize_adjust_settings(settings) == want[name], name
    assert R.normalize_adjust_settings("nope") == want["not_a_dict"]


# ------------------------------------------------------------------ uint8 codec edge (section 8f rank 3)

def test_u8_codec_edge_restatement_against_reference_fixtures():
    z = _npz("io_u8.npz")
    for tag in ("rand", "ramp"):
        assert np.array_equal(R.frames_to_tensor(list(z[f"{tag}.frames"])).numpy(), z[f"{tag}.tensor"]), tag
    for tag in ("tens", "edge"):
        assert np.array_equal(np.stack(R.tensor_to_frames(_t(z[f"{tag}.tensor"])), axis=0), z[f"{tag}.frames"]), tag
    frames = list(z["rand.frames"])
    lut = R.parse_cube_file(os.path.join(GOLDEN, "synthetic_17.cube"))
    for s in (10.0, 4.5):
        out = R.apply_lut_with_strength(R.frames_to_tensor(frames), lut, s)
        assert np.array_equal(np.stack(R.tensor_to_frames(out), axis=0), z[f"batch.lut.s{s}"]), s
    cases = _adjust_cases()["cases"]
    for name in ("all", "both", "fade_vig", "tone"):
        out = R.adjust_tensor(R.frames_to_tensor(frames), cases[name])
        assert np.array_equal(np.stack(R.tensor_to_frames(out), axis=0), z[f"batch.adjust.{name}"]), name


# ------------------------------------------------------------------ opening colour match (section 8f rank 4)

def _opening_meta():
    with open(os.path.join(GOLDEN, "opening_match.json")) as fh:
        return json.load(fh)


def test_opening_match_restatement_against_reference_fixtures():
    """Statistics (PIL.ImageStat), gains / offsets, the cube text and the blend weight: fixtures come from the
    reference's own statements (oracle/reference_loader.py::opening_color_match_reference)."""
    z = _npz("opening_match.npz")
    for name, m in _opening_meta().items():
        rs, ts = R.image_stat_rgb(z[f"{name}.ref"]), R.image_stat_rgb(z[f"{name}.tgt"])
        assert rs[0] == m["reference_mean"] and ts[0] == m["target_mean"], name
        assert [max(1.0, v) for v in rs[1]] == m["reference_std"] and [max(1.0, v) for v in ts[1]] == m["target_std"], name
        scales, offsets = R.opening_match_terms(rs, ts)
        assert scales == m["scales"] and offsets == m["offsets"], name
        text = R.opening_match_cube_text(scales, offsets)
        assert hashlib.sha256(text.encode()).hexdigest() == m["cube_sha256"], name
        assert text.splitlines()[:6] == m["cube_head"] and text.splitlines()[-2:] == m["cube_tail"]
        # the weight expression the reference formats for ffmpeg, evaluated at a few times
        s6, f6 = m["weight"].split("*(1-T/")[0].split("\\,")[-1], m["weight"].split("*(1-T/")[1].rstrip(")")
        for k in (0, 1, 7, 24, 500):
            want = max(0.0, min(1.0, float(s6) * (1.0 - (k / 24.0) / float(f6))))
            assert R.opening_match_weight(k, 24.0, m["strength"], m["fade_seconds"]) == want, (name, k)


def test_opening_match_against_live_reference():
    """The reference's opening colour match (strength 0.5, fade 3 s) on a seeded pair of frames, recorded from a live run of its statements:
    scales and offsets exactly, the cube text by SHA-256."""
    z, meta = _reference_nodes()
    out = meta["opening"]
    scales, offsets = R.opening_match_terms(R.image_stat_rgb(z["opening.ref"]), R.image_stat_rgb(z["opening.tgt"]))
    assert scales == out["scales"] and offsets == out["offsets"]
    assert hashlib.sha256(R.opening_match_cube_text(scales, offsets).encode()).hexdigest() == out["cube_sha256"]


def test_lab_restatement_known_answers_from_colour_science():
    """kornia is absent (colour match stays "parity unpinned"), so the restated transforms are anchored on published
    CIELAB (D65, 2 deg) values of the sRGB primaries / secondaries -- the algorithm, not the last bit (kornia's 6-digit
    ITU matrix moves them by ~1e-3)."""
    known = {
        (1.0, 0.0, 0.0): (53.2408, 80.0925, 67.2032),
        (0.0, 1.0, 0.0): (87.7347, -86.1827, 83.1793),
        (0.0, 0.0, 1.0): (32.2970, 79.1875, -107.8602),
        (1.0, 1.0, 0.0): (97.1393, -21.5537, 94.4780),
        (0.0, 1.0, 1.0): (91.1132, -48.0875, -14.1312),
        (1.0, 0.0, 1.0): (60.3242, 98.2343, -60.8249),
        (1.0, 1.0, 1.0): (100.0, 0.0, 0.0),
        (128 / 255.0,) * 3: (53.5850, 0.0, 0.0),
        (0.0, 0.0, 0.0): (0.0, 0.0, 0.0),
    }
    rgb = torch.tensor(list(known.keys()), dtype=torch.float32).t().reshape(1, 3, 1, -1)
    lab = R.kornia_rgb_to_lab(rgb).reshape(3, -1).t()
    want = torch.tensor(list(known.values()), dtype=torch.float32)
    assert (lab - want).abs().max().item() < 0.05, (lab - want).abs().max().item()
    back = R.kornia_lab_to_rgb(R.kornia_rgb_to_lab(rgb))
    assert (back - rgb).abs().max().item() < 1e-5


def test_baseline_config_1_oracle_equals_reference_node_on_cpu():
    """BASELINE.json configs[0] on the reference's own CPU path: same seed, same mt19937 noise -> the restatement and the
    reference node agree bit for bit on the 512x512 frame (the node's output recorded by the SHA-256 of its fp32 bytes)."""
    _, meta = _reference_nodes()
    torch.manual_seed(0)
    x = torch.rand(1, 512, 512, 3)
    assert hashlib.sha256(x.numpy().tobytes()).hexdigest() == meta["grain_512"]["input_sha256"]
    torch.manual_seed(1)
    got = R.fast_film_grain(x, 0.04, 0.5, 4)
    assert hashlib.sha256(got.contiguous().numpy().tobytes()).hexdigest() == meta["grain_512"]["out_sha256"]


def test_ffmpeg_style_lut3d_restatement_properties():
    """oracle.restated.ffmpeg_lut3d_blend_u8 is restated from ffmpeg's published sources with nothing here to pin it to
    (parity unpinned).  What can be checked without ffmpeg: grid nodes return the node value (truncated to 8 bits), an affine
    cube interpolates exactly like the trilinear node arithmetic up to the 8-bit rule, weights 0 / 1 select source / result."""
    n = 17
    ax = torch.linspace(0, 1, n, dtype=torch.float64)
    b, g, r = torch.meshgrid(ax, ax, ax, indexing="ij")
    affine = torch.stack([(0.9 * r + 0.02), (0.5 * g + 0.1), (1.0 * b)], -1).to(torch.float32).clamp(0, 1)
    data = {"size": n, "lut": affine, "domain_min": torch.zeros(3), "domain_max": torch.ones(3)}
    gen = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (2, 32, 32, 3), generator=gen, dtype=torch.uint8).numpy()
    out = R.ffmpeg_lut3d_blend_u8(frames, data)
    tri = R.tensor_to_frames(R.apply_lut_with_strength(R.frames_to_tensor(list(frames)), data, 10.0))
    assert np.abs(out.astype(np.int32) - np.stack(tri, 0).astype(np.int32)).max() <= 1
    # byte 255 * k / 16 is a grid node only for k = 0, 16 at 8 bits: check the two ends and the clamp of an out-of-range table
    ends = np.array([[[[0, 0, 0], [255, 255, 255]]]], dtype=np.uint8)
    rnd = {"size": n, "lut": torch.rand((n, n, n, 3), generator=gen) * 1.4 - 0.2, "domain_min": torch.zeros(3), "domain_max": torch.ones(3)}
    got = R.ffmpeg_lut3d_blend_u8(ends, rnd)
    for px, node in ((got[0, 0, 0], rnd["lut"][0, 0, 0]), (got[0, 0, 1], rnd["lut"][n - 1, n - 1, n - 1])):
        want = np.clip((node.numpy() * np.float32(255.0)).astype(np.int32), 0, 255)[::-1]          # B, G, R bytes
        assert np.array_equal(px, want.astype(np.uint8))
    assert np.array_equal(R.ffmpeg_lut3d_blend_u8(frames, rnd, [0.0, 0.0]), frames)
    assert np.array_equal(R.ffmpeg_lut3d_blend_u8(frames, rnd, [1.0, 1.0]), R.ffmpeg_lut3d_blend_u8(frames, rnd))

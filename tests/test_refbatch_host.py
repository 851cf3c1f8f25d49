"""The multi-reference image batches without a GPU: csrc/vrg_refbatch_math.hpp compiled for the host against torch itself (run live, plain
CPU kernels), numpy and live Pillow, driven by the package's own planning; sizes, surfaces, path forms and error texts against the
fixture recorded from the reference's classes; the host check's refusals, the ABI, and the node module's data flow."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import refbatch_support as S
from conftest import PKG_NAME, ROOT
from test_facefix_packed_host import SEARCH_COUNTS

NEW_SYMBOLS = ("vrg_refbatch_check", "vrg_refbatch_f32", "vrg_refbatch_quantise_u8")


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext, ops
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return ops


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return S.build_host_lib(tmp_path_factory.mktemp("refbatch_host"))


@pytest.fixture(scope="module")
def truth(tmp_path_factory):
    return S.torch_results(S.CASES, tmp_path_factory.mktemp("refbatch_torch"))


@pytest.fixture()
def node(pkg):
    return importlib.import_module(PKG_NAME + ".VRGDG_MultiReference")


def _index(name):
    return next(i for i, c in enumerate(S.CASES) if c["name"] == name)


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=[c["name"] for c in S.CASES])
def test_header_equals_torch(ops, host, truth, monkeypatch, i):
    """every picture of every case bit for bit (NaN by position), one launch a call, the inputs untouched"""
    c = S.CASES[i]
    pictures = truth.inputs(i)
    before = [p.clone() for p in pictures]
    with S.on_host(monkeypatch, ops, host) as launches:
        got = S.run_case(ops, pictures, c)
    assert len(launches) == 1
    want = truth.pictures(i)
    assert [tuple(g.shape) for g in got] == [w.shape for w in want]
    for g, w in zip(got, want):
        assert S.same_bits(g.numpy(), w) == 0, (c["name"], truth.describe())
    assert all(S.same_bits(a.numpy(), b.numpy()) == 0 for a, b in zip(pictures, before))


def test_the_cases_reach_what_they_are_for(ops, truth):
    # not clamped: torch's own bicubic result leaves [0, 1] on both sides
    want = np.concatenate([w.reshape(-1) for w in truth.pictures(_index("ragged-bicubic-0.008"))])
    assert (want < 0).any() and (want > 1).any()
    # equal sizes: the filter is evaluated -- an Inf becomes NaN under bilinear, its neighbours under bicubic
    pictures = truth.inputs(_index("equal-bilinear"))
    for method, spreads in (("bilinear", False), ("bicubic", True), ("nearest-exact", None), ("area", None)):
        i = _index(f"equal-{method}")
        for src, out in zip(pictures, truth.pictures(i)):
            assert src.shape == out.shape
            src = src.numpy()
            if spreads is None:      # a window of one pixel: the values themselves (0.0f + -0.0 loses the sign under area, in torch too)
                assert S.same_bits(out, src) == 0 if method == "nearest-exact" else np.array_equal(out, src, equal_nan=True)
                continue
            special = np.isnan(src) | np.isinf(src)
            if spreads:             # Inf * 1 + neighbour * 0 stays Inf, and every pixel whose taps reach it is NaN
                assert np.isnan(out).sum() > special.sum() and np.isnan(out[np.isnan(src)]).all()
            else:                   # x * 1 + x * 0: NaN exactly where the source is Inf or NaN
                assert np.array_equal(np.isnan(out), special) and np.isinf(src).sum() >= 4
    # the kernel-choice cases lie on both sides of the sum, and on both sides of "contiguous"
    sums = {c["name"]: c["shapes"][0][1] + c["shapes"][0][2] for c in S.KERNEL_CASES if c["kind"] == "batch"}
    assert sums["sum-128"] == 128 and sums["sum-129"] == 129
    # copy: the fitting picture of the batch rule arrives bit for bit, specials included, next to a channel of 1.0
    i = _index("rule-bicubic")
    src, out = truth.inputs(i)[3].numpy(), truth.pictures(i)[0]
    assert out.shape == (4, 20, 37, 4) and S.same_bits(out[3][..., :3], src[0]) == 0 and (out[3][..., 3] == 1).all()
    assert (out[0][..., 3] == 1).all() and (src == np.float32(1e-40)).any() and np.isinf(src).any() and np.isnan(src).any()
    assert np.signbit(src[src == 0]).any()


def test_half_pair_lands_on_a_half(ops):
    old_w, old_h, new_w, new_h = S.HALF_PAIR
    half = (old_w - old_w * ((new_w / new_h) / (old_w / old_h))) / 2
    assert half == 2.5 and round(half) == 2
    assert ops.center_crop_rect(*S.HALF_PAIR) == (2, 0, 5, 4)
    c = S.CASES[_index("half-rect-bilinear")]
    assert (c["shapes"][1][2], c["shapes"][1][1], c["shapes"][0][2], c["shapes"][0][1]) == S.HALF_PAIR


def test_sizes_equal_the_fixture(ops):
    assert len(S.FIXTURE["sizes"]) >= 20
    for rec in S.FIXTURE["sizes"]:
        assert list(ops.total_pixels_size(rec["height"], rec["width"], rec["megapixels"], rec["resolution_steps"])) == rec["result"], rec
    for (h, w), mp, steps, want in (((1080, 1920), 1.0, 1, (768, 1365)), ((333, 517), 0.25, 8, (408, 640)), ((7, 5), 0.01, 1, (121, 87)),
                                    ((4000, 3000), 16.0, 64, (4736, 3520))):
        assert ops.total_pixels_size(h, w, mp, steps) == want
    assert ops.total_pixels_size(16, 16, S.EQUAL_MP, 1) == (16, 16)
    for mp, steps in S.BUDGETS:
        assert all(max(ops.total_pixels_size(s[1], s[2], mp, steps)) <= 160 for s in S.RAGGED)
    with pytest.raises(ValueError):
        ops.total_pixels_size(0, 4, 1.0, 1)


def test_quantise_and_bytes_equal_numpy(ops, host, monkeypatch):
    """np.clip(255. * x, 0, 255).astype(np.uint8) for every finite class of x (NaN -> 0 is this project's choice), and byte / 255.0"""
    grid = np.arange(256, dtype=np.float32) / np.float32(255.0)
    values = np.concatenate([grid, np.nextafter(grid, np.float32(2)), np.nextafter(grid, np.float32(-2)),
                             np.array([-0.0, 1e-40, -1e-40, -0.1, 1.1, 300.0, -300.0, np.inf, -np.inf, 0.999999, 1.0000001], dtype=np.float32),
                             np.random.default_rng(5).uniform(-0.1, 1.1, 1249).astype(np.float32)])
    values = values[:values.size // 12 * 12]
    x = torch.from_numpy(values.reshape(1, -1, 4, 3).copy())
    h, w = int(x.shape[1]), 4
    out = torch.zeros(x.numel() + 5, dtype=torch.uint8)
    with S.on_host(monkeypatch, ops, host):
        job = ops._RefJob(x, 0, (h, w, 3), (0, 0, w, h), 3, (h, w, 3), 4, 1)
        ops._refbatch_launch(torch.device("cpu"), [job], out)
        want = np.clip(255. * x.numpy(), 0, 255).astype(np.uint8).reshape(-1)
        assert np.array_equal(out.numpy()[3:3 + x.numel()], want) and not out[:3].any() and not out[3 + x.numel():].any()
        nan = torch.full((1, 1, 4, 3), float("nan"))
        q = torch.full((12,), 9, dtype=torch.uint8)
        ops._refbatch_launch(torch.device("cpu"), [ops._RefJob(nan, 0, (1, 4, 3), (0, 0, 4, 1), 0, (1, 4, 3), 4, 1)], q)
        assert not q.any()
        ramp = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3).astype(np.uint8)
        got = ops.reference_bytes_to_images([ramp, ramp[:5, :7]])
    assert [tuple(g.shape) for g in got] == [(1, 16, 16, 3), (1, 5, 7, 3)]
    for g, src in zip(got, (ramp, ramp[:5, :7])):
        assert S.same_bits(g.numpy()[0], src.astype(np.float32) / 255.0) == 0


class _PillowPlan:
    """stands in for far_face_repair.ResizePlan (vrg_pil_resize_u8, a GPU kernel held to Pillow by tests/test_gpu_far_face.py): live Pillow"""

    def __init__(self, src, src_offsets, sizes, channels, device):
        from PIL import Image
        assert channels == 3
        parts, self.offsets, at = [], [], 0
        for off, (iw, ih, ow, oh) in zip(src_offsets, sizes):
            image = Image.fromarray(src[off:off + ih * iw * 3].numpy().reshape(ih, iw, 3))
            parts.append(torch.from_numpy(np.array(image.resize((ow, oh), resample=Image.Resampling.LANCZOS)).reshape(-1)))
            self.offsets.append(at)
            at += ow * oh * 3
        self.dst = torch.cat(parts)

    def run(self):
        return self.dst


def test_lanczos_path_equals_pillow(ops, host, monkeypatch):
    """quantise -> Pillow's LANCZOS -> bytes / 255 as comfy does it, finite inputs; scale and the batch rule (centre crop before the bytes)"""
    pytest.importorskip("PIL")
    from comfyui_vrgamedevgirl_amd import far_face_repair
    monkeypatch.setattr(far_face_repair, "ResizePlan", _PillowPlan)
    c = S.scale_case("lanczos", ((1, 20, 37, 3), (2, 33, 29, 3)), "lanczos", 0.0005, seed=9)
    pictures = S.ref_pictures(c)
    sizes = [ops.total_pixels_size(p.shape[1], p.shape[2], c["megapixels"], c["steps"]) for p in pictures]
    with S.on_host(monkeypatch, ops, host) as launches:
        got = ops.scale_reference_images(pictures, "lanczos", c["megapixels"], c["steps"])
        assert len(launches) == 2                       # the quantise launch and the bytes launch
        batch = ops.batch_reference_images(pictures, "lanczos")
    for g, w in zip(got, S.pil_lanczos(pictures, sizes)):
        assert S.same_bits(g.numpy(), w) == 0
    x, y, w, h = ops.center_crop_rect(29, 33, 37, 20)
    want = S.pil_lanczos([pictures[1][:, y:y + h, x:x + w]], [(20, 37)])[0]
    assert tuple(batch.shape) == (3, 20, 37, 3) and S.same_bits(batch[:1].numpy(), pictures[0].numpy()) == 0
    assert S.same_bits(batch[1:].numpy(), want) == 0


def test_operator_refusals(ops, host, monkeypatch):
    rgb, rgba = torch.rand(1, 4, 6, 3), torch.rand(1, 5, 3, 4)
    with S.on_host(monkeypatch, ops, host):
        for call in (lambda: ops.scale_reference_images([rgb], "bislerp"), lambda: ops.batch_reference_images([rgb, rgba], "nearest"),
                     lambda: ops.scale_reference_images([rgb[0]]), lambda: ops.scale_reference_images(rgb),
                     lambda: ops.scale_reference_images([rgb.double()]), lambda: ops.scale_reference_images([torch.rand(1, 4, 6, 2)]),
                     lambda: ops.scale_reference_images([torch.rand(1, 0, 6, 3)]), lambda: ops.batch_reference_images([]),
                     lambda: ops.batch_reference_images([rgb, rgb, rgba])):
            with pytest.raises(ValueError):
                call()
        for call in (lambda: ops.scale_reference_images([rgb, rgba], "lanczos"), lambda: ops.batch_reference_images([rgb, rgba], "lanczos")):
            with pytest.raises(NotImplementedError, match="3-channel"):
                call()
        assert ops.batch_reference_images([rgba], "lanczos") is rgba                       # a single picture is returned as it is
        same = ops.batch_reference_images([rgba, rgba + 1], "lanczos")                     # nothing to resize: lanczos is never reached
        assert S.same_bits(same.numpy(), torch.cat([rgba, rgba + 1]).numpy()) == 0
    assert ops.batch_channels([3, 4, 3, 4]) == 4 and ops.batch_channels([4, 3, 3]) == 4 and ops.batch_channels([3, 3]) == 3
    assert list(ops.REFBATCH_METHODS) == S.FIXTURE["upscale_methods"] == list(S.METHODS)


def test_abi_and_check_refusals(ops):
    """the three names are declared, exported and bound, the ABI version stays 8, and vrg_refbatch_check refuses without a device"""
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    header = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in _hip.EXPORTED_SYMBOLS and hasattr(lib._cdll, name)
    assert lib.vrg_abi_version() == 8 and "#define VRG_ABI_VERSION 8" in header
    assert f"#define VRG_REFBATCH_TILE {S.TILE}" in header and _hip.REFBATCH_TILE == S.TILE
    assert "vrg_refbatch_math.hpp" in build_ext.HEADERS and "vrg_refbatch.hip" in build_ext.SOURCES
    assert C.sizeof(_hip.RefbatchDesc) == ops.REFBATCH_DESC.itemsize == 72

    def check(records, src_floats=10 ** 6, src_bytes=10 ** 6, out=10 ** 6, tiles=True):
        desc = np.zeros(len(records), dtype=ops.REFBATCH_DESC)
        at = 0
        for k, r in enumerate(records):
            rec = dict(src_offset=0, dst_offset=0, src_h=7, src_w=5, src_c=3, src_x0=0, src_y0=0, src_rw=5, src_rh=7, dst_h=9, dst_w=11, dst_c=3,
                       method=1, frames=1, first_tile=at if tiles else 0, reserved=0)
            rec.update(r)
            desc[k] = tuple(rec[n] for n in ops.REFBATCH_DESC.names)
            at += rec["frames"] * -(-rec["dst_h"] * rec["dst_w"] * rec["dst_c"] // S.TILE)
        return lib.vrg_refbatch_check(C.c_void_p(desc.ctypes.data), len(records), src_floats, src_bytes, out)

    assert check([]) == 0 and check([{}]) == 0 and check([{}, {"dst_offset": 297}]) == 0
    assert check([{"dst_c": 4}, {"dst_offset": 396, "frames": 0}, {"dst_offset": 396, "method": 0}]) == 0
    assert check([{"method": 4, "dst_h": 7, "dst_w": 5}, {"method": 5, "dst_h": 7, "dst_w": 5, "dst_offset": 105}]) == 0
    for bad in ({"src_h": 0}, {"src_w": 0}, {"dst_h": 0}, {"dst_w": 0}, {"frames": -1}, {"src_offset": -1}, {"dst_offset": -1},
                {"src_c": 2}, {"src_c": 5}, {"dst_c": 5}, {"src_c": 4, "dst_c": 3},
                {"src_x0": 1}, {"src_y0": 1}, {"src_x0": -1}, {"src_rw": 0}, {"src_rh": 0}, {"src_rw": 6}, {"src_x0": 2 ** 31 - 1},
                {"method": 6}, {"method": -1}, {"method": 4}, {"method": 5, "dst_h": 7},
                {"src_offset": 10 ** 6 - 104}, {"dst_offset": 10 ** 6 - 296}, {"frames": 2 ** 20}):
        assert check([bad]) == 1, bad
    assert check([{}, {"dst_offset": 296}]) == 1 and check([{"dst_offset": 5}, {"dst_offset": 0, "frames": 2}]) == 1          # overlapping outputs
    assert check([{}, {"dst_offset": 297}], tiles=False) == 1                                 # first_tile is not the running sum
    assert check([{"method": 5}], src_bytes=104) == 1 and check([{"method": 5, "dst_h": 7, "dst_w": 5}], src_bytes=105, src_floats=0) == 0
    big = 2 ** 40
    assert check([{"src_h": 46341, "src_w": 46341, "src_rw": 46341, "src_rh": 46341}], src_floats=big) == 2
    assert check([{"dst_h": 46341, "dst_w": 46341}], out=big) == 2
    assert check([{"method": 2, "src_h": 4000, "src_w": 3000, "src_rw": 3000, "src_rh": 4000, "dst_h": 1, "dst_w": 1}], src_floats=big) == 2
    assert check([{"method": 2, "src_h": 4000, "src_w": 3000, "src_rw": 3000, "src_rh": 4000, "dst_h": 100, "dst_w": 100}], src_floats=big) == 0
    assert check([{"dst_h": 20000, "dst_w": 20000, "frames": 2000}], out=2 ** 50) == 2                                       # tiles past 2^31 - 1
    null, one, two, three = (C.c_void_p(v) for v in (0, 16, 32, 48))                                                       # never dereferenced
    assert lib.vrg_refbatch_f32(null, 0, null, 0, null, 0, 0, null, 0, null) == 0
    assert lib.vrg_refbatch_f32(one, 8, null, 0, two, 1, 0, three, 8, null) == 0
    for args in ((one, 8, null, 0, null, 1, 1, three, 8), (one, 8, null, 0, two, 1, 1, null, 8), (null, 8, null, 0, two, 1, 1, three, 8),
                 (null, 0, null, 0, two, 1, 1, three, 8), (one, 8, null, 0, two, 1, 1, one, 8), (one, 8, null, 0, two, -1, 1, three, 8),
                 (C.c_void_p(18), 8, null, 0, two, 1, 1, three, 8), (one, 8, null, 0, C.c_void_p(36), 1, 1, three, 8)):
        assert lib.vrg_refbatch_f32(*args, null) == 1, args
    assert lib.vrg_refbatch_f32(one, 8, null, 0, two, 1, 2 ** 31, three, 8, null) == 2
    assert lib.vrg_refbatch_quantise_u8(null, 0, null, 0, 0, null, 0, null) == 0
    assert lib.vrg_refbatch_quantise_u8(null, 8, two, 1, 1, three, 8, null) == 1 and lib.vrg_refbatch_quantise_u8(one, 8, two, 1, 1, null, 8, null) == 1


@pytest.mark.parametrize("counts", SEARCH_COUNTS)
def test_search_finds_first_and_last_tile_of_every_record(ops, host, counts):
    """rb_find as the kernels of csrc/vrg_refbatch.hip call it -- tile_owner of csrc/vrg_packed_tiles.hpp through the first_tile of the
    records -- on the tile-count lists of the packed routes' search: counts of 0 repeat a first_tile in front, in the middle, at the end"""
    host.hm_rb_find.argtypes, host.hm_rb_find.restype = [C.c_void_p, C.c_int64, C.c_int32], C.c_int64
    n, first = len(counts), np.concatenate([[0], np.cumsum(counts)])
    desc = np.zeros(n, dtype=ops.REFBATCH_DESC)
    desc["first_tile"] = first[:-1]

    def find(tile):
        return host.hm_rb_find(desc.ctypes.data, n, tile)

    for rec, count in enumerate(counts):
        if count:
            assert find(int(first[rec])) == rec == find(int(first[rec]) + count - 1), (counts[:8], rec)
    for tile in range(min(int(first[-1]), 64)):                              # every tile has the owner a linear walk finds
        assert find(tile) == max(i for i in range(n) if first[i] <= tile and counts[i] > 0)
    assert 0 <= find(int(first[-1]) + 5) < n                                 # a tile past the grid still names a record of the table


def test_surfaces_paths_and_errors_equal_the_fixture(node, pkg):
    assert set(node.NODE_CLASS_MAPPINGS) == set(S.FIXTURE["surface"]) == set(node.NODE_DISPLAY_NAME_MAPPINGS)
    for name, want in S.FIXTURE["surface"].items():
        cls = node.NODE_CLASS_MAPPINGS[name]
        assert json.loads(json.dumps(cls.INPUT_TYPES())) == want["INPUT_TYPES"], name
        for group in want["INPUT_TYPES"]:
            assert list(cls.INPUT_TYPES()[group]) == list(want["INPUT_TYPES"][group])
        assert [list(cls.RETURN_TYPES), list(cls.RETURN_NAMES), cls.FUNCTION, cls.CATEGORY, cls.DESCRIPTION] == \
            [want["RETURN_TYPES"], want["RETURN_NAMES"], want["FUNCTION"], want["CATEGORY"], want["DESCRIPTION"]], name
        assert node.NODE_DISPLAY_NAME_MAPPINGS[name] == want["display_name"]
        assert name not in pkg.NODE_CLASS_MAPPINGS and name not in pkg.NODE_DISPLAY_NAME_MAPPINGS           # the package's pinned set
    multi = node.VRGDG_MultiReferenceConditioning
    assert multi.MAX_IMAGES == S.FIXTURE["max_images"] == len(multi.INPUT_TYPES()["optional"]) and multi.upscale_methods == S.FIXTURE["upscale_methods"]
    for rec in S.FIXTURE["paths"]:
        assert node._parse_image_paths(rec["input"]) == rec["result"], rec
        assert node.VRGDG_MultiReferenceConditioningFromPaths._parse_image_paths(rec["input"]) == rec["result"]


def test_error_texts_equal_the_fixture(node, monkeypatch, tmp_path):
    errors = S.FIXTURE["errors"]
    monkeypatch.setattr(node, "path_roots", lambda: [str(tmp_path / "input"), str(tmp_path / "output")])
    monkeypatch.chdir(tmp_path)
    vae = types.SimpleNamespace(encode=lambda x: x)
    for name, call in (("no_images", lambda: node.VRGDG_MultiReferenceConditioning().apply("P", "N", vae, 4, "bilinear", 1.0, 1)),
                       ("no_paths", lambda: node.VRGDG_MultiReferenceConditioningFromPaths().apply("P", "N", vae, "", "bilinear", 1.0, 1)),
                       ("no_batch_paths", lambda: node.VRGDG_ImageBatchMultiFromPaths().load_batch("  ", "bilinear")),
                       ("empty_path", lambda: node._resolve_image_path(" '' ")),
                       ("missing_path", lambda: node._resolve_image_path("no-such-picture.png"))):
        kind = {"ValueError": ValueError, "FileNotFoundError": FileNotFoundError}[errors[name]["type"]]
        with pytest.raises(kind) as caught:
            call()
        assert str(caught.value) == errors[name]["message"], name
    # a relative path is found in the working directory first, then in the roots, in their order
    (tmp_path / "output").mkdir()
    (tmp_path / "output" / "b.png").write_bytes(b"x")
    assert node._resolve_image_path("'b.png'") == str(tmp_path / "output" / "b.png")
    (tmp_path / "b.png").write_bytes(b"x")
    assert node._resolve_image_path("b.png") == str(tmp_path / "b.png")
    assert node._resolve_image_path(str(tmp_path / "output" / "b.png")) == str(tmp_path / "output" / "b.png")


def test_module_imports_without_comfyui(pkg):
    code = ("import sys; sys.path.insert(0, %r); import conftest; conftest.load_package(); import importlib; "
            "m = importlib.import_module(conftest.PKG_NAME + '.VRGDG_MultiReference'); "
            "assert not [n for n in sys.modules if n.split('.')[0] in ('comfy', 'comfy_extras', 'folder_paths', 'node_helpers')]; "
            "assert len(m.NODE_CLASS_MAPPINGS) == 3 and callable(m.conditioning_appender) and callable(m.image_loader) "
            "and callable(m.path_roots)") % os.path.join(ROOT, "tests")
    ran = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stderr


class Fakes:
    """a recording vae and appender, as the fixture's recorder stood in for ComfyUI's"""

    def __init__(self):
        self.encoded, self.appended = [], []

    def encode(self, pixels):
        self.encoded.append(pixels)
        return torch.zeros(1, 16, pixels.shape[1] // 8, pixels.shape[2] // 8)

    def append(self, conditioning, latent):
        self.appended.append({"to": conditioning, "shapes": [list(latent["samples"].shape)]})
        return conditioning + "+"


def test_node_data_flow_equals_the_fixture(node, ops, host, monkeypatch):
    """the order of the encode calls, the shapes of what is encoded and appended, the returns and the batch, as recorded from the
    reference's class; the pictures themselves against the package's own functions.  No GPU: the launch is the host-compiled header."""
    want = S.FIXTURE["flow"]
    fakes = Fakes()
    monkeypatch.setattr(node, "conditioning_appender", fakes.append)
    images = {k: torch.rand(*shape) for k, shape in want["inputs"].items()}
    with S.on_host(monkeypatch, ops, host):
        pos, neg, batch = node.VRGDG_MultiReferenceConditioning().apply("P", "N", fakes, want["image_count"], "bilinear", want["megapixels"],
                                                                        want["resolution_steps"], **images)
        scaled = ops.scale_reference_images([images["image1"], images["image3"]], "bilinear", want["megapixels"], want["resolution_steps"])
        joined = ops.batch_reference_images(scaled, "bilinear")
    assert [pos, neg] == want["returns"] and list(batch.shape) == want["batch_shape"]
    assert [list(e.shape) for e in fakes.encoded] == want["encoded"]
    assert [(a["to"], a["shapes"]) for a in fakes.appended] == [(a["to"], a["shapes"]) for a in want["appended"]]
    assert all(S.same_bits(e.numpy(), s.numpy()) == 0 for e, s in zip(fakes.encoded, scaled)) and S.same_bits(batch.numpy(), joined.numpy()) == 0


def test_path_nodes_with_a_fake_loader(node, ops, host, monkeypatch, tmp_path):
    fakes = Fakes()
    rng = np.random.default_rng(3)
    files = {"a.png": rng.integers(0, 256, (20, 37, 3), dtype=np.uint8), "b.png": rng.integers(0, 256, (33, 29, 3), dtype=np.uint8)}
    for name in files:
        (tmp_path / name).write_bytes(b"x")
    monkeypatch.setattr(node, "path_roots", lambda: [str(tmp_path)])
    monkeypatch.setattr(node, "image_loader", lambda path: files[os.path.basename(path)])
    monkeypatch.setattr(node, "conditioning_appender", fakes.append)
    pictures = [torch.from_numpy(files[n].astype(np.float32) / 255.0).unsqueeze(0) for n in ("a.png", "b.png")]
    with S.on_host(monkeypatch, ops, host):
        (batch,) = node.VRGDG_ImageBatchMultiFromPaths().load_batch('["a.png", "b.png"]', "bicubic")
        want = ops.batch_reference_images(pictures, "bicubic")
        pos, neg, out = node.VRGDG_MultiReferenceConditioningFromPaths().apply("P", "N", fakes, "a.png\nb.png", "area", 0.0005, 4)
        scaled = ops.scale_reference_images(pictures, "area", 0.0005, 4)
        (single,) = node.VRGDG_ImageBatchMultiFromPaths().load_batch("b.png", "bilinear")
    assert tuple(batch.shape) == (2, 20, 37, 3) and S.same_bits(batch.numpy(), want.numpy()) == 0
    assert (pos, neg) == ("P++", "N++") and [tuple(e.shape) for e in fakes.encoded] == [tuple(s.shape) for s in scaled]
    assert all(S.same_bits(e.numpy(), s.numpy()) == 0 for e, s in zip(fakes.encoded, scaled))
    assert tuple(out.shape) == (2, *scaled[0].shape[1:]) and S.same_bits(single.numpy(), pictures[1].numpy()) == 0


def test_restatement_equals_comfy(ops, host, monkeypatch):
    """unpinned unless ComfyUI is installed: the real comfy.utils.common_upscale, every method, crop disabled and centre"""
    comfy_utils = pytest.importorskip("comfy.utils")
    pytest.importorskip("PIL")
    from comfyui_vrgamedevgirl_amd import far_face_repair
    monkeypatch.setattr(far_face_repair, "ResizePlan", _PillowPlan)
    base, other = (t.clamp(0, 1) for t in S.ref_pictures(S.batch_case("comfy", ((1, 20, 37, 3), (1, 33, 29, 3)), "bilinear", seed=11)))
    for method in S.METHODS:
        with S.on_host(monkeypatch, ops, host):
            got = ops.batch_reference_images([base, other], method)[1:]
            (scaled,) = ops.scale_reference_images([other], method, 0.0005, 4)
        want = comfy_utils.common_upscale(other.movedim(-1, 1), 37, 20, method, "center").movedim(1, -1)
        assert torch.allclose(got, want, atol=2e-6, rtol=0), method
        h, w = ops.total_pixels_size(33, 29, 0.0005, 4)
        want = comfy_utils.common_upscale(other.movedim(-1, 1), w, h, method, "disabled").movedim(1, -1)
        assert torch.allclose(scaled, want, atol=2e-6, rtol=0), method

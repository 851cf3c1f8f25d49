"""Video Enhance Prepare without a GPU: the node surface, messages, fps rule and anchor lists against the recorded run of the reference
(tests/golden/prepare.json), the C ABI of vrg_prepare_frames_f32, the band / segment plan of csrc/vrg_prepare_math.hpp compiled for the
host, the walk of the bicubic kernel replayed on the host against the recorded fp32 frames and PNG bytes, and the PNG writer.  No test
here reads the reference checkout."""
import ctypes as C
import inspect
import json
import os
import re
import shutil

import numpy as np
import pytest
import torch

import prepare_support as PS
from conftest import ROOT

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return PS.build_host_lib(tmp_path_factory.mktemp("prepare_check"))


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def vep(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_VideoEnhancePrepare
    return VRGDG_VideoEnhancePrepare


def test_fixture_provenance():
    prov = PS.META["provenance"]
    assert prov["ATEN_CPU_CAPABILITY"] == "default" and prov["cpu_capability"].upper() in ("DEFAULT", "NO AVX")
    assert len(PS.META["cases"]) == 5 and len(PS.META["errors"]) == 5
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "prepare.npz")) < (1 << 20)
    assert prov["recorder"] == "tools/record_prepare_golden.py" and prov["covers"] == ["prepare.json", "prepare.npz"]


def test_node_surface_equals_the_reference(vep):
    want = PS.META["surface"]
    cls = vep.VRGDGVideoEnhancePrepare
    assert cls.__name__ == want["class"]
    got = cls.INPUT_TYPES()
    assert list(got) == list(want["INPUT_TYPES"])
    for group in got:
        assert list(got[group]) == list(want["INPUT_TYPES"][group])                  # names and order
    assert json.loads(json.dumps(got)) == want["INPUT_TYPES"]                         # lists, defaults, min / max / step, tooltips
    assert list(cls.RETURN_TYPES) == want["RETURN_TYPES"] and list(cls.RETURN_NAMES) == want["RETURN_NAMES"]
    assert (cls.FUNCTION, cls.CATEGORY, cls.DESCRIPTION) == (want["FUNCTION"], want["CATEGORY"], want["DESCRIPTION"])
    assert list(inspect.signature(cls.prepare).parameters) == want["signature"]
    assert vep.VIDEO_ENHANCE_CONTEXT == want["context_type"]
    for name, params in want["helpers"].items():
        assert list(inspect.signature(getattr(vep, name)).parameters)[1:] == params[1:], name     # (the first is images_or_bytes here)
        assert len(inspect.signature(getattr(vep, name)).parameters) == len(params)
    assert list(inspect.signature(vep._save_image_batch).parameters) == ["images_or_bytes", "folder", "prefix"]


def test_mappings_are_separate_and_the_pinned_ones_unchanged(vep, pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_VideoEnhanceNodes as ven
    cls = vep.VRGDGVideoEnhancePrepare
    assert vep.PREPARE_NODE_CLASS_MAPPINGS == {"VRGDGVideoEnhancePrepare": cls}
    assert vep.PREPARE_NODE_DISPLAY_NAME_MAPPINGS == {"VRGDGVideoEnhancePrepare": PS.META["surface"]["display_name"]}
    assert ven.NODE_CLASS_MAPPINGS == {"VRGDGVideoEnhanceRestoreOriginal": ven.VRGDGVideoEnhanceRestoreOriginal}
    assert set(ven.NODE_DISPLAY_NAME_MAPPINGS) == {"VRGDGVideoEnhanceRestoreOriginal"}
    with open(os.path.join(ROOT, "tests", "golden", "node_surface.json"), encoding="utf-8") as fh:
        assert set(json.load(fh)) == set(pkg.NODE_CLASS_MAPPINGS) == set(pkg.NODE_DISPLAY_NAME_MAPPINGS)
    assert "VRGDGVideoEnhancePrepare" not in pkg.NODE_CLASS_MAPPINGS


def test_fps_table(vep):
    for info, fallback, want in PS.META["fps"]:
        got = vep._fps(info, fallback)
        assert isinstance(got, float) and got == want, (info, fallback)
    assert vep._fps({"fps": float("nan")}, 7.0) == 7.0


def test_anchor_lists(vep):
    want = {(1, 8): [0], (8, 8): [0, 7], (9, 8): [0, 8], (17, 8): [0, 8, 16], (18, 8): [0, 8, 16, 17], (16, 16): [0, 15], (120, 16): [0, 16, 32, 48, 64, 80, 96, 112, 119]}
    for (frames, interval), indices in want.items():
        assert vep._anchor_indices(frames, interval) == indices == PS.anchor_list(frames, interval)
    for case in PS.META["cases"]:
        interval = int(case["args"]["anchor_interval"].split()[0])
        assert vep._anchor_indices(case["shape"][0], interval) == case["anchor_indices"]
        assert case["returns"][:2] == [len(case["anchor_indices"]), ",".join(map(str, case["anchor_indices"]))]


def test_error_texts_are_the_reference_s(vep, tmp_path, monkeypatch):
    import types
    node = vep.VRGDGVideoEnhancePrepare()
    seen = 0
    with PS.stub_folder_paths(tmp_path):
        for e in PS.META["errors"]:
            if e["what"] == "batch":
                with pytest.raises(ValueError) as exc:
                    node.prepare(torch.zeros(e["shape"]), "8 frames", 16, 16, 16, 16, "8", PS.LETTERBOX, PS.BICUBIC, 24.0)
            elif e["what"] == "ffmpeg absent":
                monkeypatch.setattr(vep.shutil, "which", lambda name: None)
                monkeypatch.setitem(__import__("sys").modules, "imageio_ffmpeg", None)
                with pytest.raises(RuntimeError) as exc:
                    vep._encode_mp4(str(tmp_path), 3, 24.0, str(tmp_path / "none.mp4"))
            else:
                monkeypatch.setattr(vep.shutil, "which", lambda name: "ffmpeg")
                monkeypatch.setattr(vep.subprocess, "run", lambda command, **kw: types.SimpleNamespace(returncode=e["returncode"], stderr=e["stderr"], stdout=""))
                with pytest.raises(RuntimeError) as exc:
                    vep._encode_mp4(str(tmp_path / "frames"), 7, 29.97, str(tmp_path / "none.mp4"))
            assert type(exc.value).__name__ == e["type"] and str(exc.value) == e["text"], e["what"]
            seen += 1
    assert seen == 5


def test_ffmpeg_command_line(vep, tmp_path, monkeypatch):
    import types
    want = PS.META["ffmpeg"]
    frames, out = str(tmp_path / "frames"), str(tmp_path / "out.mp4")
    calls = []

    def run(command, **kwargs):
        calls.append((list(command), kwargs))
        open(out, "wb").close()
        return types.SimpleNamespace(returncode=0, stderr="", stdout="")

    monkeypatch.setattr(vep.shutil, "which", lambda name: "ffmpeg")
    monkeypatch.setattr(vep.subprocess, "run", run)
    vep._encode_mp4(frames, want["frame_count"], want["fps"], out)
    command, kwargs = calls[0]
    assert command == [a.replace("{frames}", frames).replace("{out}", out) for a in want["argv"]]
    assert kwargs == want["run_kwargs"]


def _prototype(name):
    header = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vrgdg_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_prototype_matches_the_ctypes_signature(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    name = "vrg_prepare_frames_f32"
    assert name in _hip.EXPORTED_SYMBOLS and name not in _hip.DEBUG_SYMBOLS
    res, args = _hip._SIGNATURES[name]
    proto = _prototype(name)
    assert res is C.c_int and len(proto) == len(args) == 21
    for text, ctype in zip(proto, args):
        assert ctype is (C.c_void_p if "*" in text else kinds[text.split()[0]]), text
    names = [a.split()[-1] for a in _prototype("vrg_resize_f32")]
    assert [a.split()[-1] for a in proto] == (["in", "frames", "in_h", "in_w", "in_channels", "frame_index", "n_out"] + names[6:17] +
                                              ["out_f32", "out_u8", "stream"])
    assert _hip.ABI_VERSION == 8
    assert "vrg_prepare_math.hpp" in build_ext.HEADERS and "vrg_prepare.hip" in build_ext.SOURCES


def test_argument_validation_without_device(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    lib = _hip.load_library()
    null, one, two, three, four = (C.c_void_p(v) for v in (0, 16, 32, 48, 64))
    ok = dict(in_h=8, in_w=8, in_c=3, src=(0, 0, 8, 8), out_h=4, out_w=4, dst=(0, 0, 4, 4))

    def prepare(a=one, frames=2, index=null, n_out=1, method=0, f32=two, u8=three, **kw):
        g = dict(ok, **kw)
        return lib.vrg_prepare_frames_f32(a, frames, g["in_h"], g["in_w"], g["in_c"], index, n_out, *g["src"], g["out_h"], g["out_w"], *g["dst"],
                                          method, f32, u8, null)

    assert prepare(n_out=0) == 0 and prepare(n_out=0, frames=0) == 0 and prepare(n_out=0, u8=null) == 0 and prepare(n_out=0, index=four) == 0
    assert prepare(f32=null, u8=null) == 1 and prepare(a=null) == 1                   # both outputs null, no input
    assert prepare(f32=one) == 1 and prepare(u8=one) == 1 and prepare(f32=two, u8=two) == 1     # aliasing
    assert prepare(index=one) == 1 and prepare(index=two) == 1 and prepare(index=three) == 1
    # overlap anywhere, not only equal starts: the input is 2 * 8 * 8 * 3 floats from 16, out_f32 16 * 3 floats, out_u8 48 bytes, the list 4 bytes
    far = C.c_void_p(1 << 20)
    assert prepare(f32=C.c_void_p(16 + 1532), u8=far) == 1 and prepare(f32=far, u8=C.c_void_p(16 + 1535)) == 1
    assert prepare(a=far, f32=C.c_void_p(4096), u8=C.c_void_p(4096 + 191)) == 1 and prepare(a=far, f32=C.c_void_p(4096 - 188), u8=C.c_void_p(4096)) == 1
    assert prepare(a=far, f32=C.c_void_p(4096), u8=C.c_void_p(8192), index=C.c_void_p(4096 + 188)) == 1
    assert prepare(a=far, f32=C.c_void_p(4096), u8=C.c_void_p(8192), index=C.c_void_p(8192 + 44)) == 1
    assert prepare(n_out=-1) == 1 and prepare(frames=-1) == 1
    assert prepare(method=4) == 1 and prepare(method=-1) == 1
    assert prepare(in_c=2) == 1 and prepare(in_h=0) == 1 and prepare(out_w=0) == 1 and prepare(src=(0, 0, 8, 9)) == 1
    assert prepare(dst=(4, 0, 4, 4)) == 1 and prepare(dst=(0, 0, 0, 4)) == 1
    assert prepare(frames=0, n_out=1) == 1 and prepare(frames=0, n_out=1, index=four) == 1
    assert prepare(frames=2, n_out=3) == 1                                            # no list: frames 0 .. n_out - 1 must exist
    assert prepare(a=C.c_void_p(18)) == 1 and prepare(f32=C.c_void_p(34)) == 1        # fp32 pointers are 4-byte aligned


def test_op_checks_its_arguments_before_anything_is_launched(ops):
    g = ops.ResizeGeometry(4, 4, (0, 0, 8, 8), (0, 0, 4, 4))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.prepare_frames(torch.zeros(2, 8, 8, 3), g, PS.BICUBIC)
    with pytest.raises(ValueError, match="frames, height, width, channels"):
        ops.prepare_frames(torch.zeros(8, 8, 3), g, PS.BICUBIC)
    assert ops._check_frame_indices([1, 0, 0, 1], 2) == [1, 0, 0, 1] and ops._check_frame_indices((), 2) == []
    for bad in ([2], [-1], [0, 5]):
        with pytest.raises(ValueError, match="outside the batch of 2 frame"):
            ops._check_frame_indices(bad, 2)
    with pytest.raises(ValueError, match="sequence of frame numbers"):
        ops._check_frame_indices(3, 2)


def _sweep(ops):
    for source in PS.SOURCES:
        for g in PS.geometries(ops, source):
            yield (1, *source), g
    yield (1, 2160, 3840, 3), ops.resize_geometry(2160, 3840, 960, 544, PS.LETTERBOX)
    yield (1, 8, 3840, 3), ops.resize_geometry(8, 3840, 960, 2, PS.STRETCH)
    yield (1, 8, 3840, 4), ops.resize_geometry(8, 3840, 960, 2, PS.STRETCH)
    yield (1, 1, 1, 3), ops.resize_geometry(1, 1, 8, 8, PS.STRETCH)


@needs_gxx
def test_plan_covers_every_pixel_once_and_fits_the_buffer(hm, ops):
    threads, band, stage = (hm.hm_prepare_constants(i) for i in range(3))
    assert (threads, band) == (256, 8) and stage % (4 * threads) == 0                  # prep_stage: whole 16-byte loads per thread
    seen = 0
    for shape, g in _sweep(ops):
        g13 = PS.geom13(shape, g)
        for staged in (1, 0):
            plan = np.zeros(3, dtype=np.int32)
            assert hm.hm_prepare_plan(g13, staged, plan) == 1, (shape, g)
            cps, segments, bands = (int(v) for v in plan)
            assert 1 <= cps <= threads and segments == -(-g.out_w // cps) and bands == -(-g.out_h // band)
            rows, cols, worst = np.zeros(g.out_h, dtype=np.int32), np.zeros(g.out_w, dtype=np.int32), np.zeros(3, dtype=np.int64)
            assert hm.hm_prepare_cover(g13, staged, rows, cols, worst) == 0, (shape, g)             # every tap inside its staged span
            assert (rows == 1).all() and (cols == 1).all(), (shape, g)
            if staged:
                assert 0 < worst[0] <= stage or g.dst[0] >= g.out_w, (shape, g, worst)
                assert worst[1] == 1 and worst[2] <= 4, (shape, g, worst)               # a row once per workgroup; a band primes four rows, so shares four at most
            seen += 1
    assert seen >= 2 * (4 * 12 + 1 + 4)
    # the seams that matter are there: the node's default fits one column per thread, the wide source is cut by the stage size
    plan = np.zeros(3, dtype=np.int32)
    hm.hm_prepare_plan(PS.geom13((1, 2160, 3840, 3), ops.resize_geometry(2160, 3840, 960, 544, PS.LETTERBOX)), 1, plan)
    assert list(plan) == [256, 4, 68]
    wide = PS.SOURCES[3]
    hm.hm_prepare_plan(PS.geom13((1, *wide), ops.resize_geometry(wide[0], wide[1], *PS.WIDE_TARGET, PS.STRETCH)), 1, plan)
    assert 1 < plan[0] < PS.WIDE_TARGET[0] and plan[1] >= 2
    # a single column whose taps do not fit is refused, not clipped
    assert hm.hm_prepare_plan(PS.geom13((1, 4, 8, 2000), ops.ResizeGeometry(2, 2, (0, 0, 8, 4), (0, 0, 2, 2))), 1, plan) == 0


@needs_gxx
def test_bicubic_walk_on_the_host_equals_the_recording(hm, ops):
    """the ring walk of k_prepare_bicubic, replayed by tests/host_math/prepare_check.cpp, gives the reference's fp32 frames bit for bit
    and the bytes of its PNG files, for the gathered anchors as for all frames"""
    golden = PS.arrays()
    seen = 0
    for case in PS.META["cases"]:
        if case["args"]["resize_method"] != PS.BICUBIC:
            continue
        x = PS.seeded_frames(case["seed"], case["shape"]).numpy()
        for which, indices in (("ltx", None), ("anchors", case["anchor_indices"])):
            width, height = (case["resolved"][("ltx_" if which == "ltx" else "anchor_") + k] for k in ("width", "height"))
            g = ops.resize_geometry(x.shape[1], x.shape[2], width, height, case["args"]["fit_mode"])
            n_out = x.shape[0] if indices is None else len(indices)
            f32 = np.empty((n_out, g.out_h, g.out_w, 3), dtype=np.float32)
            u8 = np.empty(f32.shape, dtype=np.uint8)
            index = None if indices is None else np.array(indices, dtype=np.int32)
            hm.hm_prepare_bicubic(x, None if index is None else index.ctypes.data, n_out, PS.geom13(x.shape, g), f32.ctypes.data, u8.ctypes.data)
            want = golden[f"{case['key']}.{which}"]
            assert f32.shape == want.shape and (f32.view(np.uint32) != want.view(np.uint32)).sum() == 0, (case["key"], which)
            assert np.array_equal(u8, golden[f"{case['key']}.{which}_png"]) and np.array_equal(u8, PS.quantise(f32))
            seen += 1
    assert seen == 4


@needs_gxx
def test_byte_rule_is_numpys(hm):
    k = np.arange(256, dtype=np.float32)
    half = ((k + np.float32(0.5)) / np.float32(255)).astype(np.float32)
    values = np.concatenate([k / np.float32(255), half, np.nextafter(half, np.float32(2)), np.nextafter(half, np.float32(-1)),
                             np.linspace(0, 1, 4097, dtype=np.float32)])
    values = values[(values >= 0) & (values <= 1)]
    got = np.array([hm.hm_prepare_byte(float(v)) for v in values], dtype=np.uint8)
    assert np.array_equal(got, PS.quantise(values))


def test_save_image_batch(vep, tmp_path):
    from PIL import Image
    folder = tmp_path / "frames"
    folder.mkdir()
    for stale in ("old.png", "OLD.JPG", "b.jpeg", "c.webp", "d.bmp", "frame_000009.png"):
        (folder / stale).write_bytes(b"x")
    (folder / "notes.txt").write_bytes(b"kept")
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, size=(3, 5, 7, 3), dtype=np.uint8)
    vep._save_image_batch(torch.from_numpy(frames), str(folder), "frame")
    assert sorted(os.listdir(folder)) == ["frame_000000.png", "frame_000001.png", "frame_000002.png", "notes.txt"]
    for i in range(3):
        with Image.open(folder / f"frame_{i:06d}.png") as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), frames[i])
    # float images are quantised as the reference quantises them
    x = PS.special_frames((2, 4, 6, 4), 9)
    vep._save_image_batch(x, str(tmp_path / "new" / "anchors"), "anchor")
    for i in range(2):
        with Image.open(tmp_path / "new" / "anchors" / f"anchor_{i:06d}.png") as im:
            assert np.array_equal(np.asarray(im), PS.quantise(x[i, ..., :3].clamp(0, 1).numpy()))


@pytest.mark.parametrize("ci", range(5))
def test_node_sequence_on_the_host(vep, ops, tmp_path, monkeypatch, ci):
    """prepare() run without a GPU: the two ops.prepare_frames results are stood in for by the recording (the pixels are the GPU test's),
    everything around them runs -- rounded sizes, fps, anchor list, geometries asked for, job folder, PNG files, the ffmpeg hand-off,
    the context and the 9-tuple -- and equals the recorded run of the reference"""
    from PIL import Image
    case, golden = PS.META["cases"][ci], PS.arrays()
    a = case["args"]
    x = PS.seeded_frames(case["seed"], case["shape"])
    asked, encodes = [], []

    def pixels(frames, ltx_geometry, anchor_geometry, indices, method):
        asked.append((frames, ltx_geometry, anchor_geometry, list(indices), method))
        return tuple(torch.from_numpy(golden[f"{case['key']}.{k}"]) for k in ("ltx", "ltx_png", "anchors", "anchors_png"))

    monkeypatch.setattr(vep, "_prepare_pixels", pixels)
    monkeypatch.setattr(vep, "_encode_mp4", lambda folder, count, fps, path: encodes.append((folder, count, fps, path)))
    monkeypatch.setattr(vep, "_log", lambda message: None)
    with PS.stub_folder_paths(tmp_path):
        out = vep.VRGDGVideoEnhancePrepare().prepare(x, **a)
    assert isinstance(out, tuple) and len(out) == 9
    frames, ltx_geometry, anchor_geometry, indices, method = asked[0]
    r = case["resolved"]
    assert len(asked) == 1 and frames is x and indices == case["anchor_indices"] and method == a["resize_method"]
    assert ltx_geometry == ops.resize_geometry(x.shape[1], x.shape[2], r["ltx_width"], r["ltx_height"], a["fit_mode"])
    assert anchor_geometry == ops.resize_geometry(x.shape[1], x.shape[2], r["anchor_width"], r["anchor_height"], a["fit_mode"])
    ctx = out[8]
    assert np.array_equal(out[0].numpy(), golden[f"{case['key']}.ltx"]) and np.array_equal(out[1].numpy(), golden[f"{case['key']}.anchors"])
    assert [out[2], out[3], out[5], out[6], out[7]] == case["returns"] and isinstance(out[7], float)
    assert list(ctx) == case["context_keys"] and ctx["original_frames"] is x
    assert {k: ctx[k] for k in case["context"]} == case["context"] and {k: ctx[k] for k in r} == r
    assert ctx["anchor_indices"] == case["anchor_indices"] and re.fullmatch(case["job_id_pattern"], ctx["job_id"])
    layout = case["layout"]
    job = os.path.join(str(tmp_path), *layout["job_folder"].replace("{job_id}", ctx["job_id"]).split("/"))
    frames_folder = os.path.join(job, layout["ltx_working_frames"])
    assert ctx["job_folder"] == job and ctx["anchor_sources_folder"] == os.path.join(job, layout["anchor_sources_folder"])
    assert out[4] == ctx["ltx_video_path"] == os.path.join(job, layout["ltx_video_path"])
    assert sorted(os.listdir(job)) == sorted([layout["anchor_sources_folder"], layout["ltx_working_frames"]])
    for folder, files, key in ((frames_folder, case["frame_files"], "ltx_png"), (ctx["anchor_sources_folder"], case["anchor_files"], "anchors_png")):
        assert sorted(os.listdir(folder)) == files
        decoded = np.stack([np.asarray(Image.open(os.path.join(folder, n))) for n in files])
        assert np.array_equal(decoded, golden[f"{case['key']}.{key}"])
    assert encodes == [(frames_folder, case["encode"]["frame_count"], case["encode"]["fps"], out[4])]
    assert case["frame_files"] == [f"frame_{i:06d}.png" for i in range(case["shape"][0])]
    assert case["anchor_files"] == [f"anchor_{i:06d}.png" for i in range(len(case["anchor_indices"]))]

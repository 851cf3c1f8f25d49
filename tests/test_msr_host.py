"""The LTX MSR reference frames without a GPU: the op's planning against the reference's recorded frames, the host check's refusals,
csrc/vrg_msr_math.hpp compiled for the host against the numpy restatement, the strip planner, the surface of the two node classes and
their error texts.  Fixture: tests/golden/msr_reference.npz (tools/make_golden_msr.py, the reference's own module)."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msr_support as M
from conftest import PKG_DIR, PKG_NAME, ROOT

HOST_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse"]
HOST_SOURCE = os.path.join(ROOT, "tests", "host_math", "msr_check.cpp")
INCLUDES = ["-I", os.path.join(PKG_DIR, "csrc"), "-I", os.path.join(ROOT, "include")]
MSR_SLOTS, MSR_TH = 40, 32

#: (in_w, in_h, out_w, out_h): the geometries of tests/test_gpu_msr.py
GEOMETRIES = ((1, 1, 32, 32), (7, 5, 33, 5), (37, 53, 96, 64), (301, 203, 64, 96), (1024, 16, 32, 64), (96, 64, 96, 64))


@pytest.fixture(scope="module")
def fixture():
    return np.load(M.FIXTURE)


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext, ops
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return ops


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    directory = tmp_path_factory.mktemp("msr_inputs")
    M.write_inputs(directory)
    return directory


@pytest.fixture()
def nodes(pkg, inputs):
    before = M.install_folder_paths(inputs)
    yield importlib.import_module(PKG_NAME + ".vrgdg_ltx_msr_reference_builder")
    M.restore_folder_paths(before)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("msr_host") / "libmsr_check.so")
    subprocess.run(["g++", *HOST_FLAGS, "-fPIC", "-shared", *INCLUDES, HOST_SOURCE, "-o", out], check=True)
    lib = C.CDLL(out)
    lib.hm_msr_check.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32]
    lib.hm_msr_frames.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    lib.hm_msr_frames.restype = None
    lib.hm_msr_strips.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    return lib


def test_inputs_are_the_recorded_ones(fixture, inputs):
    for name, (w, h, _seed, orientation) in M.PICTURES.items():
        assert np.array_equal(M.picture(name), fixture[f"in.{name}"]), name
        shown = M.decoded(inputs, name)
        assert shown.shape == ((w, h, 3) if orientation == 6 else (h, w, 3)), name
    assert np.array_equal(M.decoded(inputs, "turned.png"), np.rot90(fixture["in.turned.png"], -1))        # orientation 6: a quarter turn clockwise


def test_planning_gives_the_reference_frame_order(fixture, ops, nodes, inputs):
    """descriptors, repeats and frame ranges: frame f of the reference's batch is the restated resize of the picture whose run holds f"""
    for name, case in M.BUILDER_CASES.items():
        want = fixture[f"builder.{name}"]
        pics = [M.decoded(inputs, case[k]) for k in ("subject_1", "subject_2", "subject_3", "subject_4") if case[k] != M.NONE_IMAGE]
        frame_count = nodes.VRGDG_LTXMSRReferenceBuilder._resolve_frame_count(case["reference_strength"], len(pics))
        neutral = case["background_mode"] == "neutral_placeholder_wip"
        if not neutral:
            pics.append(M.decoded(inputs, case["background_image"]))
        size = (case["width"], case["height"])
        plan = ops.msr_plan([p.shape[:2] for p in pics], size, frame_count, (127, 127, 127) if neutral else None)
        plan.check()
        d = plan.desc
        assert len(d) == len(pics) + neutral and plan.frames == frame_count == want.shape[0], name
        assert d["repeats"].tolist() == ops.expand_counts(len(d), frame_count) and int(d["repeats"].sum()) == frame_count
        assert d["first_frame"].tolist() == [int(d["repeats"][:i].sum()) for i in range(len(d))]
        assert d["repeats"].max() - d["repeats"].min() <= 1 and sorted(d["repeats"].tolist(), reverse=True) == d["repeats"].tolist()
        for i, rec in enumerate(d):
            first, repeats = int(rec["first_frame"]), int(rec["repeats"])
            if i < len(pics):
                h, w = pics[i].shape[:2]
                same = (w, h) == size
                assert (rec["in_h"], rec["in_w"]) == (h, w) and (rec["taps"] == -1) == same, (name, i)
                if not same:
                    assert rec["taps"] == plan.offsets[(h, w)] and rec["taps"] % (size[0] + size[1]) == 0
                one = M.resized(pics[i], *size)
            else:
                assert rec["taps"] == -1 and rec["fill"].tolist() == [127, 127, 127, 0]
                one = np.full((size[1], size[0], 3), 127, dtype=np.uint8)
            assert repeats > 0 and all(np.array_equal(want[f], one) for f in range(first, first + repeats)), (name, i)
        assert plan.n_taps == len(plan.sizes) * (size[0] + size[1]) and plan.table().size == plan.n_taps * ops.LANCZOS_TAP_BYTES


def test_one_table_per_distinct_size(ops):
    plan = ops.msr_plan([(5, 7), (64, 96), (5, 7), (9, 9)], (96, 64), 41)
    assert plan.sizes == ((5, 7), (9, 9)) and plan.desc["taps"].tolist() == [0, -1, 0, 160] and plan.n_taps == 320
    assert plan.desc["repeats"].tolist() == [11, 10, 10, 10]
    few = ops.msr_plan([(5, 7), (5, 7), (5, 7)], (8, 8), 2)                    # fewer frames than pictures: the last repeats are 0
    assert few.desc["repeats"].tolist() == [1, 1, 0] and few.desc["first_frame"].tolist() == [0, 1, 2]
    few.check()
    for bad in (lambda: ops.msr_plan([], (8, 8), 1), lambda: ops.msr_plan([(0, 4)], (8, 8), 1), lambda: ops.msr_plan([(4, 4)], (0, 8), 1),
                lambda: ops.msr_plan([(4, 4)], (8, 8), -1), lambda: ops.msr_plan([(4, 4)], (8, 8), 1, fill=(1, 2, 256))):
        with pytest.raises(ValueError):
            bad()


def _records(ops, rows):
    d = np.zeros(len(rows), dtype=ops.MSR_DESC)
    for i, (src, in_h, in_w, taps, first, repeats) in enumerate(rows):
        d[i] = (src, in_h, in_w, taps, first, repeats, (0, 0, 0, 0))
    return d


def test_check_refusals(ops, host):
    """vrg_msr_check and the header compiled for the host agree: disjoint ranges that cover 0 .. frames - 1, table ranges, -1 only at the size"""
    from comfyui_vrgamedevgirl_amd import _hip
    lib = _hip.load_library()
    out_h, out_w, n_taps = 24, 40, 2 * 64
    cases = {
        "ok": ([(16, 5, 7, 0, 0, 3), (16, 9, 9, 64, 3, 2), (0, 0, 0, -1, 5, 1)], 6, 0),
        "ok_unordered_and_empty": ([(16, 9, 9, 64, 3, 3), (16, 5, 7, 0, 3, 0), (16, 5, 7, 0, 0, 3)], 6, 0),
        "ok_same_size": ([(16, 24, 40, -1, 0, 1)], 1, 0),
        "overlap": ([(16, 5, 7, 0, 0, 3), (16, 9, 9, 64, 2, 4)], 6, 1),
        "gap": ([(16, 5, 7, 0, 0, 3), (16, 9, 9, 64, 4, 2)], 6, 1),
        "short": ([(16, 5, 7, 0, 0, 3)], 4, 1),
        "starts_late": ([(16, 5, 7, 0, 1, 3)], 4, 1),
        "past_the_batch": ([(16, 5, 7, 0, 0, 5)], 4, 1),
        "negative_frame": ([(16, 5, 7, 0, -1, 5)], 4, 1),
        "negative_repeats": ([(16, 5, 7, 0, 0, 4), (16, 5, 7, 0, 4, -1)], 4, 1),
        "taps_past_the_table": ([(16, 5, 7, 65, 0, 1)], 1, 1),
        "taps_negative": ([(16, 5, 7, -2, 0, 1)], 1, 1),
        "unfiltered_at_another_size": ([(16, 24, 41, -1, 0, 1)], 1, 1),
        "empty_picture": ([(16, 0, 7, 0, 0, 1)], 1, 1),
        "nothing_for_one_frame": ([], 1, 1),
        "nothing_for_nothing": ([], 0, 0),
    }
    for name, (rows, frames, want) in cases.items():
        d = _records(ops, rows)
        p = C.c_void_p(d.ctypes.data) if len(d) else None
        assert lib.vrg_msr_check(p, len(d), n_taps, frames, out_h, out_w) == want, name
        assert host.hm_msr_check(p, len(d), n_taps, frames, out_h, out_w) == want, name
    d = _records(ops, cases["ok"][0])
    p = C.c_void_p(d.ctypes.data)
    assert lib.vrg_msr_check(p, 3, n_taps, 6, 0, out_w) == 1 and lib.vrg_msr_check(None, 3, n_taps, 6, out_h, out_w) == 1
    assert lib.vrg_msr_check(p, 3, 127, 6, out_h, out_w) == 1                   # the second table no longer fits
    # the launch validates before it touches a device: nothing to do is ok, a null or misaligned output is an argument error
    one = C.c_void_p(16)
    assert lib.vrg_msr_frames_f32(one, 0, one, n_taps, one, 6, out_h, out_w, None) == 0
    assert lib.vrg_msr_frames_f32(one, 3, one, n_taps, one, 0, out_h, out_w, None) == 0
    assert lib.vrg_msr_frames_f32(one, 3, one, n_taps, None, 6, out_h, out_w, None) == 1
    assert lib.vrg_msr_frames_f32(one, 3, one, n_taps, C.c_void_p(18), 6, out_h, out_w, None) == 1
    assert lib.vrg_msr_frames_f32(None, 3, one, n_taps, one, 6, out_h, out_w, None) == 1
    assert lib.vrg_msr_frames_f32(one, 3, one, n_taps, one, 6, out_h, 0, None) == 1


def test_header_gives_the_restatement(ops, host):
    """csrc/vrg_msr_math.hpp on the host -- the kernel's tiles, strips and slots -- equals restated(...) / 255 bit for bit, every repeat"""
    from lanczos_support import random_frames
    for seed, (in_w, in_h, out_w, out_h) in enumerate(GEOMETRIES):
        pics = [random_frames((1, in_h, in_w, 3), 40 + seed)[0], random_frames((1, in_h + 2, in_w + 1, 3), 50 + seed)[0]]
        plan = ops.msr_plan([p.shape[:2] for p in pics], (out_w, out_h), 6, fill=(3, 127, 252))
        assert plan.desc["repeats"].tolist() == [2, 2, 2]
        table = plan.table()
        desc = plan.desc.copy()
        for i, p in enumerate(pics):
            desc["src"][i] = p.ctypes.data
        plan.check(desc)
        out = np.full((plan.frames, out_h, out_w, 3), np.nan, dtype=np.float32)
        host.hm_msr_frames(C.c_void_p(desc.ctypes.data), len(desc), C.c_void_p(table.ctypes.data), C.c_void_p(out.ctypes.data), out_h, out_w)
        want = M.expected_frames(pics + [(3, 127, 252)], (out_w, out_h), [2, 2, 2])
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (in_w, in_h, out_w, out_h)


def test_strips_hold_what_their_rows_read(host):
    """a strip never passes the LDS rows; enlarging shares rows between neighbours, shrinking past 8 leaves no gap in the slots"""
    strips = np.zeros(2 * MSR_TH, dtype=np.int32)

    def plan(in_h, out_h, y0=0):
        n = host.hm_msr_strips(in_h, out_h, y0, C.c_void_p(strips.ctypes.data))
        return strips[:2 * n].reshape(n, 2).copy()

    for in_h, out_h in ((53, 64), (203, 96), (16, 64), (1024, 64), (1, 32), (3000, 1280), (5, 5), (900, 41)):
        for y0 in range(0, out_h, MSR_TH):
            s = plan(in_h, out_h, y0)
            assert int(s[:, 0].sum()) == min(MSR_TH, out_h - y0) and s[:, 0].min() >= 1
            assert s[:, 1].max() <= MSR_SLOTS and s[:, 1].min() >= 1
    assert plan(53, 64).tolist() == [[32, 30]]                                  # enlarging: one strip; s(31) = floor(31.5 * 53 / 64 - 0.5) = 25, so rows 0 .. 29
    assert plan(1, 32).tolist() == [[32, 1]]                                    # every tap is the one row
    assert plan(1024, 64, 32).tolist() == [[5, 40]] * 6 + [[2, 16]]             # 16 rows apart: five rows of eight slots each, no gap
    s = plan(3000, 1280, 640)
    assert s[:-1, 0].min() >= 13                                                # the default size: 2.34 source rows per row, 13-14 rows a strip


def test_check_program_under_the_sanitizers(tmp_path):
    """the host walk as a stand-alone executable with the address and undefined-behaviour sanitizers over its own geometries"""
    exe = str(tmp_path / "msr_check")
    cmd = ["g++", *HOST_FLAGS, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMSR_CHECK_MAIN", *INCLUDES, HOST_SOURCE,
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr + built.stdout and ("cannot find" in built.stderr or "unrecognized" in built.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and ran.stdout.strip() == "ok", ran.stdout + ran.stderr


def test_surface_equals_the_reference(fixture, nodes, pkg):
    doc = json.loads(str(fixture["surface"]))
    images = doc.pop("images")
    assert M.surface(nodes) == doc
    assert nodes.VRGDG_LTXMSRReferenceBuilder.INPUT_TYPES()["required"]["subject_1"][0] == images
    assert not hasattr(nodes.VRGDG_LTXMSRReferenceBuilder, "DESCRIPTION")
    assert not set(nodes.NODE_CLASS_MAPPINGS) & set(pkg.NODE_CLASS_MAPPINGS)      # mappings of its own
    resolve = nodes.VRGDG_LTXMSRReferenceBuilder._resolve_frame_count
    assert [resolve(s, 4) for s in nodes.VRGDG_LTXMSRReferenceBuilder.STRENGTHS[1:]] == [17, 25, 33, 41]
    assert [resolve("auto - based on subject count", n) for n in (0, 1, 2, 3, 4, 5)] == [17, 17, 25, 33, 41, 41]


def test_module_imports_without_comfyui(pkg):
    code = ("import sys; sys.path.insert(0, %r); import conftest; conftest.load_package(); import importlib; "
            "m = importlib.import_module(conftest.PKG_NAME + '.vrgdg_ltx_msr_reference_builder'); "
            "assert 'folder_paths' not in sys.modules and len(m.NODE_CLASS_MAPPINGS) == 2") % os.path.join(ROOT, "tests")
    ran = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stderr


def test_error_texts(nodes):
    """the reference's refusals, word for word, raised before anything goes to a device"""
    none = M.NONE_IMAGE
    b, l = nodes.VRGDG_LTXMSRReferenceBuilder(), nodes.VRGDG_LTX25MSRReferenceLoader()
    with pytest.raises(ValueError, match=r"^At least subject_1 must be set to an uploaded image\.$"):
        b.build_reference(none, none, none, none, "bg.png", "use_uploaded_background", 64, 96, "17 - light")
    with pytest.raises(ValueError, match=r"^background_image is required unless background_mode is neutral_placeholder_wip\.$"):
        b.build_reference("a.png", none, none, none, none, "use_uploaded_background", 64, 96, "17 - light")
    with pytest.raises(ValueError, match=r"^subject_1 is required for LTX 2\.5 MSR\.$"):
        l.load_references(none, "a.png", none, none, "bg.png", "use_uploaded_background", 64, 96)


def test_the_two_greys():
    """the builder's grey is float32(127) / float32(255) (a byte picture / 255), the loader's torch.full(..., 127 / 255.0) a Python double
    rounded to fp32: two roundings against one.  They are the SAME float, 0x3EFEFEFF -- the double lies nowhere near a tie of fp32"""
    import torch
    builder = np.float32(127) / np.float32(255)
    loader = torch.full((1,), 127 / 255.0, dtype=torch.float32).numpy()[0]
    assert builder.view(np.uint32) == loader.view(np.uint32) == 0x3EFEFEFF
    assert M.unit(np.array([127], dtype=np.uint8))[0].view(np.uint32) == 0x3EFEFEFF

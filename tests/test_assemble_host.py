"""The music-video assembly without a GPU: ops.assemble_plan against the reference restated in numpy, the reference's error texts,
csrc/vrg_assemble_math.hpp compiled for the host (quantisation chain, out-of-range rule, 64-bit frame offsets, the plain loops),
vrg_assemble_check's refusals, the node surface."""
import ctypes as C
import importlib
import itertools
import os

import numpy as np
import pytest
import torch

import assemble_support as S
from conftest import PKG_NAME

F32 = np.float32


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext, ops
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return ops


@pytest.fixture(scope="module")
def hip(ops):
    from comfyui_vrgamedevgirl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return S.build_host_lib(tmp_path_factory.mktemp("assemble_host"))


@pytest.fixture()
def node(pkg):
    return importlib.import_module(PKG_NAME + ".VRGDG_VideoAssembly")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_rounding_ties_are_pythons(ops):
    """half to even, on the double: 25 x 0.1 = 2.5 -> 2, 25 x 0.3 = 7.5 -> 8; frames-mode 96.5 -> 96, 97.5 -> 98"""
    assert 25.0 * 0.1 == 2.5 and 25.0 * 0.3 == 7.5
    lengths = [100, 100, 100, 100]
    plan = ops.assemble_plan("v3", lengths, 25.0, {"durations": [0.1, 0.3]})
    assert [sum(1 for s, _ in plan if s == i) for i in range(4)] == [2, 8, 1, 1]            # missing durations: 0.0 -> a target of 1
    plan = ops.assemble_plan("v5", lengths, 25.0, {"durations_frames": [96.5, 97.5, 0], "durations": [1, 1, 1, 1]})
    assert [sum(1 for s, _ in plan if s == i) for i in range(4)] == [96, 98, 1, 1]          # durations_frames before durations
    plan = ops.assemble_plan("v2", [3, 3, 3], 25.0, {"durations": [0.1, 0.3, 0.0]})
    assert [sum(1 for s, _ in plan if s == i) for i in range(3)] == [2, 8, 3] and plan[2:10] == [(1, 0), (1, 1)] + [(1, 2)] * 6


SWEEP_LENGTHS = ([97] * 16, [1 + i % 5 for i in range(16)], [3, None, 5, None, 2], [None, 4], [0, 3, 2])
SWEEP_DURATIONS = ([0.1, 0.3, 3.88, 0.0, 4.0], [96.5, 97.5, 1, 0, 3.5] * 4, [], [0.04] * 20)


@pytest.mark.parametrize("mode", ("v3", "v5"))
def test_plan_equals_the_restatement_v3_v5(ops, mode):
    n = 0
    for lengths, durations, key, fps, (index, total), groups in itertools.product(
            SWEEP_LENGTHS, SWEEP_DURATIONS, ("durations", "durations_frames"), (25.0, 24.0, 1.0), ((0, 1), (0, 3), (2, 3)), (0, 5, 16)):
        meta = {key: list(durations)}
        kw = dict(fps=fps, audio_meta=meta, index=index, total_sets=total, groups_in_last_set=groups)
        last = index == total - 1
        if not any(x is not None for x in lengths[:max(1, min(groups, 16)) if last else 16]):
            continue
        got = ops.assemble_plan(mode, lengths, **kw)
        assert got == S.restated_plan(mode, lengths, **kw), (lengths, kw)
        n += 1
    assert n > 500
    # groups_in_last_set = 0 on a last run: slot 1 is looked at and skipped -- an empty plan; on another run all 16 count
    assert ops.assemble_plan(mode, [4, 4], 25.0, {"durations": [1, 1]}, 0, 1, 0) == []
    assert len(ops.assemble_plan(mode, [4, 4], 25.0, {"durations": [1, 1]}, 0, 2, 0)) == 8
    assert meta == {key: list(durations)}                                                  # the caller's lists are not extended


def test_plan_equals_the_restatement_v2_pad_load(ops):
    for lengths, durations, fps in itertools.product(SWEEP_LENGTHS, SWEEP_DURATIONS + (["x", None, 0.2],), (25.0, 24.0)):
        if lengths[0] == 0:
            continue                                                                        # the reference pads an empty clip with nothing
        for meta in ({"durations": list(durations)}, {"durations": tuple(durations)}, {"durations_frames": [1]}, None):
            kw = dict(fps=fps, audio_meta=meta)
            assert ops.assemble_plan("v2", lengths, **kw) == S.restated_plan("v2", lengths, **kw), (lengths, kw)
    assert ops.assemble_plan("v2", [0, 2], 25.0, {"durations": [0.2, 0.2]}) == [(1, 0), (1, 1), (1, 1), (1, 1), (1, 1)]
    for frames, pad, front in itertools.product((0, 1, 4), (-1, 0, 1, 3), (False, True)):
        kw = dict(pad_frames=pad, pad_front=front)
        assert ops.assemble_plan("pad", [frames], **kw) == S.restated_plan("pad", [frames], **kw), (frames, kw)
    assert ops.assemble_plan("pad", [3], pad_frames=2, pad_front=True) == [(0, 0), (0, 0), (0, 0), (0, 1), (0, 2)]
    assert ops.assemble_plan("pad", [3], pad_frames=2, pad_front=False) == [(0, 0), (0, 1), (0, 2), (0, 2), (0, 2)]
    for lengths in SWEEP_LENGTHS:
        assert ops.assemble_plan("load", lengths) == S.restated_plan("load", lengths)


def test_error_texts_are_the_references(ops):
    ok = (2, 4, 4, 3)
    cases = [
        (("v2", [None, None], 25.0, {"durations": [1]}), "Provide at least one videos (e.g., video_1)."),
        (("v2", [ok, (4, 4, 3)], 25.0, None), "video_2 must have shape (frames,H,W,C), got (4, 4, 3)"),
        (("v3", [ok], 25.0, [1.0]), "[CombineV3] audio_meta must be a dict"),
        (("v3", [ok], 25.0, {"fps": 25}), "[CombineV3] audio_meta missing 'durations' or 'durations_frames' list"),
        (("v3", [None, ok], 25.0, {"durations": [1]}, 0, 1, 1), "[CombineV3] No video inputs detected. Connect at least one video_x input."),
        (("v3", [ok, (1, 2, 4, 4, 3)], 25.0, {"durations": [1]}), "video_2 must have shape (frames,H,W,C), got (1, 2, 4, 4, 3)"),
        (("v5", [ok], 25.0, None), "[CombineV5] audio_meta must be a dict"),
        (("v5", [ok], 25.0, {}), "[CombineV5] audio_meta missing durations info"),
        (("v5", [None], 25.0, {"durations": [1]}), "[CombineV5] No video inputs detected."),
        (("v5", [(4, 4, 3)], 25.0, {"durations": [1]}), "Expected (frames,H,W,C), got (4, 4, 3)"),
    ]
    for args, text in cases:
        with pytest.raises(ValueError) as e:
            ops.assemble_plan(*args)
        assert str(e.value) == text, args
    # V5 skips a slot beyond groups_in_last_set before it looks at its shape; V3 looks first
    assert ops.assemble_plan("v5", [ok, (4, 4, 3)], 25.0, {"durations": [1, 1]}, 0, 1, 1) == [(0, 0), (0, 1)]
    with pytest.raises(ValueError):
        ops.assemble_plan("v9", [ok])


def test_no_cpu_fallback(ops):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    clip = torch.zeros(2, 4, 4, 3)
    with pytest.raises(RuntimeError):
        ops.assemble_frames([clip], [(0, 0)])
    with pytest.raises(RuntimeError):
        ops.assemble_labelled_bytes([clip], [(0, 0)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the header on the host
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_quantisation_levels(host):
    """all 256 levels through q1 -> / 255 -> * 255 -> q2: the header equals numpy, and the levels that drop by one are the recorded ones"""
    k = np.arange(256, dtype=np.uint8)
    unit_np = k.astype(np.float32) / 255.0
    q2_np = (unit_np * 255).astype(np.uint8)
    q2, unit = np.zeros(256, np.uint8), np.zeros(256, F32)
    host.hm_assemble_levels(q2.ctypes.data, unit.ctypes.data)
    assert (unit.view(np.uint32) == unit_np.view(np.uint32)).all()
    assert (q2 == q2_np).all()
    drops = [int(i) for i in k if q2_np[i] != i]
    print("levels that drop by one:", drops)
    assert all(int(q2_np[i]) == i - 1 for i in drops) and drops == S.LEVELS_THAT_DROP
    # the whole chain from fp32: k / 255 and both neighbours, and a dense sweep of the contract range
    x = np.concatenate([unit_np, np.nextafter(unit_np, F32(2.0)), np.nextafter(unit_np, F32(-1.0))[1:],
                        np.linspace(0.0, 256.0 / 255.0, 200001, dtype=F32)[:-1]])
    x = x[(x * 255 >= 0) & (x * 255 < 256)]
    want = ((((x * 255).astype(np.uint8)).astype(np.float32) / 255.0) * 255).astype(np.uint8)
    got = np.zeros(len(x), np.uint8)
    host.hm_assemble_label_bytes(np.ascontiguousarray(x).ctypes.data, len(x), got.ctypes.data)
    assert (got == want).all()


def test_out_of_range_rule(host):
    """outside the contract the bytes saturate and NaN gives 0 -- this pack's own rule, stated in the header and the node's docstring"""
    x = np.array([np.nan, -np.inf, -3.0, -1e-3, -0.0, 256.0 / 255.0, 1.01, 7.0, 1e30, np.inf], dtype=F32)
    got = np.zeros(len(x), np.uint8)
    host.hm_assemble_label_bytes(x.ctypes.data, len(x), got.ctypes.data)
    assert got.tolist() == [0, 0, 0, 0, 0, 255, 255, 255, 255, 255]
    assert (x[5] * F32(255)) >= 256


def test_frame_offsets_are_64_bit(host):
    """a plan entry past 2^32 elements: arithmetic only, nothing is allocated"""
    n = 1080 * 1920 * 3
    assert host.hm_assemble_frame_offset(1551, n) == 1551 * n > 2 ** 32
    assert host.hm_assemble_frame_offset(96, n) == 96 * n < 2 ** 32 < host.hm_assemble_frame_offset(700, n) == 700 * n
    assert host.hm_assemble_frame_offset(2 ** 31 - 1, 2 ** 31 - 1) == (2 ** 31 - 1) ** 2
    # the launch shape: about 8192 workgroups, never more x tiles than a frame has, never none
    assert host.hm_assemble_grid_x(1519, 1552) == 6 and host.hm_assemble_grid_x(1519, 1) == 1519 and host.hm_assemble_grid_x(1, 5) == 1
    assert host.hm_assemble_grid_x(10, 100000) == 1


@pytest.mark.parametrize("name", ("v3-dword-5x7", "v5-sixteen", "v2-pad", "rgba-join", "two-tiles"))
def test_header_loops_equal_the_restatement(ops, hip, host, name):
    case = next(c for c in S.CASES if c["name"] == name)
    plan = ops.assemble_plan(case["mode"], [None if n is None else (n, *case["hwc"]) for n in case["lengths"]], **case["kw"])
    used = sorted({s for s, _ in plan})
    rows = np.array([(used.index(s), f) for s, f in plan], dtype=ops.ASSEMBLE_ENTRY)
    clips = S.case_clips(case, "special")
    want = S.expected_join(case, clips)
    out = np.zeros(want.shape, F32)
    d = S.host_desc(hip, [clips[s] for s in used])
    assert host.hm_assemble_join(C.byref(d), rows.ctypes.data, len(rows), out.ctypes.data) == 0
    assert S.same_bits(out, want) == 0
    data = [S.bytes_clip(c.shape, 7 + i) for i, c in enumerate(clips) if c is not None]
    every = iter(data)
    as_bytes = [None if c is None else next(every) for c in clips]
    d8 = S.host_desc(hip, [as_bytes[s] for s in used], is_bytes=True)
    assert host.hm_assemble_join(C.byref(d8), rows.ctypes.data, len(rows), out.ctypes.data) == 0
    assert S.same_bits(out, S.expected_join(case, [None if b is None else b.astype(np.float32) / 255.0 for b in as_bytes])) == 0
    if case["hwc"][2] != 3:
        return
    for with_overlays in (False, True):
        clips = S.case_clips(case, "contract")
        overlays = S.overlays_for(case) if with_overlays else None
        want = S.expected_labelled(case, clips, with_overlays)
        got = np.zeros(want.shape, np.uint8)
        d = S.host_desc(hip, [clips[s] for s in used], None if overlays is None else [overlays[s] for s in used])
        assert host.hm_assemble_labelled(C.byref(d), rows.ctypes.data, len(rows), got.ctypes.data) == 0
        assert S.same_bits(got, want) == 0


def test_check_refusals(ops, hip, host):
    """vrg_assemble_check, the library's and the header's: the same refusals with the status codes of the other _check entry points"""
    lib = hip.host_library()
    clips = [np.zeros((3, 5, 7, 3), F32) for _ in range(17)]
    out = np.zeros((4, 5, 7, 3), F32)
    data = np.zeros((4, 65, 7, 3), np.uint8)
    rows = np.array([(0, 0), (1, 2), (0, 1), (1, 0)], dtype=ops.ASSEMBLE_ENTRY)

    def both(d, table, n, f32, u8, labelled):
        a = lib.vrg_assemble_check(C.byref(d), None if table is None else table.ctypes.data, n, None if f32 is None else f32.ctypes.data,
                                   None if u8 is None else u8.ctypes.data, labelled)
        b = host.hm_assemble_check(C.byref(d), None if table is None else table.ctypes.data, n, None if f32 is None else f32.ctypes.data,
                                   None if u8 is None else u8.ctypes.data, labelled)
        assert a == b
        return a

    d = S.host_desc(hip, clips[:2])
    assert both(d, rows, 4, out, None, 0) == hip.VRG_OK and both(d, rows, 4, out, data, 1) == hip.VRG_OK
    assert both(d, None, 4, out, None, 0) == hip.VRG_OK and both(d, rows, 0, None, None, 0) == hip.VRG_OK
    d.n_src = 17                                                                            # more than 16 sources
    assert both(d, rows, 4, out, None, 0) == hip.VRG_ERR_BAD_ARG
    d.n_src = 0
    assert both(d, rows, 4, out, None, 0) == hip.VRG_ERR_BAD_ARG
    assert both(S.host_desc(hip, clips[:16]), rows, 4, out, None, 0) == hip.VRG_OK
    for other in ((3, 5, 8, 3), (3, 6, 7, 3), (3, 5, 7, 4)):                                # H, W or C differ
        assert both(S.host_desc(hip, [clips[0], np.zeros(other, F32)]), rows, 4, out, None, 0) == hip.VRG_ERR_BAD_ARG
    for bad in ((2, 0), (-1, 0), (1, 3), (0, -1)):                                          # a map entry outside its source
        table = rows.copy()
        table[1] = bad
        assert both(S.host_desc(hip, clips[:2]), table, 4, out, None, 0) == hip.VRG_ERR_BAD_ARG
    d = S.host_desc(hip, clips[:2])
    big = np.zeros((8, 5, 7, 3), F32)                                                       # out overlapping a source
    assert both(S.host_desc(hip, [big[:3], clips[1]]), rows, 4, big[2:6], None, 0) == hip.VRG_ERR_BAD_ARG
    assert both(S.host_desc(hip, [big[:2], clips[1]]), rows[2:], 2, big[2:6], None, 0) == hip.VRG_OK
    assert both(S.host_desc(hip, [np.zeros((3, 5, 7, 4), F32)]), rows[:1], 1, None, data, 1) == hip.VRG_ERR_BAD_ARG    # labelled, C != 3
    overlay = np.zeros((60, 7, 3), np.uint8)
    assert both(S.host_desc(hip, clips[:2], [overlay, None]), rows, 4, out, data, 1) == hip.VRG_OK
    assert both(S.host_desc(hip, clips[:2], [data.reshape(-1)[100:].reshape(-1)[:1260].reshape(60, 7, 3), None]), rows, 4, out, data, 1) == hip.VRG_ERR_BAD_ARG
    wide = hip.AssembleDesc()                                                               # a frame past 2^31 - 1 elements: nothing is read
    wide.n_src, wide.src[0], wide.frames[0], wide.height[0], wide.width[0], wide.channels[0] = 1, 1 << 20, 1, 32768, 32768, 3
    assert both(wide, None, 1, None, None, 0) == hip.VRG_ERR_UNSUPPORTED
    # the routes: bases and frame size on the 16-byte grid or not
    base = np.zeros(4 * 4 * 4 * 3 + 8, F32)
    at = (-base.ctypes.data // 4) % 4
    grid = base[at:at + 192].reshape(4, 4, 4, 3)
    assert grid.ctypes.data % 16 == 0
    assert host.hm_assemble_on_grid(C.byref(S.host_desc(hip, [grid])), grid.ctypes.data, None, 0) == 1
    off = base[at + 1:at + 1 + 144].reshape(3, 4, 4, 3)
    assert host.hm_assemble_on_grid(C.byref(S.host_desc(hip, [off])), grid.ctypes.data, None, 0) == 0
    odd = base[at:at + 105].reshape(1, 5, 7, 3)
    assert host.hm_assemble_on_grid(C.byref(S.host_desc(hip, [odd])), grid.ctypes.data, None, 0) == 0


def test_the_library_is_wired(ops, hip):
    from comfyui_vrgamedevgirl_amd import build_ext
    assert "vrg_assemble_math.hpp" in build_ext.HEADERS and "vrg_assemble.hip" in build_ext.SOURCES
    assert hip.ABI_VERSION == 8 and hip.host_library().vrg_abi_version() == 8
    assert {"vrg_assemble_check", "vrg_assemble_f32", "vrg_assemble_labelled_u8"} <= set(hip.EXPORTED_SYMBOLS)
    assert ops.ASSEMBLE_ENTRY.itemsize == 8 and ops.ASSEMBLE_BAR == S.BAR and ops.ASSEMBLE_SLOTS == S.SLOTS
    assert C.sizeof(hip.AssembleDesc) == 16 * 8 * 2 + 16 * 4 * 4 + 8


# ---------------------------------------------------------------------------------------------------------------------------------------
# the nodes
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_node_surface_equals_the_reference(pkg, node):
    assert sorted(node.ASSEMBLY_NODE_CLASS_MAPPINGS) == sorted(S.SURFACE)
    assert node.ASSEMBLY_NODE_DISPLAY_NAME_MAPPINGS == S.DISPLAY_NAMES
    for key, ref in S.SURFACE.items():
        cls = node.ASSEMBLY_NODE_CLASS_MAPPINGS[key]
        assert cls.__name__ == key
        got = cls.INPUT_TYPES()
        assert got == ref["INPUT_TYPES"], key
        for group in got:
            assert list(got[group]) == list(ref["INPUT_TYPES"][group]), (key, group)
        assert cls.RETURN_TYPES == ref["RETURN_TYPES"] and cls.RETURN_NAMES == ref["RETURN_NAMES"]
        assert cls.FUNCTION == ref["FUNCTION"] and cls.CATEGORY == ref["CATEGORY"] and callable(getattr(cls, cls.FUNCTION))
        assert getattr(cls, "VERSION", None) == ref.get("VERSION")
    assert len(node.VRGDG_CombinevideosV5.INPUT_TYPES()["optional"]) == 16
    # the package's own mappings are unchanged: the new module carries its own
    assert not set(S.SURFACE) & set(pkg.NODE_CLASS_MAPPINGS)
    for seam in ("label_renderer", "video_writer", "video_decoder"):
        assert callable(getattr(node, seam))


def test_nodes_pass_through_and_refuse_as_the_reference(node, monkeypatch, tmp_path):
    images = torch.zeros(0, 4, 4, 3)
    assert node.VRGDG_PadVideoWithLastFrame().pad_video(images, 3, False)[0] is images
    images = torch.zeros(2, 4, 4, 3)
    assert node.VRGDG_PadVideoWithLastFrame().pad_video(images, 0, True)[0] is images
    with pytest.raises(ValueError, match="No video files found in"):
        node.VRGDG_LoadVideos().load_videos(None, str(tmp_path), 3)
    (tmp_path / "a.mp4").write_bytes(b"")
    monkeypatch.setattr(node, "video_decoder", lambda path: None)
    with pytest.raises(ValueError, match="No frames loaded from any videos."):
        node.VRGDG_LoadVideos().load_videos(None, str(tmp_path), 3)
    with pytest.raises(ValueError, match="audio_meta must be a dict"):
        node.VRGDG_CombinevideosV5().blend_videos(25.0, 4.0, None, video_1=images)
    with pytest.raises(ValueError, match="Provide at least one videos"):
        node.VRGDG_CombinevideosV2().blend_videos(25.0, {"durations": [1]})

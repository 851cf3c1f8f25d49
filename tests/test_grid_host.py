"""The Video Folder Grid Plot without a GPU: csrc/vrg_grid_math.hpp compiled for the host (tests/host_math/grid_check.cpp) against the
independent numpy restatement and the float64 filters of tests/grid_support.py; the quantiser and the / 255 table against numpy; the
restatement's route against the reference's own methods as recorded in tests/golden/video_grid.json / .npz; the node's surface against
tests/golden/video_grid_surface.json; cv2 itself where a fixture or the package is at hand; the plan, the C ABI of the new entry points and
the refusals.  No test here reads the reference checkout."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import grid_support as G
from conftest import PKG_DIR, ROOT

F32 = np.float32
SWEEP = [(src, tile, mode, kind, c) for src, tile, mode in G.GEOMETRIES for kind in ("uniform", "smooth", "special") for c in (3, 4)]


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return G.build_host_lib(tmp_path_factory.mktemp("grid_check"))


@pytest.fixture(scope="module")
def node_module(pkg):
    from comfyui_vrgamedevgirl_amd import LTXLoraTrain
    return LTXLoraTrain


@pytest.fixture(scope="module")
def golden():
    with open(G.golden_paths()[0]) as fh:
        return json.load(fh), np.load(G.golden_paths()[1])


@pytest.mark.parametrize("src,tile,mode,kind,c", SWEEP)
def test_host_header_equals_the_restatement(hm, src, tile, mode, kind, c):
    x = G.FRAME_KINDS[kind]((1, src[0], src[1], c), 500 + src[0] + src[1])[0]
    keep = x.copy()
    assert hm.hm_grid_mode(src[0], src[1], tile[0], tile[1]) == mode == G.mode_of(src[0], src[1], tile[0], tile[1])
    want = G.resize_area(G.quantise(x), tile[1], tile[0])
    got = G.host_resize(hm, x, tile[0], tile[1])
    worst, share = G.differences(got, want)
    print(f"{src} -> {tile} {G.MODE_NAMES[mode]} {kind} C={c}: largest difference {worst} levels, {share:.4%} of the bytes differ")
    assert np.array_equal(got, want) and np.array_equal(x, keep, equal_nan=True)


@pytest.mark.parametrize("src,tile,mode", G.GEOMETRIES)
def test_byte_frames_are_their_own_quantisation(hm, src, tile, mode):
    b = G.bytes_frames((src[0], src[1], 3), 9)
    assert np.array_equal(G.host_resize(hm, b, tile[0], tile[1]), G.resize_area(b[..., ::-1], tile[1], tile[0]))
    assert np.array_equal(G.host_resize(hm, b, tile[0], tile[1]), G.host_resize(hm, b[..., ::-1].astype(F32) / F32(255.0), tile[0], tile[1]))


@pytest.mark.parametrize("src,tile,mode", G.GEOMETRIES)
def test_float64_yardstick(hm, src, tile, mode):
    """one final rounding: at most 1 level from the exact float64 area average (area rules) or from float64 bilinear at the same s, f (linear
    rule).  The share of differing bytes is a measurement: capped at 1.5 x the worst the restatement shows over these geometries
    (grid_support.AREA_WORST_SHARE = 0.02, LINEAR_WORST_SHARE = 0.0445)"""
    for kind in ("uniform", "smooth"):
        u8 = G.quantise(G.FRAME_KINDS[kind]((1, src[0], src[1], 3), 7)[0])
        got = G.host_resize(hm, u8[..., ::-1].copy(), tile[0], tile[1])
        assert np.array_equal(got, G.resize_area(u8, tile[1], tile[0]))
        worst, share = G.differences(got, G.yardstick64(u8, tile[0], tile[1]))
        cap = 1.5 * (G.LINEAR_WORST_SHARE if mode == G.LINEAR else G.AREA_WORST_SHARE)
        print(f"{src} -> {tile} {G.MODE_NAMES[mode]} {kind}: largest difference {worst} levels, {share:.4%} of the bytes differ (cap {cap:.4%})")
        assert worst <= G.YARDSTICK_MAX_LEVELS and share <= cap


def test_measured_shares_are_the_recorded_ones():
    worst = G.measure_shares()
    assert worst == {"area": G.AREA_WORST_SHARE, "linear": G.LINEAR_WORST_SHARE}


def test_quantiser_equals_numpy(hm):
    k = np.arange(256, dtype=F32) / F32(255.0)
    values = np.concatenate([k, np.nextafter(k, F32(2.0)), np.nextafter(k, F32(-1.0)), -k, k + F32(1.0), k * F32(3.0),
                             np.array([np.inf, -np.inf, -0.0, 0.0, 1.0, 255.0, 1e30, -1e30, 1e-45, -1e-45], dtype=F32)]).astype(F32)
    with np.errstate(over="ignore"):
        want = np.clip(values * 255.0, 0, 255).astype(np.uint8)
    assert np.array_equal(G.host_quant(hm, values), want) and np.array_equal(G.quantise(values[:, None].repeat(3, 1))[:, 0], want)
    assert np.array_equal(G.host_quant(hm, k), np.arange(256, dtype=np.uint8))                    # byte / 255 comes back as the byte
    assert G.host_quant(hm, np.array([np.nan], dtype=F32))[0] == 0                                # undefined in numpy: 0 here
    # truncation, not rounding: just below (k + 1) / 255 stays k
    assert np.array_equal(G.host_quant(hm, np.nextafter(k[1:], F32(-1.0))), np.arange(255, dtype=np.uint8))


def test_unit_table_equals_numpy(hm):
    table = np.empty(256, dtype=F32)
    hm.hm_grid_unit(table.ctypes.data)
    assert np.array_equal(table.view(np.uint32), (np.arange(256, dtype=np.float32) / 255.0).astype(F32).view(np.uint32))


def test_tables(hm, pkg):
    from comfyui_vrgamedevgirl_amd import ops
    for (H, W), (h, w), mode in G.GEOMETRIES:
        for n_in, n_out in ((W, w), (H, h)):
            cells = G.host_cells(hm, n_in, n_out, mode)
            assert np.array_equal(ops.grid_taps(n_in, n_out, mode).view(np.uint8), cells.view(np.uint8))
            first, count = cells["first"].astype(np.int64), cells["count"].astype(np.int64)
            assert first.min() >= 0 and (first + count).max() <= n_in and count.min() >= 1                 # every tap lies inside the axis
            if mode == G.LINEAR:
                s, _, c0, c1 = G.linear_taps(n_in, n_out)
                assert np.array_equal(first, s) and np.array_equal(cells["w_first"], c0.astype(F32)) and np.array_equal(cells["w_last"], c1.astype(F32))
                assert ((c0 + c1) == 2048).all() and (count == np.where(s + 1 <= n_in - 1, 2, 1)).all()
            elif mode == G.GENERAL:
                taps = G.area_taps(n_in, n_out)
                got = [(d, int(c["first"]) + k, F32(c["w_first"] if k == 0 else (c["w_last"] if k == int(c["count"]) - 1 else c["w_mid"])))
                       for d, c in enumerate(cells) for k in range(int(c["count"]))]
                assert got == taps
            else:
                step = n_in // n_out
                assert np.array_equal(first, np.arange(n_out) * step) and (count == step).all()
        assert 1 <= hm.hm_grid_cps(W, w, mode, 3) <= 64 and 1 <= hm.hm_grid_cps(W, w, mode, 4) <= 64
    assert hm.hm_grid_cps(20000, 2, G.GENERAL, 3) == 0 and hm.hm_grid_cps(4000, 64, G.GENERAL, 3) < 64     # segments, and too wide for one


def test_plan_geometry(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    for (H, W, cw, ch, band) in ((1080, 1920, 480, 270, 0), (1080, 1920, 480, 310, 40), (90, 30, 60, 60, 40), (5, 3, 64, 78, 40), (48, 64, 64, 88, 40),
                                 (33, 47, 47, 33, 0), (2160, 3840, 35, 80, 40)):
        t = ops.grid_tile(H, W, 3, cw, ch, band)
        assert (t.new_w, t.new_h, t.x_off, t.y_off) == G.tile_geometry(W, H, cw, ch, band)
        assert t.mode == G.mode_of(H, W, t.new_h, t.new_w) and ops.GRID_MODES[t.mode] == G.MODE_NAMES[t.mode]
    plan = ops.grid_plan([(48, 64, 3)] * 5, 35, 80, 3, 40)
    assert (plan.rows, plan.grid_w, plan.grid_h, len(plan.tiles)) == (2, 105, 160, 5)
    with pytest.raises(ValueError, match="does not fit"):
        ops.grid_plan([(40, 60, 3)], 60, 50, 1, 40)
    with pytest.raises(ValueError, match="3 or 4 channels"):
        ops.grid_plan([(40, 60, 2)], 60, 50, 1, 0)
    with pytest.raises(ValueError, match="more than 4096 source values"):
        ops.grid_plan([(16, 8192, 3)], 4, 16, 1, 0)
    assert ops.grid_plan([(16, 4000, 3)], 64, 16, 1, 0).tiles[0].cps < 64
    with pytest.raises(ValueError):
        ops.grid_plan([], 60, 50, 1, 0)


def test_golden_cases_pin_the_route_of_the_reference(golden):
    meta, grids = golden
    cases = meta["cases"]
    assert len(cases) >= 12 and meta["band"] == G.LABEL_BAND
    assert {len(c["inputs"]) for c in cases} >= {1, 2, 5, 10} and any(c.get("raises") == "ValueError" for c in cases)
    assert any(len(s) == 3 for c in cases for s, _ in c["inputs"]) and any(s[-1] == 4 for c in cases for s, _ in c["inputs"])
    modes = set()
    for case in cases:
        batches = G.golden_inputs(case)
        cw, ch = case["resolved_cell"]
        band = G.LABEL_BAND if case["label_tiles"] else 0
        first = batches[0] if batches[0].ndim == 4 else batches[0][None]
        assert cw == (case["cell_width"] or first.shape[2]) and ch == (case["cell_height"] or first.shape[1] + band)
        assert case["columns"] == G.choose_columns(len(batches))
        overlays = [G.pattern_label(t, cw, ch, band)[:band] for t in case["labels"]] if band else None
        if case.get("raises"):
            with pytest.raises(ValueError):
                G.grid_frames(batches, cw, ch, case["columns"], band, overlays)
            continue
        for b in batches:
            h, w = b.shape[-3], b.shape[-2]
            nw, nh, _, _ = G.tile_geometry(w, h, cw, ch, band)
            modes.add(G.mode_of(h, w, nh, nw))
        got = G.grid_frames(batches, cw, ch, case["columns"], band, overlays)
        want = grids[case["key"]].astype(F32) / F32(255.0)
        assert list(got.shape) == case["shape"] and np.array_equal(got.view(np.uint32), want.view(np.uint32)), case["key"]
    assert modes == {G.COPY, G.FAST, G.FAST_2X2, G.GENERAL, G.LINEAR}


def test_node_surface_equals_the_reference(node_module):
    with open(G.surface_path()) as fh:
        want = json.load(fh)
    node = node_module.VRGDG_VideoFolderGridPlot
    assert node.__bases__ == (object,)
    for name in ("RETURN_TYPES", "RETURN_NAMES"):
        assert list(getattr(node, name)) == want[name]
    for name in ("FUNCTION", "CATEGORY", "DESCRIPTION", "MAX_VIDEO_SLOTS", "LABEL_BAND_HEIGHT"):
        assert getattr(node, name) == want[name]
    assert sorted(node.VIDEO_EXTENSIONS) == want["VIDEO_EXTENSIONS"]
    assert json.loads(json.dumps(node.INPUT_TYPES())) == want["INPUT_TYPES"]
    assert list(node.INPUT_TYPES()["required"]) == list(want["INPUT_TYPES"]["required"])
    assert want["registered"] and node_module.NODE_CLASS_MAPPINGS == {"VRGDG_VideoFolderGridPlot": node}
    assert node_module.NODE_DISPLAY_NAME_MAPPINGS == {"VRGDG_VideoFolderGridPlot": want["display_name"]}
    assert node._choose_columns(0) == 1 and [node._choose_columns(n) for n in (1, 2, 4, 5, 9, 10, 20)] == [1, 2, 2, 3, 3, 4, 5]
    assert node._safe_name(" my grid!! ", "VideoGrid") == "my_grid" and node._safe_name("", "VideoGrid") == "VideoGrid"


def test_node_without_gpu_work(node_module, tmp_path, monkeypatch):
    node = node_module.VRGDG_VideoFolderGridPlot()
    (tmp_path / "notes.txt").write_text("x")
    (tmp_path / "a_VIDEOGRID_1.mp4").write_text("x")
    images, prefix, fps, status = node.run(str(tmp_path), "Grid", "", 4, 0, 0, True, 12)
    assert tuple(images.shape) == (1, 64, 64, 3) and images.dtype == torch.float32 and not images.any()
    assert (prefix, fps) == ("Grid", 12) and status == (f"No video files were found in {os.path.normpath(str(tmp_path))}. Connect video inputs or "
                                                        "point video_folder at a folder with videos.")
    # the seams name cv2 when it is missing, and only when they are needed
    try:
        import cv2  # noqa: F401
    except Exception:
        with pytest.raises(RuntimeError, match="cv2"):
            node_module.render_label("a", 64, 88, 40)
        with pytest.raises(RuntimeError, match="cv2"):
            node_module.open_capture(str(tmp_path / "a.mp4"))
    # a label that leaves the band is refused before anything reaches the GPU
    monkeypatch.setattr(node_module, "render_label", lambda text, w, h, band: np.full((h, w, 3), 9, dtype=np.uint8))
    with pytest.raises(ValueError, match="leaves the 40-row band"):
        node.run("", "Grid", "", 1, 0, 0, True, 12, video1=torch.zeros(1, 48, 64, 3))
    # nested inputs are flattened in order
    a, b, c = torch.zeros(1, 4, 4, 3), torch.zeros(4, 4, 3), torch.zeros(2, 4, 4, 3)
    flat = node._collect_selected_image_batches({"video2": {"x": [a, (b,)]}, "video1": c, "video3": "ignored"})
    assert [tuple(t.shape) for t in flat] == [(2, 4, 4, 3), (1, 4, 4, 3), (1, 4, 4, 3)]
    assert node._resolve_labels(["video1", "video2"], {"label_2": " mine "}) == ["video1", "mine"]


def test_grid_equals_cv2(hm, node_module):
    """the pin: cv2's own resizes in all five modes and its putText, from the fixture if it was made, else from an importable cv2; neither
    is at hand everywhere"""
    inputs = G.cv2_pin_inputs()
    if os.path.exists(G.cv2_fixture_path()):
        data = np.load(G.cv2_fixture_path())
        assert json.loads(str(data["provenance"]))["cases"] == [key for key, _, _ in inputs]
        cases = [(u8, data[key]) for key, u8, _ in inputs]
        labels = []
    else:
        cv2 = pytest.importorskip("cv2", reason="neither tests/golden/video_grid_cv2.npz nor the cv2 package (opencv-python) is available")
        cases = [(u8, cv2.resize(u8, (w, h), interpolation=cv2.INTER_AREA)) for _, u8, (h, w) in inputs]
        labels = [("video1", 480, 310, 40), ("a longer label", 200, 140, 40)]
    # one case at least tells 1.0 / ((double)n_out / n_in) from n_in / (double)n_out: the pin fails with the other formation
    assert any(G.scale_formations_differ(i.shape[1], o.shape[1]) or G.scale_formations_differ(i.shape[0], o.shape[0]) for i, o in cases
               if G.mode_of(i.shape[0], i.shape[1], o.shape[0], o.shape[1]) == G.GENERAL)
    assert {G.mode_of(i.shape[0], i.shape[1], o.shape[0], o.shape[1]) for i, o in cases} == {G.COPY, G.FAST, G.FAST_2X2, G.GENERAL, G.LINEAR}
    for u8, want in cases:
        got = G.resize_area(u8, want.shape[1], want.shape[0])
        worst, share = G.differences(got, want)
        print(f"{u8.shape} -> {want.shape}: largest difference {worst} levels, {share:.4%} of the bytes differ")
        assert np.array_equal(got, want) and np.array_equal(G.host_resize(hm, u8[..., ::-1].copy(), want.shape[0], want.shape[1]), want)
    for text, cw, ch, band in labels:
        import cv2
        canvas = np.zeros((ch, cw, 3), dtype=np.uint8)
        scale = max(0.45, min(1.0, cw / 420.0))
        size, base = cv2.getTextSize(text, cv2.FONT_HERSHEY_SIMPLEX, scale, 2)
        org = (max(8, (cw - size[0]) // 2), max(size[1] + 6, (band + size[1]) // 2 - base))
        cv2.putText(canvas, text, org, cv2.FONT_HERSHEY_SIMPLEX, scale, (255, 255, 255), 2, cv2.LINE_AA)
        assert np.array_equal(node_module.render_label(text, cw, ch, band), canvas)


def test_scale_formations(hm):
    """cv2 forms scale = 1.0 / ((double)n_out / n_in), vrg_area_math.hpp forms n_in / 64.0 for its own case.  The general-rule cells of the
    two differ for 44 of the pairs n_out <= n_in <= 1024 and for 27,025 of those up to 4096 (the latter takes a minute on
    one core and is not repeated here: grid_support.scale_pairs(lib, 4096)); the first pair is (953, 413), which is in the sweep and in the
    cv2 pin"""
    limit, count, first = G.SCALE_PAIRS_1024
    assert G.scale_pairs(hm, limit) == (count, first) and G.SCALE_PAIRS_4096[2] == first
    assert G.scale_formations_differ(*first) and not G.scale_formations_differ(131, 57)
    assert ((8, first[0]), (8, first[1]), G.GENERAL) in G.GEOMETRIES
    a, b = G.scales(*first)[1], first[0] / first[1]
    assert a != b
    cells = G.host_cells(hm, first[0], first[1], G.GENERAL)
    got = [(d, int(c["first"]) + k, F32(c["w_first"] if k == 0 else (c["w_last"] if k == int(c["count"]) - 1 else c["w_mid"])))
           for d, c in enumerate(cells) for k in range(int(c["count"]))]
    assert got == G.area_taps(*first) and got != G.area_taps(*first, scale=b)                # the header forms cv2's scale, not the other


def test_segmented_geometries_take_the_row_buffer_in_pieces(hm):
    for (H, W), (h, w) in G.SEGMENTED:
        mode = G.mode_of(H, W, h, w)
        assert hm.hm_grid_cps(W, w, mode, 3) < 64 and hm.hm_grid_cps(W, w, mode, 4) < 64
    assert all(hm.hm_grid_cps(W, w, m, 3) == 64 for (H, W), (h, w), m in G.GEOMETRIES if ((H, W), (h, w)) not in G.SEGMENTED)


def test_check_program_under_the_sanitizers(tmp_path):
    """the check program as a stand-alone executable with the address and undefined-behaviour sanitizers: every rule once"""
    exe = str(tmp_path / "grid_check")
    cmd = ["g++", *G.HOST_FLAGS, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGRID_CHECK_MAIN",
           "-I", os.path.join(PKG_DIR, "csrc"), G.host_source(), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr + built.stdout and ("cannot find" in built.stderr or "unrecognized" in built.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("grid_check:"), run.stderr


def test_library_exports_the_symbols_and_the_abi_is_8(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    lib = _hip.load_library()
    assert lib.vrg_abi_version() == 8 == _hip.ABI_VERSION
    for name in ("vrg_grid_plan", "vrg_grid_taps", "vrg_grid_check", "vrg_grid_tiles_f32", "vrg_grid_tiles_u8"):
        assert name in _hip.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert "vrg_grid_math.hpp" in build_ext.HEADERS and "vrg_grid.hip" in build_ext.SOURCES
    header = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    fields = header[header.index("typedef struct vrg_grid_desc"):header.index("} vrg_grid_desc;")]
    assert C.sizeof(_hip.GridDesc) == 88 == np.dtype(__import__("comfyui_vrgamedevgirl_amd").ops.GRID_DESC).itemsize
    for name, _ in _hip.GridDesc._fields_:
        assert name in fields, name


def test_entry_point_refusals_without_device(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, ops
    lib = _hip.load_library()
    null, a, b = C.c_void_p(0), C.c_void_p(64), C.c_void_p(4096)
    for entry in (lib.vrg_grid_tiles_f32, lib.vrg_grid_tiles_u8):
        assert entry(a, 0, b, 1, 8, 8, 8, 8, null) == _hip.VRG_OK == entry(a, 1, b, 0, 8, 8, 8, 8, null)                # nothing to do: no launch
        assert entry(null, 1, b, 1, 8, 8, 8, 8, null) == entry(a, 1, null, 1, 8, 8, 8, 8, null) == _hip.VRG_ERR_BAD_ARG
        assert entry(a, -1, b, 1, 8, 8, 8, 8, null) == entry(a, 1, b, 1, 0, 8, 8, 8, null) == entry(a, 1, b, 1, 8, 8, 7, 8, null) == _hip.VRG_ERR_BAD_ARG
        assert entry(C.c_void_p(68), 1, b, 1, 8, 8, 8, 8, null) == entry(a, 1, C.c_void_p(4098), 1, 8, 8, 8, 8, null) == _hip.VRG_ERR_BAD_ARG
    mode, cps, inv = C.c_int32(), C.c_int32(), C.c_float()
    assert lib.vrg_grid_plan(96, 128, 3, 48, 64, C.byref(mode), C.byref(cps), C.byref(inv)) == _hip.VRG_OK
    assert (mode.value, cps.value, inv.value) == (_hip.GRID_FAST_2X2, 64, 0.25)
    assert lib.vrg_grid_plan(4, 20000, 3, 2, 2, C.byref(mode), C.byref(cps), C.byref(inv)) == _hip.VRG_ERR_UNSUPPORTED
    assert lib.vrg_grid_plan(0, 8, 3, 8, 8, C.byref(mode), C.byref(cps), C.byref(inv)) == _hip.VRG_ERR_BAD_ARG
    assert lib.vrg_grid_plan(8, 8, 5, 8, 8, C.byref(mode), C.byref(cps), C.byref(inv)) == _hip.VRG_ERR_BAD_ARG
    table = np.zeros(64, dtype=ops.AREA_CELL)
    assert lib.vrg_grid_taps(20, 64, _hip.GRID_GENERAL, C.c_void_p(table.ctypes.data)) == _hip.VRG_ERR_BAD_ARG       # enlarging is linear
    assert lib.vrg_grid_taps(100, 64, _hip.GRID_FAST, C.c_void_p(table.ctypes.data)) == _hip.VRG_ERR_BAD_ARG
    assert lib.vrg_grid_taps(64, 64, 9, C.c_void_p(table.ctypes.data)) == lib.vrg_grid_taps(64, 64, 0, null) == _hip.VRG_ERR_BAD_ARG
    # descriptors: a tile outside the grid, a picture outside its tile, a mode other than the plan's
    d = np.zeros(1, dtype=ops.GRID_DESC)
    check = lambda: lib.vrg_grid_check(C.c_void_p(d.ctypes.data), 1, 0, 2, 64, 48, 128, 48)
    assert check() == _hip.VRG_OK
    for field, value in (("frame", 2), ("frame", -1), ("dst_x", 65), ("dst_y", 1), ("band", 49)):
        keep = d[field][0]
        d[field] = value
        assert check() == _hip.VRG_ERR_BAD_ARG, field
        d[field] = keep
    good = dict(src=4096, xtab=4096, ytab=4096, height=96, width=128, channels=3, mode=_hip.GRID_FAST_2X2, new_w=64, new_h=48, cps=64)
    for k, v in good.items():
        d[k] = v
    assert check() == _hip.VRG_OK
    for field, value in (("mode", _hip.GRID_GENERAL), ("new_w", 65), ("x_off", 1), ("y_off", 1), ("channels", 2), ("cps", 0), ("cps", 65), ("xtab", 0),
                         ("src", 4098), ("height", 0)):
        keep = d[field][0]
        d[field] = value
        assert check() == _hip.VRG_ERR_BAD_ARG, field
        d[field] = keep
    assert lib.vrg_grid_check(C.c_void_p(d.ctypes.data), 1, 1, 2, 64, 48, 128, 48) == _hip.VRG_OK
    d["channels"] = 4
    assert check() == _hip.VRG_OK and lib.vrg_grid_check(C.c_void_p(d.ctypes.data), 1, 1, 2, 64, 48, 128, 48) == _hip.VRG_ERR_BAD_ARG

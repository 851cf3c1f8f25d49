"""Reference sheets without a GPU: the layout code equals the reference's recorded rect lists as floats, exactly, and its integer panel
rectangles; csrc/vrg_sheet_math.hpp compiled for the host (tests/host_math/sheet_check.cpp) equals the canvases the reference itself
recorded (tests/golden/sheet.{json,npz}) and the plain-Pillow restatement of tests/sheet_support.py byte for byte, and byte / 255 bit for
bit; the case list reaches every class of panel; the check program runs under the sanitizers as a stand-alone executable; the C ABI of the
new entry points and their refusals.  No test here reads the reference checkout."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import sheet_support as S
from conftest import PKG_DIR, ROOT

NEW_SYMBOLS = ("vrg_sheet_fit", "vrg_sheet_plan", "vrg_sheet_check", "vrg_sheet_rows_f32", "vrg_sheet_rows_u8", "vrg_sheet_compose_f32",
               "vrg_sheet_compose_u8")


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return S.build_host_lib(tmp_path_factory.mktemp("sheet_check"))


@pytest.fixture(scope="module")
def golden():
    with open(S.FIXTURE_JSON) as fh:
        return json.load(fh), np.load(S.FIXTURE_NPZ)


@pytest.fixture(scope="module")
def grid(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    from comfyui_vrgamedevgirl_amd import VRGDG_LTXICIngredientsGrid
    return VRGDG_LTXICIngredientsGrid


@pytest.fixture(scope="module")
def case_runs(hm):
    """every small case once: (status, bytes, floats, details, byte sources)"""
    out = {}
    for name, case in S.CASES.items():
        sources = [S.source(n) for n in case["sources"]]
        out[name] = (*S.host_sheet(hm, sources, case["panels"], case["canvas"], case["background"]), [S.quantise(s) for s in sources])
    return out


def test_layouts_equal_the_recorded_rects_as_floats(grid, golden):
    z = golden[1]
    keys, counts, rects = S.layout_keys(), z["layout.counts"], z["layout.rects"]
    assert len(keys) == len(counts) == 7 * 24 * 4 and rects.dtype == np.float64 and int(counts.sum()) == len(rects)
    at = 0
    for key, n in zip(keys, counts):
        got = np.array(grid.layout_rects(*key), dtype=np.float64).reshape(-1, 4)
        assert len(got) == n == key[1] and np.array_equal(got, rects[at:at + n]), key         # float equality, exactly
        at += n
    keys, values, rects = S.aspect_keys(), z["aspect.values"], z["aspect.rects"]
    assert len(keys) >= 36
    at = 0
    for aspects, canvas in keys:
        n = len(aspects)
        got = np.array(grid.aspect_row_rects([float(v) for v in values[at:at + n]], *canvas), dtype=np.float64).reshape(-1, 4)
        assert np.array_equal(got, rects[at:at + n]), (aspects, canvas)
        at += n
    assert at == len(values) == len(rects)


def test_panel_rectangles_equal_the_recorded_integers(grid, golden):
    for name, case in S.NODE_CASES.items():
        panels, _bg = S.node_panels(grid, case, [f.shape for f in S.node_frames(case)])
        assert [list(p["rect"]) for p in panels] == golden[0]["panels"][name], name


def test_parse_color(grid):
    f = grid.parse_color
    assert f("black", "#b8b8b8") == (0, 0, 0) and f("White", "#000000") == (255, 255, 255) and f(" grey ", "#000000") == (128, 128, 128)
    assert f("neutral_gray", "#000000") == f("neutral_grey", "#000000") == (184, 184, 184) and f("gray", "#000000") == (128, 128, 128)
    assert f("#abc", "#000000") == (0xAA, 0xBB, 0xCC) and f("abc", "#000000") == (0xAA, 0xBB, 0xCC) and f("#102030", "#ffffff") == (16, 32, 48)
    assert f("", "#b8b8b8") == f(None, "#b8b8b8") == (184, 184, 184)
    assert f("#12345", "#b8b8b8") == (184, 184, 184) and f("nonsense", "#b8b8b8") == (184, 184, 184)         # wrong length: the fallback
    assert f("#gggggg", "#b8b8b8") == (184, 184, 184) and f("zzzzzz", "#zzzzzz") == (0, 0, 0)                # not hex: the fallback, then black


def test_node_surface_is_the_references(grid):
    node = grid.VRGDG_LTXICIngredientsGrid
    types = node.INPUT_TYPES()
    assert list(types["required"]) == ["image_count", "layout", "output_width", "output_height", "columns", "gutter", "outer_padding",
                                       "corner_radius", "fit_mode", "batch_mode", "background_color", "cell_background_color"]
    assert list(types["optional"]) == [f"image{i}" for i in range(1, 25)] and node.MAX_IMAGES == 24
    assert node.LAYOUTS == S.LAYOUTS and node.FIT_MODES == S.FIT_MODES and node.BATCH_MODES == ["first_image_only", "all_images"]
    assert (node.RETURN_TYPES, node.RETURN_NAMES, node.FUNCTION, node.CATEGORY) == (("IMAGE",), ("reference_sheet",), "build", "VRGDG/LTX")
    assert grid.NODE_CLASS_MAPPINGS == {"VRGDG_LTXICIngredientsGrid": node}
    assert grid.NODE_DISPLAY_NAME_MAPPINGS == {"VRGDG_LTXICIngredientsGrid": "VRGDG LTX IC Ingredients Grid"}
    with pytest.raises(ValueError, match="needs at least one connected image input"):
        node().build(**S.NODE_DEFAULTS)


def test_units_are_numpys_division_bit_for_bit(hm):
    got = np.zeros(256, np.float32)
    hm.hm_sheet_units(got.ctypes.data)
    want = np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_quantiser_is_numpys_line_and_nan_gives_zero(hm):
    v = S.source("97x8").reshape(-1)
    want = S.quantise(v[:, None])[:, 0]
    assert np.array_equal(np.array([hm.hm_sheet_quant(float(x)) for x in v], dtype=np.uint8), want)
    assert hm.hm_sheet_quant(float("nan")) == 0                             # numpy leaves NaN undefined: pinned to 0 here, kept out of Pillow


@pytest.mark.parametrize("name", sorted(S.NODE_CASES))
def test_host_build_equals_the_references_canvases(hm, grid, golden, name):
    case = S.NODE_CASES[name]
    frames = S.node_frames(case)
    panels, background = S.node_panels(grid, case, [f.shape for f in frames])
    rc, u8, f32, _ = S.host_sheet(hm, frames, panels, (case["output_width"], case["output_height"]), background)
    assert rc == 0
    assert np.array_equal(u8, golden[1][f"node.{name}"])
    assert np.array_equal(f32.view(np.uint32), (u8.astype(np.float32) / np.float32(255)).view(np.uint32))
    assert np.array_equal(S.pillow_sheet([S.quantise(f) for f in frames], panels, (case["output_width"], case["output_height"]), background), u8)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_host_build_equals_plain_pillow(case_runs, name):
    pytest.importorskip("PIL")
    case = S.CASES[name]
    rc, u8, f32, _details, byte_sources = case_runs[name]
    assert rc == 0
    assert np.array_equal(u8, S.pillow_sheet(byte_sources, case["panels"], case["canvas"], case["background"]))
    assert np.array_equal(f32.view(np.uint32), (u8.astype(np.float32) / np.float32(255)).view(np.uint32))


def test_byte_sources_are_their_own_quantisation(hm):
    case = S.CASES["overlap_clip"]
    byte_sources = [S.quantise(S.source(n)) for n in case["sources"]]
    rc, u8, _f, _d = S.host_sheet(hm, byte_sources, case["panels"], case["canvas"], case["background"])
    assert rc == 0 and np.array_equal(u8, S.pillow_sheet(byte_sources, case["panels"], case["canvas"], case["background"]))


def test_the_case_list_reaches_every_class(case_runs):
    """a thinned list fails here"""
    seen = set()
    for name, case in S.CASES.items():
        _rc, u8, _f, details, byte_sources = case_runs[name]
        width, height = case["canvas"]
        for p, d in zip(case["panels"], details):
            d = dict(zip(S.DETAILS, (int(v) for v in d)))
            sh, sw = byte_sources[p["source"]].shape[:2]
            left, top, w, h = p["rect"]
            hp, vp = sw != d["new_w"], sh != d["new_h"]
            seen.add({(True, True): "both passes", (False, True): "h skipped", (True, False): "v skipped", (False, False): "both skipped"}[(hp, vp)])
            seen.add("upscale" if d["new_w"] > sw or d["new_h"] > sh else "downscale" if d["new_w"] < sw or d["new_h"] < sh else "same size")
            if p["fit"] == "cover_crop" and (d["win_x"] > 0 or d["win_y"] > 0):
                seen.add("crop offset")
            if p["fit"] == "contain_pad":
                for margin in (w - d["new_w"], h - d["new_h"]):
                    seen.add("margin 0" if margin == 0 else "odd margin" if margin % 2 else "even margin")
            if p["radius"] > 0 and (w, h) == (1, 1):
                seen.add("1x1 pastes nothing")
                without = S.pillow_sheet(byte_sources, [q for q in case["panels"] if q is not p], case["canvas"], case["background"])
                assert np.array_equal(u8[top, left], without[top, left])                # what was there before stays
            if p["radius"] > min(w // 2, h // 2) > 0:
                seen.add("clamped radius")
            if left < 0 or top < 0 or left + w > width or top + h > height:
                seen.add("cut by the edge")
            if d["h_ksize"] > 100:
                seen.add("hundreds of taps")
            if d["rows"] < sh and vp:
                seen.add("rows left out")
            seen.add(f"C={S.SOURCES[case['sources'][p['source']]][2]}")
        rects = [p["rect"] for p in case["panels"]]
        if any(a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3] for i, a in enumerate(rects) for b in rects[:i]):
            seen.add("overlap")
        if len(rects) > 24:
            seen.add("more than 24 panels")
        if width * 3 % 4 or width * 3 % 16:
            seen.add("off the vector grid")
    want = {"both passes", "h skipped", "v skipped", "both skipped", "upscale", "downscale", "crop offset", "margin 0", "odd margin",
            "1x1 pastes nothing", "clamped radius", "cut by the edge", "hundreds of taps", "overlap", "more than 24 panels", "off the vector grid",
            "C=1", "C=3", "C=4"}
    assert want <= seen, want - seen


def test_mask_rows_are_single_runs():
    for w, h, r in ((5, 5, 2), (40, 23, 3), (40, 23, 11), (200, 100, 96), (7, 3, 1), (2, 9, 1), (1, 1, 0)):
        spans = S.mask_spans(w, h, r)                                       # asserts one run per row
        if (w, h) == (1, 1):
            assert spans.tolist() == [[1, 0]]                               # the 1 x 1 mask is empty


def test_check_program_under_the_sanitizers(tmp_path):
    """the check program as a stand-alone executable with the address and undefined-behaviour sanitizers, over the case list"""
    exe, listing = str(tmp_path / "sheet_check"), str(tmp_path / "cases.txt")
    cmd = ["g++", *S.HOST_FLAGS, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSHEET_CHECK_MAIN",
           "-I", os.path.join(PKG_DIR, "csrc"), "-I", os.path.join(ROOT, "include"), S.HOST_SOURCE, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr + built.stdout and ("cannot find" in built.stderr or "unrecognized" in built.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert built.returncode == 0, built.stderr
    words = [len(S.CASES)]
    for case in S.CASES.values():
        recs, spans, n_spans = S.panel_records(case["panels"])
        r, g, b = case["background"]
        words += [*case["canvas"], r | (g << 8) | (b << 16), len(case["sources"])]
        for n in case["sources"]:
            words += list(S.SOURCES[n][:3])
        words += [len(recs), *recs.reshape(-1).tolist(), n_spans, *spans[:n_spans].reshape(-1).tolist()]
    with open(listing, "w") as fh:
        fh.write(" ".join(str(int(v)) for v in words))
    run = subprocess.run([exe, listing], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith(f"sheet_check: {len(S.CASES)} sheets"), run.stdout + run.stderr


# ------------------------------------------------------------------------------------------------
# the C ABI without a device
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip(grid):
    from comfyui_vrgamedevgirl_amd import _hip, ops
    return _hip, ops, _hip.load_library()


def test_library_exports_the_symbols_and_the_abi_is_8(hip, hm):
    _hip, ops, lib = hip
    assert lib.vrg_abi_version() == 8 == _hip.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert hasattr(lib._cdll, name), name
    assert hm.hm_sheet_panel_bytes() == C.sizeof(_hip.SheetPanel) == ops.SHEET_PANEL.itemsize == 128
    assert [n for n, _ in _hip.SheetPanel._fields_] == list(ops.SHEET_PANEL.names)
    assert [getattr(_hip.SheetPanel, n).offset for n in ops.SHEET_PANEL.names] == [ops.SHEET_PANEL.fields[n][1] for n in ops.SHEET_PANEL.names]
    header = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    assert f"#define VRG_SHEET_MAX_SIDE {_hip.SHEET_MAX_SIDE}" in header and f"#define VRG_SHEET_STAGE_VALUES {_hip.SHEET_STAGE_VALUES}" in header


def test_fit_is_the_header_and_the_plan_is_the_host_builds(hip, hm, case_runs):
    _hip, ops, lib = hip
    got, want = np.zeros(8, np.int32), np.zeros(8, np.int32)
    for sw, sh, w, h in ((7, 5, 64, 40), (7, 5, 64, 41), (301, 7, 5, 3), (3840, 2160, 250, 140), (1, 1, 9, 9), (53, 37, 53, 20), (1920, 1080, 1, 1)):
        for cover in (0, 1):
            assert lib.vrg_sheet_fit(sw, sh, w, h, cover, got.ctypes.data) == 0
            hm.hm_sheet_fit(sw, sh, w, h, cover, want.ctypes.data)
            assert np.array_equal(got, want)
    for name, case in S.CASES.items():
        plan = ops.SheetPlan([S.SOURCES[n][:3] for n in case["sources"]], [ops.SheetPanel(**p) for p in case["panels"]], case["canvas"],
                             case["background"])
        details = case_runs[name][3]
        assert np.array_equal(np.stack([plan.records[k] for k in S.DETAILS], axis=1), details), name
        rec = plan.records.copy()
        rec["src"] = 64
        plan.check(rec, False)


def _plan(ops, **change):
    case = S.CASES["skips"]
    panels = [ops.SheetPanel(**p) for p in case["panels"]] + [ops.SheetPanel(0, (3, 3, 20, 20), "contain_pad", (1, 2, 3), 4)]
    plan = ops.SheetPlan([S.SOURCES["53x37"][:3]], panels, case["canvas"], case["background"])
    rec = plan.records.copy()
    rec["src"] = 64
    return plan, rec


def test_check_refusals(hip):
    _hip, ops, lib = hip
    plan, good = _plan(ops)

    def status(rec, tables=None, table_ints=None, n_spans=None, tmp_bytes=None, byte_sources=0):
        tables = plan.tables if tables is None else tables
        return lib.vrg_sheet_check(rec.ctypes.data, len(rec), byte_sources, tables.ctypes.data, plan.table_ints if table_ints is None else table_ints,
                                   plan.n_spans if n_spans is None else n_spans, plan.tmp_bytes if tmp_bytes is None else tmp_bytes)

    assert status(good) == 0 and status(good[:0]) == 0
    resized = int(np.nonzero(good["h_ksize"] > 0)[0][0])

    def changed(i, **fields):
        rec = good.copy()
        for k, v in fields.items():
            rec[k][i] = v
        return rec

    assert status(changed(0, src=0)) == 1                                   # a null source
    assert status(changed(0, src=66)) == 1 and status(changed(0, src=66), byte_sources=1) == 0          # fp32 sources are 4-byte aligned
    assert status(changed(0, channels=2)) == 1 and status(changed(0, channels=0)) == 1
    assert status(changed(0, channels=4)) == 0 and status(changed(0, channels=1)) == 0
    bad = plan.tables.copy()
    bad[int(good["h_table"][resized]) + 2 * int(good["new_w"][resized]) + 1] += 1
    assert status(good, tables=bad) == 1                                    # not vrg_pil_lanczos_table's weights
    assert status(changed(resized, h_ksize=int(good["h_ksize"][resized]) + 2)) == 1
    assert status(changed(resized, src_w=int(good["src_w"][resized]) + 1)) == 1                        # tables of another size
    assert status(changed(resized, h_table=plan.table_ints)) == 1           # a table outside the buffer
    cover = int(np.nonzero(good["win_x"] + good["win_y"] > 0)[0][0])
    assert status(changed(cover, win_x=int(good["new_w"][cover]))) == 1     # a window outside the resized picture
    assert status(changed(cover, win_y=-1)) == 1
    assert status(changed(2, pic_x=1)) == 1                                 # a window outside the panel
    assert status(good, tmp_bytes=plan.tmp_bytes - 1) == 1                  # a temp image outside tmp
    assert status(changed(0, tmp_offset=-1)) == 1
    assert status(good, n_spans=plan.n_spans - 1) == 1                      # mask rows outside the spans
    assert status(changed(resized, rows=int(good["rows"][resized]) - 1)) == 1 and status(changed(resized, cps=0)) == 1
    assert status(changed(0, src_w=_hip.SHEET_MAX_SIDE + 1)) == 2 and status(changed(0, w=_hip.SHEET_MAX_SIDE + 1)) == 2
    assert lib.vrg_sheet_check(None, 1, 0, plan.tables.ctypes.data, plan.table_ints, 0, 0) == 1
    assert lib.vrg_sheet_check(good.ctypes.data, -1, 0, plan.tables.ctypes.data, plan.table_ints, 0, 0) == 1


def test_limits_are_stated_and_hold(hip):
    _hip, ops, lib = hip
    # the taps of ONE column against the staging buffer: 32767 -> 5 columns is 2 * ceil(3 * 6553.4) + 1 = 39323 taps of 3 values: refused;
    # 32767 -> 16 columns of one channel is 12289 taps: taken, in segments
    with pytest.raises(RuntimeError, match="staging buffer"):
        ops.SheetPlan([(8, 32767, 3)], [ops.SheetPanel(0, (0, 0, 5, 8), "resize")], (64, 64), (0, 0, 0))
    plan = ops.SheetPlan([(8, 32767, 1)], [ops.SheetPanel(0, (0, 0, 16, 8), "resize")], (64, 64), (0, 0, 0))
    assert 1 <= int(plan.records["cps"][0]) < 16 and plan.max_segments == -(-16 // int(plan.records["cps"][0]))
    with pytest.raises(ValueError, match="32767"):
        ops.SheetPlan([(8, 8, 3)], [ops.SheetPanel(0, (0, 0, 5, 8))], (32768, 64), (0, 0, 0))
    fit = np.zeros(8, np.int32)
    assert lib.vrg_sheet_fit(32768, 8, 5, 5, 0, fit.ctypes.data) == 2 and lib.vrg_sheet_fit(0, 8, 5, 5, 0, fit.ctypes.data) == 1
    assert lib.vrg_sheet_fit(8, 8, 5, 5, 0, None) == 1
    with pytest.raises(ValueError, match="channels"):
        ops.SheetPlan([(8, 8, 2)], [ops.SheetPanel(0, (0, 0, 5, 8))], (64, 64), (0, 0, 0))


def test_launch_arguments_without_a_device(hip):
    _hip, ops, lib = hip
    null, one, two, three = None, C.c_void_p(64), C.c_void_p(128), C.c_void_p(256)
    out, odd = C.c_void_p(1024), C.c_void_p(1026)
    for entry in (lib.vrg_sheet_compose_f32, lib.vrg_sheet_compose_u8):
        assert entry(null, 0, 0, null, 0, null, 0, null, 0, null, 64, 64, 0, null) == 0                # n == 0: success without a launch
        assert entry(one, 1, 0, two, 8, null, 0, three, 8, null, 64, 64, 0, null) == 1                 # null out
        assert entry(one, 1, 0, two, 8, null, 0, three, 8, three, 64, 64, 0, null) == 1                # out is tmp
        assert entry(one, 1, 0, two, 8, null, 0, three, 8, two, 64, 64, 0, null) == 1                  # out is the tables
        assert entry(one, 1, 0, two, 8, null, 0, three, 8, one, 64, 64, 0, null) == 1                  # out is the records
        assert entry(one, 1, 0, two, 8, three, 4, C.c_void_p(512), 8, three, 64, 64, 0, null) == 1     # out is the spans
        assert entry(one, 1, 0, two, 8, null, 0, three, 8, out, 0, 64, 0, null) == 1
        assert entry(one, 1, 0, two, 8, null, 0, three, 8, out, 64, 32768, 0, null) == 2
        assert entry(one, -1, 0, two, 8, null, 0, three, 8, out, 64, 64, 0, null) == 1
        assert entry(null, 1, 0, two, 8, null, 0, three, 8, out, 64, 64, 0, null) == 1
    assert lib.vrg_sheet_compose_f32(one, 1, 0, two, 8, null, 0, three, 8, odd, 64, 64, 0, null) == 1  # misaligned fp32 out
    for entry in (lib.vrg_sheet_rows_f32, lib.vrg_sheet_rows_u8):
        assert entry(null, 0, null, 0, null, 0, 1, 1, null) == 0
        assert entry(one, 1, two, 8, null, 8, 1, 1, null) == 1 and entry(null, 1, two, 8, three, 8, 1, 1, null) == 1
        assert entry(one, 1, two, 8, two, 8, 1, 1, null) == 1 and entry(one, 1, two, 8, three, 8, -1, 1, null) == 1
        assert entry(one, 1, two, 8, three, 8, 32768, 1, null) == 2


def test_fixture_sizes():
    assert os.path.getsize(S.FIXTURE_NPZ) < 512 * 1024 and os.path.getsize(S.FIXTURE_JSON) < 512 * 1024
    doc = json.load(open(S.FIXTURE_JSON))
    assert len(doc["large_sha256"]) == 64 and set(doc["builder"]) == set(S.BUILDER_SIZES)

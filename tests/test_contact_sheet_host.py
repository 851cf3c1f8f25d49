"""The far-face repair contact sheet without a GPU: csrc/vrg_pil_resample.hpp compiled for the host (the library's host entry points) equals the
INSTALLED PILLOW byte for byte -- Image.reduce on every route, Image.resize with a BICUBIC / LANCZOS filter over a source box,
Image.thumbnail as plan + reduce + tables, and the whole sheet -- and what the reference's own contact_sheet recorded in
tests/golden/contact_sheet.npz (and gives live, where the reference checkout is readable); the C ABI of the new entry points."""
import inspect
import os
import re

import numpy as np
import pytest

import contact_sheet_support as S
from conftest import ROOT
from oracle import reference_loader as RL

NEW_SYMBOLS = ("vrg_pil_filter_ksize", "vrg_pil_filter_table", "vrg_pil_reduce_host", "vrg_thumb_plan", "vrg_thumb_plan_reduce", "vrg_thumb_check",
               "vrg_thumb_rows_u8", "vrg_thumb_compose_u8")
BACKEND = os.path.join(RL.REFERENCE_ROOT, "scripts", "far_face_repair_backend.py")


@pytest.fixture(scope="module")
def lib(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return _hip.load_library()


@pytest.fixture(scope="module")
def ffr(pkg, lib):
    from comfyui_vrgamedevgirl_amd import far_face_repair
    return far_face_repair


@pytest.fixture(scope="module")
def golden():
    return np.load(S.FIXTURE_NPZ)


@pytest.mark.parametrize("factor", S.REDUCE_FACTORS)
def test_reduce_equals_pillow(lib, golden, factor):
    Image = pytest.importorskip("PIL.Image")
    fx, fy = factor
    for k, (h, w) in enumerate(S.REDUCE_SIZES):
        img = golden[f"reduce_in.{h}x{w}"] if k < 3 else S.make_reduce_input(k)
        want = np.asarray(Image.fromarray(img, "RGB").reduce((fx, fy)))
        got = S.host_reduce(lib, img, fx, fy)
        assert got.shape == want.shape and np.array_equal(got, want), (factor, (h, w))
        if k < 3:
            assert np.array_equal(golden[f"reduce.{fx}x{fy}.{h}x{w}"], want)


# (fx, fy), then the cell (cw, ch) that is probed: the full cell of every route, the partial last column, row and corner
ROUTES = (((1, 2), (1, 2)), ((1, 3), (1, 3)), ((1, 7), (1, 7)), ((2, 1), (2, 1)), ((3, 1), (3, 1)), ((7, 1), (7, 1)), ((2, 2), (2, 2)),
          ((3, 3), (3, 3)), ((4, 4), (4, 4)), ((5, 5), (5, 5)), ((6, 6), (6, 6)), ((8, 8), (8, 8)), ((10, 10), (10, 10)), ((4, 3), (4, 3)),
          ((7, 6), (7, 6)), ((2, 2), (1, 2)), ((2, 2), (2, 1)), ((3, 3), (2, 3)), ((4, 4), (4, 2)), ((5, 5), (5, 3)), ((8, 8), (5, 8)),
          ((4, 3), (3, 3)), ((1, 3), (1, 2)), ((3, 1), (2, 1)), ((7, 6), (7, 5)))


@pytest.mark.parametrize("route", ROUTES)
def test_reduce_byte_over_every_sum_of_a_cell(lib, route):
    """one picture whose cells of (cw, ch) pixels take EVERY sum 0 .. 255 n once: Pillow's byte is pil_reduce_byte's on each route"""
    Image = pytest.importorskip("PIL.Image")
    (fx, fy), (cw, ch) = route
    n = cw * ch
    sums = np.arange(255 * n + 1)
    cells = (sums[:, None] // n + (np.arange(n)[None, :] < (sums % n)[:, None])).astype(np.uint8).reshape(-1, ch, cw)
    if (cw, ch) == (fx, fy):
        img = cells.reshape(-1, cw)
        pick = (slice(None), 0)
    elif ch == fy:                                                          # the partial last column
        img = np.zeros((len(sums) * fy, fx + cw), np.uint8)
        img[:, fx:] = cells.reshape(-1, cw)
        pick = (slice(None), 1)
    else:                                                                   # the partial last row
        img = np.zeros((fy + ch, len(sums) * fx), np.uint8)
        img[fy:] = cells.transpose(1, 0, 2).reshape(ch, -1)
        pick = (1, slice(None))
    want = np.asarray(Image.fromarray(img, "L").reduce((fx, fy)))[pick]
    got = S.host_reduce(lib, img[:, :, None], fx, fy)[:, :, 0][pick]
    assert np.array_equal(got, want)
    assert np.array_equal(got, ((sums + n // 2) * ((1 << 24) // n)) >> 24)


def test_reduce_corner_cell_equals_pillow(lib):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for (fx, fy), (cw, ch) in (((3, 3), (2, 2)), ((3, 3), (1, 2)), ((4, 4), (3, 1)), ((4, 3), (3, 2)), ((7, 6), (5, 4)), ((2, 2), (1, 1))):
        for _ in range(40):
            img = rng.integers(0, 256, (fy + ch, fx + cw, 3), dtype=np.uint8)
            img[fy:, fx:] = rng.choice([0, 255, int(rng.integers(0, 256))])
            assert np.array_equal(S.host_reduce(lib, img, fx, fy), np.asarray(Image.fromarray(img, "RGB").reduce((fx, fy))))


BOX_CASES = (((41, 67), (20, 13), (67.0, 41.0)), ((41, 67), (20, 13), (67 / 4, 41 / 4)), ((41, 67), (90, 70), (67 / 3, 41 / 3)),
             ((30, 50), (50, 30), (49.5, 30.0)), ((30, 50), (17, 30), (50.0, 29.25)), ((64, 64), (7, 5), (64 / 3, 64 / 7)),
             ((9, 17), (40, 33), (16.5, 8.75)))


@pytest.mark.parametrize("case", BOX_CASES)
@pytest.mark.parametrize("resample", (S.BICUBIC, S.LANCZOS))
def test_filter_tables_equal_pillow_resize_with_a_box(lib, ffr, case, resample):
    Image = pytest.importorskip("PIL.Image")
    (h, w), size, (bw, bh) = case
    img = S.random_image(300 + BOX_CASES.index(case), h, w)
    want = np.asarray(Image.fromarray(img, "RGB").resize(size, Image.Resampling(resample), box=(0, 0, bw, bh)))
    assert np.array_equal(S.host_box_resize(lib, img, size, resample, bw, bh), want)
    name = "bicubic" if resample == S.BICUBIC else "lanczos"
    ksize, table = ffr.filter_table(name, w, 0.0, bw, size[0])
    bounds, weights = S.host_table(lib, resample, w, 0.0, bw, size[0])
    assert ksize == weights.shape[1]
    assert np.array_equal(table[:2 * size[0]].reshape(-1, 2), bounds) and np.array_equal(table[2 * size[0]:].reshape(size[0], ksize), weights)


def test_filter_table_with_the_whole_axis_is_the_lanczos_table(ffr):
    for n_in, n_out in ((33, 90), (128, 37), (300, 7)):
        ksize, table = ffr.filter_table("lanczos", n_in, 0.0, float(n_in), n_out)
        k0, t0 = ffr.lanczos_table(n_in, n_out)
        assert ksize == k0 and np.array_equal(table, t0)
    with pytest.raises(ValueError):
        ffr.filter_table("nearest", 10, 0.0, 10.0, 5)
    with pytest.raises(ValueError):
        ffr.filter_table("bicubic", 10, 0.0, 10.5, 5)


AXIS_SIZES = (1, 2, 3, 5, 7, 13, 16, 31, 64, 127, 256, 1009, 4096, 32767)        # 1, 2, 3, primes, powers of two, the largest side


def test_the_lanczos_exports_are_the_filter_exports_over_the_whole_axis(lib):
    """vrg_pil_lanczos_ksize / _table == vrg_pil_filter_ksize / _table with filter 1 and the box (0, n_in), up- and down-scaling, every
    pair of AXIS_SIZES but 32767 -> 32767 (229 K rows of the same rule as 4096 -> 4096)"""
    import ctypes as C
    for n_in in AXIS_SIZES:
        for n_out in AXIS_SIZES:
            if n_in == n_out == 32767:
                continue
            ksize = lib.vrg_pil_lanczos_ksize(n_in, n_out)
            assert ksize == lib.vrg_pil_filter_ksize(S.LANCZOS, 0.0, float(n_in), n_out) and ksize >= 7, (n_in, n_out)
            bounds, weights = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ksize), np.int32)
            assert lib.vrg_pil_lanczos_table(n_in, n_out, C.c_void_p(bounds.ctypes.data), C.c_void_p(weights.ctypes.data)) == 0
            b1, w1 = S.host_table(lib, S.LANCZOS, n_in, 0.0, float(n_in), n_out)
            assert np.array_equal(bounds, b1) and np.array_equal(weights, w1), (n_in, n_out)


def test_the_whole_axis_table_does_not_round_its_length_to_float(lib):
    """n_in = 2^24 + 1 is no C float: rounded to one it gives ksize 98305, exact 98307.  The table (n_out (2 + ksize) int32, 403 MB -- six
    ints per source pixel whatever n_out, so the fixture holds its SHA-256, its bounds and every 4099th weight, recorded from the library
    before vrg_pil_lanczos_table became a call of the one builder: tools/make_golden_pil_axis.py)"""
    import ctypes as C
    import hashlib
    rec = np.load(os.path.join(ROOT, "tests", "golden", "pil_lanczos_axis.npz"))
    n_in, n_out, ksize = (int(v) for v in rec["sizes"])
    assert n_in == (1 << 24) + 1 and float(np.float32(n_in)) != n_in
    assert lib.vrg_pil_lanczos_ksize(n_in, n_out) == ksize == 98307
    assert lib.vrg_pil_filter_ksize(S.LANCZOS, 0.0, float(np.float32(n_in)), n_out) == 98305          # what a float box gives
    table = np.zeros(n_out * (2 + ksize), np.int32)
    assert lib.vrg_pil_lanczos_table(n_in, n_out, C.c_void_p(table.ctypes.data), C.c_void_p(table[2 * n_out:].ctypes.data)) == 0
    assert np.array_equal(table[:2 * n_out].reshape(-1, 2), rec["bounds"])
    assert np.array_equal(table[2 * n_out::int(rec["stride"])], rec["weights"])
    assert hashlib.sha256(table).hexdigest() == str(rec["sha256"])


@pytest.mark.parametrize("index", range(len(S.THUMB_CASES)))
def test_thumbnail_equals_pillow(lib, golden, index):
    Image = pytest.importorskip("PIL.Image")
    _, request, resample, gap = S.THUMB_CASES[index]
    img = S.thumb_input(golden, index)
    assert img.shape[:2] == S.THUMB_CASES[index][0]
    im = Image.fromarray(img, "RGB")
    im.thumbnail(request, Image.Resampling(resample), reducing_gap=gap)
    got, _ = S.host_thumbnail(lib, img, request, resample, gap)
    assert got.shape == np.asarray(im).shape and np.array_equal(got, np.asarray(im))
    assert np.array_equal(golden[f"thumb.{index}"], got)


def test_thumbnail_cases_cover_the_plan():
    """nothing to do, one factor above 1 only, fx != fy, no reduce"""
    import comfyui_vrgamedevgirl_amd._hip as _hip
    lib = _hip.load_library()
    seen = set()
    for (h, w), request, resample, gap in S.THUMB_CASES:
        rc, e, _ = S.host_plan(lib, [(h, w)], [request], resample, gap)
        assert rc == 0
        e = e[0]
        seen.add("nothing" if (e["out_w"], e["out_h"], e["h_ksize"], e["v_ksize"]) == (w, h, 0, 0) else
                 "one" if min(e["fx"], e["fy"]) == 1 < max(e["fx"], e["fy"]) else "unequal" if e["fx"] != e["fy"] else "equal")
    assert seen == {"nothing", "one", "unequal", "equal"}


@pytest.mark.parametrize("key", sorted(S.SHEET_CASES))
def test_sheet_equals_the_reference(lib, golden, key):
    originals, fixed, limit, columns, thumb_width = S.sheet_case(golden, key)
    case = S.SHEET_CASES[key]
    assert (limit, columns, thumb_width) == (case["limit"], case["columns"], case["thumb_width"])
    got, factors = S.host_sheet(lib, originals, fixed, limit, columns, thumb_width)
    want = golden[f"sheet.{key}"]
    assert got.shape == want.shape and np.array_equal(got, want)
    if key in S.SHEET_FACTORS:
        assert factors[0] == S.SHEET_FACTORS[key]
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    assert np.array_equal(S.pillow_sheet(originals, fixed, limit, columns, thumb_width), want)


def test_the_fixture_holds_the_inputs_the_tool_makes(golden):
    """the stored frames are the seeded ones the tool makes, so that the fixture can be made again"""
    for key in S.SHEET_CASES:
        originals, fixed, _, _, _ = S.sheet_case(golden, key)
        made_o, made_f = S.make_sheet_inputs(key)
        assert len(originals) == len(made_o) and all(np.array_equal(a, b) for a, b in zip(originals, made_o))
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(fixed, made_f))


@pytest.mark.skipif(not os.path.isfile(BACKEND), reason="no reference checkout (oracle.reference_loader.REFERENCE_ROOT)")
def test_sheet_equals_the_reference_run_live(lib, golden):
    pytest.importorskip("PIL")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_contact_sheet", os.path.join(ROOT, "tools", "make_golden_contact_sheet.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    run = tool.reference_contact_sheet()
    for key in sorted(S.SHEET_CASES):
        originals, fixed, limit, columns, thumb_width = S.sheet_case(golden, key)
        live = run(originals, fixed, limit, columns, thumb_width)
        assert np.array_equal(live, golden[f"sheet.{key}"])
        assert np.array_equal(S.host_sheet(lib, originals, fixed, limit, columns, thumb_width)[0], live)


def test_plan_layout_and_refusals(lib):
    rc, e, sheet = S.host_plan(lib, [(54, 96)] * 5, [(47, 13)] * 5, columns=3, pair=True)
    assert rc == 0 and sheet[:2] == (3, 2) and sheet[2:4] == (int(e[0]["out_w"]), int(e[0]["out_h"]))
    assert [(int(x["dst_x"]), int(x["dst_y"])) for x in e] == [((i % 3) * sheet[2], (i // 3) * sheet[3]) for i in range(5)]
    assert S.host_plan(lib, [(54, 96)], [(47, 13)], columns=0, pair=True)[2][:2] == (1, 1)          # max(1, columns)
    assert S.host_plan(lib, [(8, 2600)], [(10, 1)], pair=True)[0] == 2                               # a factor of 260: unsupported
    assert S.host_plan(lib, [(2000, 4)], [(2, 300)])[0] == 2                                         # more than 100 times as tall as wide
    assert S.host_plan(lib, [(54, 96)], [(47, 0.5)])[0] == 1 and S.host_plan(lib, [(54, 96)], [(47, 13)], gap=0.5)[0] == 1
    assert S.host_plan(lib, [(54, 96)], [(47, 13)], resample=2)[0] == 1


# reducing_gap, (h, w) whose REDUCED picture is exactly 100 times as tall as wide, the request, the factors, the height one reduced row taller
TALL_CASES = ((None, (200, 2), (2, 50), (1, 1), 201), (None, (300, 3), (3, 75), (1, 1), 301), (2.0, (400, 4), (4, 100), (2, 2), 402),
              (2.0, (400, 6), (6, 100), (3, 2), 402))


@pytest.mark.parametrize("case", TALL_CASES)
def test_the_tall_picture_rule_at_its_boundary(lib, case):
    """Image.resize goes vertically first when the (reduced) picture's height is MORE than 100 times its width and the height shrinks:
    at exactly 100 times the horizontal-first tables still equal Pillow, one reduced row more is refused"""
    Image = pytest.importorskip("PIL.Image")
    gap, (h, w), request, want_factors, taller = case
    img = S.random_image(40 + TALL_CASES.index(case), h, w)
    im = Image.fromarray(img, "RGB")
    im.thumbnail(request, reducing_gap=gap)
    got, factors = S.host_thumbnail(lib, img, request, S.BICUBIC, gap)
    assert factors == want_factors and got.shape == np.asarray(im).shape and np.array_equal(got, np.asarray(im))
    assert S.host_plan(lib, [(taller, w)], [request], S.BICUBIC, gap)[0] == 2


def test_abi_of_the_new_entry_points(pkg, lib):
    from comfyui_vrgamedevgirl_amd import _hip, far_face_repair
    with open(os.path.join(ROOT, "include", "vrgdg_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define VRG_ABI_VERSION 8\b", header) and _hip.ABI_VERSION == 8 and lib.vrg_abi_version() == 8
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _hip.EXPORTED_SYMBOLS and name not in _hip.DEBUG_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert "typedef struct vrg_thumb_entry" in header
    fields = re.search(r"typedef struct vrg_thumb_entry \{(.*?)\} vrg_thumb_entry;", header, re.S).group(1)
    declared = [n.strip() for kind, names in re.findall(r"(int64_t|int32_t) ([^;]+);", fields) for n in names.split(",")]
    assert declared == [n for n, _ in _hip.ThumbEntry._fields_] == list(far_face_repair._THUMB_ENTRY.names)
    assert "contact_sheet" in inspect.getdoc(far_face_repair) and "``contact_sheet`` and ``rebuild_video`` are out of scope" not in \
        inspect.getdoc(far_face_repair)

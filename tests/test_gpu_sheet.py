"""Reference sheets on the GPU (csrc/vrg_sheet.hip through ops.reference_sheet, the node and the Builder functions): byte-equal and
bit-equal to the canvases the reference recorded (tests/golden/sheet.{json,npz}), to the header compiled for the host and to plain Pillow.
Shapes are the smallest that reach every path: see tests/sheet_support.py and tests/test_sheet_host.py, which asserts what the case list
covers.  A view that is not contiguous is made contiguous by the operator (a copy); inputs are never written."""
import hashlib
import json

import numpy as np
import pytest
import torch

import sheet_support as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_LTXICIngredientsGrid as grid
    from comfyui_vrgamedevgirl_amd import VRGDG_MusicVideoBuilderNodes as builder
    from comfyui_vrgamedevgirl_amd import ops
    return ops, grid, builder


@pytest.fixture(scope="module")
def golden():
    with open(S.FIXTURE_JSON) as fh:
        return json.load(fh), np.load(S.FIXTURE_NPZ)


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return S.build_host_lib(tmp_path_factory.mktemp("sheet_check_gpu"))


def panels_of(ops, case):
    return [ops.SheetPanel(**p) for p in case["panels"]]


def unit(u8):
    return u8.astype(np.float32) / np.float32(255)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_small_cases_equal_the_host_build_and_pillow(mods, hm, name):
    ops = mods[0]
    case = S.CASES[name]
    host = [S.source(n) for n in case["sources"]]
    rc, want, want_f, _ = S.host_sheet(hm, host, case["panels"], case["canvas"], case["background"])
    assert rc == 0
    dev = [torch.from_numpy(a).cuda() for a in host]
    before = [d.clone() for d in dev]
    f32 = ops.reference_sheet(dev, panels_of(ops, case), case["canvas"], case["background"])
    u8 = ops.reference_sheet(dev, panels_of(ops, case), case["canvas"], case["background"], out_bytes=True)
    assert f32.dtype == torch.float32 and u8.dtype == torch.uint8 and tuple(f32.shape) == (case["canvas"][1], case["canvas"][0], 3)
    assert np.array_equal(u8.cpu().numpy(), want)
    assert np.array_equal(f32.cpu().numpy().view(np.uint32), want_f.view(np.uint32))                 # float == byte / 255, bit for bit
    assert np.array_equal(f32.cpu().numpy().view(np.uint32), unit(u8.cpu().numpy()).view(np.uint32))
    assert np.array_equal(want, S.pillow_sheet([S.quantise(a) for a in host], case["panels"], case["canvas"], case["background"]))
    assert all(torch.equal(a, b) for a, b in zip(dev, before))                                        # inputs are never written
    # host-fed and byte sources give the same sheet
    fed = ops.reference_sheet([torch.from_numpy(a) for a in host], panels_of(ops, case), case["canvas"], case["background"], out_bytes=True)
    assert np.array_equal(fed.cpu().numpy(), want)
    if name != "special":
        byte_sources = [torch.from_numpy(S.quantise(a) if a.shape[2] != 1 else S.quantise(a)[..., :1].copy()).cuda() for a in host]
        assert np.array_equal(ops.reference_sheet(byte_sources, panels_of(ops, case), case["canvas"], case["background"], out_bytes=True).cpu().numpy(), want)


def test_nan_gives_zero(mods):
    ops = mods[0]
    a = S.source("53x37").copy()
    a[3, 5, 1] = np.nan
    a[36, 52, :] = np.nan
    got = ops.reference_sheet([torch.from_numpy(a).cuda()], [ops.SheetPanel(0, (0, 0, 53, 37))], (53, 37), (9, 9, 9), out_bytes=True).cpu().numpy()
    want = S.quantise(np.nan_to_num(a, nan=0.0))
    assert np.array_equal(got, want) and got[3, 5, 1] == 0 and not got[36, 52].any()


def test_views_are_made_contiguous_and_offsets_off_the_vector_grid(mods, hm):
    ops = mods[0]
    big = torch.from_numpy(np.concatenate([np.zeros((37, 1, 3), np.float32), S.source("53x37"), np.ones((37, 2, 3), np.float32)], axis=1)).cuda()
    view = big[:, 1:54]                                                      # rows 56 floats apart, starting one pixel in
    assert not view.is_contiguous()
    case = S.CASES["skips"]
    rc, want, _f, _d = S.host_sheet(hm, [S.source("53x37")], case["panels"], case["canvas"], case["background"])
    keep = big.clone()
    got = ops.reference_sheet([view], panels_of(ops, case), case["canvas"], case["background"], out_bytes=True)
    assert rc == 0 and np.array_equal(got.cpu().numpy(), want) and torch.equal(big, keep)
    flat = torch.zeros(37 * 53 * 3 + 1, device="cuda")                       # a contiguous source one float off the 16-byte grid
    flat[1:] = torch.from_numpy(S.source("53x37")).cuda().reshape(-1)
    got = ops.reference_sheet([flat[1:].reshape(37, 53, 3)], panels_of(ops, case), case["canvas"], case["background"], out_bytes=True)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", sorted(S.NODE_CASES))
def test_node_equals_the_reference(mods, golden, name):
    ops, grid, _ = mods
    case = S.NODE_CASES[name]
    inputs = {k: torch.from_numpy(v) for k, v in S.node_inputs(case).items()}
    before = {k: v.clone() for k, v in inputs.items()}
    node = grid.VRGDG_LTXICIngredientsGrid()
    (out,) = node.build(**case, **inputs)
    want = golden[1][f"node.{name}"]
    assert out.device.type == "cpu" and out.dtype == torch.float32 and tuple(out.shape) == (1, *want.shape)
    assert np.array_equal(out[0].numpy().view(np.uint32), unit(want).view(np.uint32))
    with torch.inference_mode():
        (again,) = node.build(**case, **{k: v.clone() for k, v in inputs.items()})
    (on_device,) = node.build(**case, **{k: v.cuda() for k, v in inputs.items()})
    assert on_device.is_cuda and torch.equal(again, out) and torch.equal(on_device.cpu(), out)
    assert all(torch.equal(inputs[k], before[k]) for k in inputs)
    if name == "all_images":
        assert len(golden[0]["panels"][name]) == 27


def test_large_case_by_digest(mods, golden):
    _ops, grid, _ = mods
    inputs = {k: torch.from_numpy(v).cuda() for k, v in S.large_inputs().items()}
    (out,) = grid.VRGDG_LTXICIngredientsGrid().build(**S.LARGE_CASE, **inputs)
    b = torch.round(out[0] * 255.0).to(torch.uint8).cpu().numpy()
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), unit(b).view(np.uint32))
    assert hashlib.sha256(np.ascontiguousarray(b).tobytes()).hexdigest() == golden[0]["large_sha256"]


@pytest.mark.parametrize("key", sorted(S.BUILDER_SIZES))
def test_builder_sheets_equal_the_reference(mods, golden, key):
    from PIL import Image
    _ops, _grid, builder = mods
    arrays = S.builder_inputs(key)
    keep = [a.copy() for a in arrays]
    if key == "subject_location":
        out = builder.combine_subject_location_images(Image.fromarray(arrays[0]), arrays[1])
    elif key.startswith("flux"):
        out = builder.combine_flux_ingredient_images(arrays)
    else:
        out = builder.combine_story_reference_batch([Image.fromarray(a) for a in arrays])
    got = np.asarray(out)
    rec = golden[0]["builder"][key]
    assert list(out.size) == rec["size"] and out.mode == "RGB"
    assert np.array_equal(got[::7, ::5], golden[1][f"builder.{key}"])
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == rec["sha256"]
    assert all(np.array_equal(a, b) for a, b in zip(arrays, keep))


# ------------------------------------------------------------------------------------------------
# the flat piece writer and the byte staging at their edges.  Before these, every `out` was torch's own allocation (16-byte aligned: no
# lead) and the smallest canvas 16 x 9; byte sources came in whole tensors (phase 0) or, in fp32 only, one float off the grid.
# ------------------------------------------------------------------------------------------------
def compose_at(ops, sources, case, out_bytes, lead):
    """the two launches through the C ABI with `out` starting `lead` ELEMENTS into a larger buffer -> (canvas, the buffer, its fill)"""
    from comfyui_vrgamedevgirl_amd import _hip
    lib = _hip.lib()
    panels = panels_of(ops, case)
    width, height = case["canvas"]
    plan = ops.SheetPlan([tuple(s.shape) for s in sources], panels, case["canvas"], case["background"])
    byte_sources = sources[0].dtype == torch.uint8
    rec = plan.records.copy()
    for i, p in enumerate(panels):
        rec["src"][i] = sources[p.source].data_ptr()
    plan.check(rec, byte_sources)
    d = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
    tables, spans = torch.from_numpy(plan.tables).cuda(), torch.from_numpy(plan.spans).cuda()
    tmp = torch.empty(max(plan.tmp_bytes, 1), dtype=torch.uint8, device="cuda")
    total = height * width * 3
    fill = 0xA5 if out_bytes else -7.0
    big = torch.full((total + 64,), fill, dtype=torch.uint8 if out_bytes else torch.float32, device="cuda")
    out = big[lead:lead + total]
    assert out.data_ptr() % 16 == (lead * big.element_size()) % 16
    rows = lib.vrg_sheet_rows_u8 if byte_sources else lib.vrg_sheet_rows_f32
    compose = lib.vrg_sheet_compose_u8 if out_bytes else lib.vrg_sheet_compose_f32
    assert rows(_hip.ptr(d), len(rec), _hip.ptr(tables), plan.table_ints, _hip.ptr(tmp), plan.tmp_bytes, plan.max_segments, plan.max_rows,
                _hip.current_stream()) == 0
    r, g, b = plan.background
    assert compose(_hip.ptr(d), len(rec), int(byte_sources), _hip.ptr(tables), plan.table_ints, _hip.ptr(spans), plan.n_spans, _hip.ptr(tmp),
                   plan.tmp_bytes, _hip.ptr(out), width, height, r | (g << 8) | (b << 16), _hip.current_stream()) == 0
    torch.cuda.synchronize()
    host = big.cpu().numpy()
    around = np.concatenate([host[:lead], host[lead + total:]])
    assert len(around) == 64 and (around == host.dtype.type(fill)).all(), "bytes around the canvas were written"
    return host[lead:lead + total].reshape(height, width, 3)


def one_panel(canvas, fit="contain_pad"):
    return {"sources": ["53x37"], "canvas": canvas, "background": (9, 200, 31),
            "panels": [S.P(0, (0, 0, canvas[0], canvas[1]), fit, (1, 2, 3), 0)]}


# (canvas, elements in front of `out`, as bytes / as floats): 3 and 12 elements end before the first 16-byte boundary or one piece
# (pieces == 0, lead clamped to total); 3 x 3 = 27 elements: bytes 5 in -> lead 11, 16 left: no tail; 6 in -> lead 10, 17 left: a tail of
# one; floats 1 in -> lead 3, 24 left: no tail; 2 in -> lead 2, 25 left: a tail of one.  A float canvas starts on a float: 0, 1, 3 floats
# in are bytes 0, 4, 12.
FLAT_CASES = [((1, 1), (0, 1, 15), (0, 1, 3)), ((2, 2), (0, 1, 15), (0, 1, 3)), ((3, 3), (5, 6), (1, 2))]


@pytest.mark.parametrize("canvas,byte_leads,float_leads", FLAT_CASES)
def test_canvases_around_one_piece_at_every_lead(mods, hm, canvas, byte_leads, float_leads):
    ops = mods[0]
    case = one_panel(canvas)
    host = [S.source(n) for n in case["sources"]]
    rc, want, want_f, _ = S.host_sheet(hm, host, case["panels"], case["canvas"], case["background"])
    assert rc == 0 and np.array_equal(want, S.pillow_sheet([S.quantise(a) for a in host], case["panels"], case["canvas"], case["background"]))
    dev = [torch.from_numpy(a).cuda() for a in host]
    for lead in byte_leads:
        assert np.array_equal(compose_at(ops, dev, case, True, lead), want), lead
    for lead in float_leads:
        assert np.array_equal(compose_at(ops, dev, case, False, lead).view(np.uint32), want_f.view(np.uint32)), lead


def at_phase(array, phase):
    """a dense device copy of a uint8 array whose first byte lies at an address = phase (mod 16)"""
    buf = torch.zeros(array.size + 32, dtype=torch.uint8, device="cuda")
    view = buf[phase:phase + array.size].view(array.shape)
    view.copy_(torch.from_numpy(array))
    assert view.data_ptr() % 16 == phase and view.is_contiguous()
    return view


# (height, width, channels, phase of the first byte).  One channel, two pixels at 13: n = 2 < head = 3.  Three channels, two pixels, eight
# rows from 13: the rows lie at 13, 3, 9, 15, 5, 11, 1, 7 -- at 9 n = 6 < head = 7.  Two pixels at 10 and six pixels at 14 end on a
# 16-byte boundary (head == n, and head 2 + one whole piece, no tail).
STAGED = [(8, 2, 1, 13), (8, 2, 3, 13), (1, 2, 3, 10), (1, 6, 3, 14)]


@pytest.mark.parametrize("shape", STAGED)
def test_byte_sources_staged_from_short_and_boundary_segments(mods, hm, shape):
    ops = mods[0]
    h, w, c, phase = shape
    src = np.random.default_rng(sum(shape)).integers(0, 256, (h, w, c), dtype=np.uint8)
    rgb = np.repeat(src, 3, axis=2) if c == 1 else src
    for canvas, fit in (((5, h), "resize"), ((w, 2 * h), "resize"), ((7, 11), "cover_crop")):         # taps over the row; the row itself; a window
        case = {"sources": [None], "canvas": canvas, "background": (0, 0, 0), "panels": [S.P(0, (0, 0, canvas[0], canvas[1]), fit, (4, 5, 6), 0)]}
        rc, want, _f, _d = S.host_sheet(hm, [src], case["panels"], canvas, case["background"])
        assert rc == 0 and np.array_equal(want, S.pillow_sheet([rgb], case["panels"], canvas, case["background"]))
        got = ops.reference_sheet([at_phase(src, phase)], panels_of(ops, case), canvas, case["background"], out_bytes=True)
        assert np.array_equal(got.cpu().numpy(), want), (canvas, fit)

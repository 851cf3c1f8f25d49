"""The far-face repair contact sheet on the GPU (comfyui-vrgamedevgirl_amd/far_face_repair.py: contact_sheet, pil_thumbnail, pil_reduce;
csrc/vrg_thumb.hip): sheets, thumbnails and reduced pictures equal what the reference's own contact_sheet and the installed Pillow recorded
in tests/golden/contact_sheet.npz byte for byte -- and Pillow itself where it is importable."""
import ctypes as C

import numpy as np
import pytest
import torch

import contact_sheet_support as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ffr(pkg):
    from comfyui_vrgamedevgirl_amd import far_face_repair
    return far_face_repair


@pytest.fixture(scope="module")
def golden():
    return np.load(S.FIXTURE_NPZ)


def _differs(got, want):
    return got.shape, want.shape, int(np.abs(got.astype(int) - want.astype(int)).max()) if got.shape == want.shape else None


@pytest.mark.parametrize("key", sorted(S.SHEET_CASES))
def test_sheet_equals_the_reference(ffr, golden, key):
    """lists of numpy frames (uploaded) and lists of device tensors (read where they lie), fixed frames missing and of other sizes"""
    originals, fixed, limit, columns, thumb_width = S.sheet_case(golden, key)
    case = dict(limit=limit, columns=columns, thumb_width=thumb_width)
    want = golden[f"sheet.{key}"]
    got = ffr.contact_sheet(originals, fixed, case["limit"], case["columns"], case["thumb_width"])
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    assert got.shape == want.shape and np.array_equal(got, want), _differs(got, want)
    dev = ffr.contact_sheet([torch.from_numpy(o).cuda() for o in originals], [None if f is None else torch.from_numpy(f).cuda() for f in fixed],
                            limit=case["limit"], columns=case["columns"], thumb_width=case["thumb_width"])
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    assert np.array_equal(S.pillow_sheet(originals, fixed, case["limit"], case["columns"], case["thumb_width"]), want)


def test_sheet_of_batch_tensors_without_fixed_frames_and_off_the_16_byte_grid(ffr, golden):
    """[n, H, W, 3] tensors on the CPU and on the device; fixed=None pairs every original with itself; a dense view that starts 5 bytes
    into its buffer is read in place"""
    originals, fixed, _, columns, thumb_width = S.sheet_case(golden, "f2")
    case = dict(columns=columns, thumb_width=thumb_width)
    o, f = np.stack(originals), np.stack(fixed)
    want = golden["sheet.f2"]
    cpu = ffr.contact_sheet(torch.from_numpy(o), torch.from_numpy(f), columns=case["columns"], thumb_width=case["thumb_width"])
    assert isinstance(cpu, torch.Tensor) and not cpu.is_cuda and np.array_equal(cpu.numpy(), want)
    for lead in (5, 16, 3):
        views = []
        for a in (o, f):
            buf = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda")
            buf[lead:lead + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
            views.append(buf[lead:lead + a.size].view(a.shape))
        assert views[0].data_ptr() % 16 == lead % 16 and views[0].is_contiguous()
        dev = ffr.contact_sheet(views[0], views[1], columns=case["columns"], thumb_width=case["thumb_width"])
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want), lead
    alone = ffr.contact_sheet(torch.from_numpy(o).cuda(), None, columns=case["columns"], thumb_width=case["thumb_width"])
    assert np.array_equal(alone.cpu().numpy(), S.host_sheet(ffr._host(), originals, [None] * len(originals), 24, case["columns"],
                                                            case["thumb_width"])[0])
    strided = torch.from_numpy(np.concatenate([o, o], axis=2)).cuda()[:, :, :o.shape[2]]           # not dense: copied first
    assert np.array_equal(ffr.contact_sheet(strided, torch.from_numpy(f).cuda(), columns=case["columns"],
                                            thumb_width=case["thumb_width"]).cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="No frames were available for the contact sheet."):
        ffr.contact_sheet(torch.from_numpy(o).cuda(), limit=0)
    with pytest.raises(RuntimeError, match="No frames were available for the contact sheet."):
        ffr.contact_sheet([])


def test_thumbnails_equal_pillow(ffr, golden):
    """every thumbnail case as a list of images of differing sizes per (resample, reducing_gap), on the device and from arrays"""
    groups = {}
    for i, (_, request, resample, gap) in enumerate(S.THUMB_CASES):
        groups.setdefault((request, resample, gap), []).append(i)
    for (request, resample, gap), members in groups.items():
        name = "bicubic" if resample == S.BICUBIC else "lanczos"
        images = [S.thumb_input(golden, i) for i in members]
        got = ffr.pil_thumbnail([torch.from_numpy(a).cuda() for a in images], request, name, gap)
        listed = ffr.pil_thumbnail(images, request, resample=name, reducing_gap=gap)
        for i, g, l in zip(members, got, listed):
            want = golden[f"thumb.{i}"]
            assert g.is_cuda and tuple(g.shape) == want.shape and np.array_equal(g.cpu().numpy(), want), (i, _differs(g.cpu().numpy(), want))
            assert isinstance(l, np.ndarray) and np.array_equal(l, want)
    batch = torch.from_numpy(np.stack([S.thumb_input(golden, 4), S.thumb_input(golden, 4)[::-1].copy()]))
    out = ffr.pil_thumbnail(batch, S.THUMB_CASES[4][1])
    assert not out.is_cuda and tuple(out.shape) == (2,) + golden["thumb.4"].shape and np.array_equal(out[0].numpy(), golden["thumb.4"])


@pytest.mark.parametrize("factor", S.REDUCE_FACTORS)
def test_reduce_equals_pillow(ffr, golden, factor):
    fx, fy = factor
    images = [golden[f"reduce_in.{h}x{w}"] for h, w in S.REDUCE_SIZES[:3]]
    got = ffr.pil_reduce([torch.from_numpy(a).cuda() for a in images], factor)
    for (h, w), g in zip(S.REDUCE_SIZES[:3], got):
        want = golden[f"reduce.{fx}x{fy}.{h}x{w}"]
        assert tuple(g.shape) == want.shape and np.array_equal(g.cpu().numpy(), want), (factor, (h, w), _differs(g.cpu().numpy(), want))
    if fx == fy:
        assert np.array_equal(ffr.pil_reduce(images[:1], fx)[0], golden[f"reduce.{fx}x{fy}.40x64"])


def test_wide_rows_take_several_segments(ffr):
    """a row wider than the staging buffer: more than one segment per row, with factors and without"""
    lib = ffr._host()
    img = S.random_image(77, 9, 3000)
    plan = ffr.ThumbPlan([torch.from_numpy(img).cuda()], None, [(700, 9)], torch.device("cuda", torch.cuda.current_device()))
    assert plan.max_segments > 1 and int(plan.entries_host[0]["fx"]) == 2
    for request, gap in (((700, 9), 2.0), ((2900, 9), 2.0), ((700, 9), None)):
        got = ffr.pil_thumbnail([img], request, reducing_gap=gap)[0]
        want, _ = S.host_thumbnail(lib, img, request, S.BICUBIC, gap)
        assert got.shape == want.shape and np.array_equal(got, want), (request, gap, _differs(got, want))
    assert np.array_equal(ffr.pil_reduce([img], (1, 2))[0], S.host_reduce(lib, img, 1, 2))


def test_a_refused_geometry_is_unsupported_without_a_launch(ffr):
    from comfyui_vrgamedevgirl_amd import _hip
    strip = torch.zeros((140, 1300, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        ffr.contact_sheet([strip], thumb_width=20)                            # 19 x 1 of 2600 x 140: int(2600 / 19 / 2.0) = 68 > VRG_THUMB_MAX_FACTOR
    with pytest.raises(RuntimeError, match="unsupported"):
        ffr.pil_reduce([strip], 65)
    rc, entries, _ = S.host_plan(ffr._host(), [(8, 2600)], [(10, 1)], pair=True)
    assert rc == 2
    # the launches themselves refuse what they cannot hold, and an entry that is not the plan's pastes nothing: the canvas colour alone
    out = torch.zeros((4, 8, 3), dtype=torch.uint8, device="cuda")
    tmp = torch.zeros(64, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(C.sizeof(_hip.ThumbEntry), dtype=torch.uint8, device="cuda")
    assert _hip.lib().vrg_thumb_rows_u8(_hip.ptr(strip), strip.numel(), _hip.ptr(bad), 1, None, 0, _hip.ptr(tmp), 64, 40000, 1,
                                        _hip.current_stream()) == 2
    assert _hip.lib().vrg_thumb_compose_u8(_hip.ptr(bad), 1, None, 0, _hip.ptr(tmp), 64, _hip.ptr(out), 8, 4, 1, 8, 4, 24 | 24 << 8 | 24 << 16,
                                           _hip.current_stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == 24).all())


# ------------------------------------------------------------------------------------------------
# the flat piece writer and the byte staging at their edges.  Before these, every sheet was torch's own allocation (16-byte aligned: no
# lead) and the smallest one 24 x 6; sources off the 16-byte grid (5, 16, 3 above) were 40 pixels wide or more: never n < head, and no
# pair had a left run of one pixel.
# ------------------------------------------------------------------------------------------------
def at_phase(array, phase):
    """a dense device copy of a uint8 array whose first byte lies at an address = phase (mod 16)"""
    buf = torch.zeros(array.size + 32, dtype=torch.uint8, device="cuda")
    view = buf[phase:phase + array.size].view(array.shape)
    view.copy_(torch.from_numpy(array))
    assert view.data_ptr() % 16 == phase and view.is_contiguous()
    return view


def sheet_at(ffr, lefts, rights, lead, requests=None, factors=None):
    """the two launches of a ThumbPlan with the sheet starting `lead` bytes into a larger buffer; the bytes around it must stay"""
    plan = ffr.ThumbPlan(lefts, rights, requests, torch.device("cuda", torch.cuda.current_device()), factors=factors)
    total = plan.height * plan.width * 3
    big = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.out = big[lead:lead + total].view(plan.height, plan.width, 3)
    assert plan.out.data_ptr() % 16 == lead % 16
    plan.run_rows()
    plan.run_compose()
    torch.cuda.synchronize()
    host = big.cpu().numpy()
    assert (host[:lead] == 0xA5).all() and (host[lead + total:] == 0xA5).all(), "bytes around the sheet were written"
    return host[lead:lead + total].reshape(plan.height, plan.width, 3)


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def pillow_thumbnail(img, request):
    from PIL import Image
    im = Image.fromarray(img, "RGB")
    im.thumbnail(request, Image.Resampling.BICUBIC, reducing_gap=2.0)
    return np.asarray(im)


# (picture h x w, the size asked for, leads).  1 x 1 and 2 x 2 sheets (3 and 12 bytes) end before the first 16-byte boundary or one piece: pieces == 0,
# lead clamped to total -- as a copy and (4 x 4 -> 2 x 2) through both passes.  3 x 3 = 27 bytes: 5 in -> lead 11, 16 left: no tail; 6 in
# -> lead 10, 17 left: a tail of one.
FLAT_CASES = [((1, 1), (1, 1), (0, 1, 15)), ((2, 2), (2, 2), (0, 1, 15)), ((4, 4), (2, 2), (0, 1, 15)), ((3, 3), (3, 3), (5, 6)),
              ((6, 6), (3, 3), (5, 6))]


@pytest.mark.parametrize("size,ask,leads", FLAT_CASES)
def test_sheets_around_one_piece_at_every_lead(ffr, size, ask, leads):
    img = noise(500 + size[0], *size)
    want, _ = S.host_thumbnail(ffr._host(), img, ask)
    assert want.shape == (ask[1], ask[0], 3)
    try:
        assert np.array_equal(pillow_thumbnail(img, ask), want)
    except ImportError:
        pass
    for lead in leads:
        assert np.array_equal(sheet_at(ffr, [torch.from_numpy(img).cuda()], None, lead, requests=[ask]), want), lead


# pairs two pixels wide: the left run is ONE pixel and the right run is staged behind it.  16 rows of 3 bytes from an address = 13 (mod 16)
# lie at every phase: at 13 the run ends on a 16-byte boundary (head == n), at 14 and 15 n = 3 > head, from 0 to 12 n < head or head == 0.
@pytest.mark.parametrize("phases", [(13, 13), (13, 2), (0, 13)])
def test_pairs_with_a_left_run_of_one_pixel(ffr, phases):
    lib = ffr._host()
    left, right = noise(610, 16, 1), noise(611, 16, 1)
    pair = S.make_pair(left, right)
    on = lambda: ([at_phase(left, phases[0])], [at_phase(right, phases[1])])
    for request in ((2, 16), (1, 8)):                                        # the pair itself (a copy); BICUBIC 2 -> 1 and 16 -> 8
        want, factors = S.host_thumbnail(lib, pair, request)
        assert factors == (1, 1) and want.shape == (request[1], request[0], 3)
        try:
            assert np.array_equal(pillow_thumbnail(pair, request), want)
        except ImportError:
            pass
        assert np.array_equal(sheet_at(ffr, *on(), 0, requests=[request]), want), request
    for fx, fy in ((2, 2), (2, 1), (1, 3)):                                  # cells that straddle the seam; rows folded with the seam whole
        assert np.array_equal(sheet_at(ffr, *on(), 0, factors=(fx, fy)), S.host_reduce(lib, pair, fx, fy)), (fx, fy)
    short = noise(612, 9, 1)                                        # the fixed frame ends at row 9: black below
    assert np.array_equal(sheet_at(ffr, [at_phase(left, phases[0])], [at_phase(short, phases[1])], 0, factors=(1, 1)), S.make_pair(left, short))

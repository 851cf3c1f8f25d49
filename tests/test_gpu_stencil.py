"""The stand-alone 3x3 stencil on the GPU (`vrg_stencil3x3_f32`, csrc/vrg_stencil.hip, through ops.stencil3x3) at every seam of its
three routes -- the float4 flat march in both forms for C = 3 and 4 (strip seams, the overlapped last strip and segment, ragged strips
and segments, workgroups that straddle two frames), the LDS tile kernel and the one-thread-per-element kernel (C = 1, 2, 5, 6, and
views off the 16-byte grid) -- over stencil_support.SWEEP, which tests/test_stencil_host.py shows to reach every such class.  Every
comparison is bit for bit against the oracle (oracle/restated.py), which the same host file holds to the float64 operators."""
import numpy as np
import pytest
import torch

from oracle import restated as R
import stencil_support as S

pytestmark = pytest.mark.gpu

SENTINEL = -7.0                           # no stencil result: those are in [0, 1] or NaN
IDS = [S.case_id(c) for c in S.SWEEP]


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops as _ops
    return _ops


def view_one_float_in(shape, fill=None):
    """-> (buffer, a contiguous view of `shape` that starts one float into it): the view's base is 4 bytes past a 16-byte boundary.  The
    buffer holds SENTINEL around (and, without `fill`, under) the view."""
    n = int(np.prod(shape))
    buf = torch.full((n + 9,), SENTINEL, device="cuda")
    view = buf[1:1 + n].view(shape)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guards_intact(buf, n):
    return bool((buf[:1] == SENTINEL).all()) and bool((buf[1 + n:] == SENTINEL).all())


def arrange(case, x_cpu):
    """The device operands of a sweep case: (input, out= or None, [(buffer, elements)] whose guard floats must survive)."""
    n = x_cpu.numel()
    guarded = []
    if case.arrangement in ("in", "both"):
        buf, x = view_one_float_in(case.shape, x_cpu.cuda())
        guarded.append((buf, n))
    else:
        x = x_cpu.cuda()
        assert x.data_ptr() % 16 == 0
    out = None
    if case.arrangement in ("out", "both"):
        buf, out = view_one_float_in(case.shape)
        guarded.append((buf, n))
    return x, out, guarded


def assert_same(case, got, want, what):
    n, where = S.first_difference(got.cpu().numpy(), want.numpy())
    if n:
        f, y, x, c = where
        pytest.fail(f"{what} on {S.case_id(case)}: {n}/{want.numel()} elements differ, the first at (frame, y, x, c) = {where}: got "
                    f"{float(got[f, y, x, c])!r} want {float(want[f, y, x, c])!r}; {S.describe(case, where)}")


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------
# the sweep
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.SWEEP, ids=IDS)
def test_stencil_over_the_sweep(ops, case):
    """Bit-equal to the oracle for every op, strength and border; the input, and the floats around views off the 16-byte grid, untouched."""
    x_cpu = S.frames(case.shape)
    x, out, guarded = arrange(case, x_cpu)
    for op, strength, zero in S.RUNS:
        got = ops.stencil3x3(x, op, strength, zero, out=out)
        assert got.shape == x.shape and got.data_ptr() != x.data_ptr() and (out is None or got.data_ptr() == out.data_ptr())
        assert_same(case, got, S.expected_of(case.shape, op, strength, zero), f"{op} {strength} {'zero' if zero else 'replicate'}")
        assert same_bits(x.cpu(), x_cpu), "the input changed"
        assert all(guards_intact(buf, n) for buf, n in guarded), "a float outside the view was written"


@pytest.mark.parametrize("op,strength,zero", [("unsharp", 0.5, False), ("sobel", 0.8, True)])
@pytest.mark.parametrize("case", S.SWEEP, ids=IDS)
def test_out_is_overwritten_everywhere_and_nowhere_else(ops, case, op, strength, zero):
    """out= prefilled with a sentinel: every element is stored (the overlapped and ragged strips / segments leave no hole), and for views
    off the 16-byte grid the floats just before and after the view keep the sentinel."""
    x, out, guarded = arrange(case, S.frames(case.shape))
    if out is None:
        out = torch.full(case.shape, SENTINEL, device="cuda")
    else:
        assert bool((out == SENTINEL).all())
    got = ops.stencil3x3(x, op, strength, zero, out=out)
    assert got.data_ptr() == out.data_ptr()
    left = int((out == SENTINEL).sum())
    assert left == 0, f"{left} elements of out= were not written; the first: {S.describe(case, tuple(int(v) for v in torch.nonzero(out == SENTINEL)[0]))}"
    assert_same(case, out, S.expected_of(case.shape, op, strength, zero), f"out= {op}")
    assert all(guards_intact(buf, n) for buf, n in guarded), "a float outside the view was written"


# ------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 37, 132, 3), (2, 73, 129, 4)], ids=lambda s: "x".join(map(str, s)))
def test_frames_are_independent(ops, shape):
    """Every frame with a constant offset of its own: the batch equals its frames run one at a time (a wave decoded to the wrong frame,
    or a workgroup that straddles two frames and reads one of them for both, moves whole vectors between frames)."""
    assert S.route(*shape).route == "flat" and shape[0] > 1          # four waves a frame, and nine (workgroups straddle the frames)
    x = (S.frames(shape) * 0.5 + torch.arange(shape[0], dtype=torch.float32).view(-1, 1, 1, 1) * 0.11).cuda()
    case = S.Case(shape, "aligned")
    for op, strength, zero in S.RUNS:
        batch = ops.stencil3x3(x, op, strength, zero)
        single = torch.cat([ops.stencil3x3(x[f:f + 1].clone(), op, strength, zero) for f in range(shape[0])])
        assert_same(case, batch, single.cpu(), f"batch vs single frames, {op} {strength} {zero}")
        assert_same(case, batch, S.expected(x.cpu(), op, strength, zero), f"batch vs oracle, {op} {strength} {zero}")


# ------------------------------------------------------------------------------------------------
# special values at the seams
# ------------------------------------------------------------------------------------------------
SPECIALS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf"), "-0.0": -0.0, "subnormal": 1e-41}


def seam_positions(shape):
    """(y, float index within the row) of the seams of a steady flat launch: the last float of a strip and the first of the next (the
    overlapped last strip's start included), both row ends; the last row of a segment, the first of the next (the overlapped last
    segment's start included), the first and the last row."""
    _, H, W, C = shape
    r = S.route(*shape)
    assert r.route == "flat" and not r.general and r.strip_overlap and r.segment_overlap
    starts = {min(s * S.WAVE, r.n4 - S.WAVE) for s in range(1, r.strips)} | {s * S.WAVE for s in range(1, r.strips)}       # where a strip begins, where one ends
    cols = sorted({0, W * C - 1} | {4 * v - 1 for v in starts} | {4 * v for v in starts})
    rows = sorted({0, S.FLAT_ROWS - 1, S.FLAT_ROWS, H - S.FLAT_ROWS - 1, H - S.FLAT_ROWS, H - 1})
    return [(y, e) for y in rows for e in cols]


@pytest.mark.parametrize("kind", list(SPECIALS) + ["mixed"])
@pytest.mark.parametrize("shape", [(2, 73, 172, 3), (2, 73, 129, 4)], ids=lambda s: "x".join(map(str, s)))
def test_special_values_at_the_seams(ops, shape, kind):
    """NaN, +Inf, -Inf, -0.0 and a subnormal on both sides of every strip and segment seam and at both row ends, one kind at a time
    and all five in turn: as the oracle (the reference's behaviour) has it -- the same NaN mask and the same values elsewhere."""
    F, H, W, C = shape
    x = S.frames(shape).clone()
    flat = x.view(F, H, W * C)
    values = list(SPECIALS.values())
    for f in range(F):
        for i, (y, e) in enumerate(seam_positions(shape)):
            if kind == "mixed" or (i + f) % 2 == 0:         # one kind alone: every other position, the other ones in the next frame
                flat[f, y, e] = values[(i + f) % 5] if kind == "mixed" else SPECIALS[kind]
    xd = x.cuda()
    case = S.Case(shape, "aligned")
    for op, strength, zero in S.RUNS:
        got = ops.stencil3x3(xd, op, strength, zero).cpu()
        want = S.expected(x, op, strength, zero)
        assert torch.equal(torch.isnan(got), torch.isnan(want)), \
            f"{kind} {op} {strength} {zero}: NaN masks differ, first at {tuple(int(v) for v in torch.nonzero(torch.isnan(got) != torch.isnan(want))[0])}"
        assert_same(case, torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0), f"{kind} {op} {strength} {zero}")
    assert same_bits(xd.cpu(), x)


# ------------------------------------------------------------------------------------------------
# the node
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,use_gpu", [((2, 37, 65, 4), False), ((2, 37, 65, 4), True), ((2, 37, 65, 1), False)])
def test_unsharp_node_on_other_channel_counts(pkg, shape, use_gpu):
    """FastUnsharpSharpen with CPU tensors in and out on RGBA (the flat march, C = 4) and single-channel frames (k_stencil3x3)."""
    from comfyui_vrgamedevgirl_amd import nodes
    x, keep = S.frames(shape).clone(), S.frames(shape)
    (got,) = nodes.FastUnsharpSharpen().apply_unsharp(x, 0.5, use_gpu)
    assert not got.is_cuda and got.shape == x.shape
    want = R.unsharp(x, 0.5, use_gpu).contiguous()
    assert torch.equal(want, S.expected_of(shape, "unsharp", 0.5, use_gpu))
    n, where = S.first_difference(got.numpy(), want.numpy())
    assert n == 0, f"{n} elements differ, the first at (frame, y, x, c) = {where}"
    assert same_bits(x, keep)

"""The resize kernels on the MI355X against torch ITSELF, run live: ops.resize_frames / resize_geometry_frames, ops.restore_frames
(csrc/vrg_resize.hip) and ops.prepare_frames (csrc/vrg_prepare.hip) against F.interpolate evaluated by one child process with torch's
plain CPU kernels (resize_support.torch_results).  The expected value does not come from csrc/vrg_resize_math.hpp: if a case fails here
while tests/test_resize_torch_host.py passes on the same geometry, the arithmetic is right and a kernel is wrong.

The rule is no differing element (resize_support.mismatches == 0), and for Prepare's bytes equality with prepare_support.quantise of
torch's fp32 frames.  The one exclusion is area with a resampled rectangle of exactly 1 x 1 (torch's mean(), documented in the header as
not restated); no case below has that form, which is asserted.

Shapes are the smallest that cross a seam of the kernels.

csrc/vrg_resize.hip
  * the column march (k_resize_bicubic): a thread walks down one output column of a strip of RS_ROWS = 32 output rows and keeps the four
    horizontally resampled source rows from one output row to the next -- the window is the SAME (enlargement), SHIFTED by one source row
    (enlargement, 1:1), or gathered afresh (every shrink past 2x, and the first row of every strip).  Cases: 7x and 3.6x up, 1:1, 1.25x,
    1.5x and 4x down; output heights 31, 32, 33 and 65, so a strip ends one row early, exactly, one row late, and a third strip starts.
  * the workgroup's tile (both kernels): 256 output columns x 32 output rows, `ox >= out_w` lanes leave.  Output widths 255, 256, 257 and
    513 with heights on both sides of 32; a letterbox whose bars and a crop whose overhang cross the tile boundary, a crop that hangs over
    the frame on BOTH axes (a geometry resize_geometry never hands out), a source rectangle off the origin.
  * the 1:1 copy route (k_clamp_copy): the unmatched tail frames of a restore are a clamped copy in a grid-stride loop of at most
    65,536 workgroups x 256 threads = 16,777,216 elements per sweep.  A tail of 2 small frames, and one of 10 frames of 750 x 750 x 3 =
    16,875,000 elements, where the loop goes round a second time.
  * torch's two bilinear forms: resampled height + width 128 and 129, and a letterbox whose frame is past 128 while its rectangle is not.

csrc/vrg_prepare.hip: stated next to the cases (PREPARE)."""
import numpy as np
import pytest
import torch

import prepare_support as PS
import resize_support as RS
from resize_support import AREA, BICUBIC, BILINEAR, CROP, LETTERBOX, METHODS, STRETCH

pytestmark = pytest.mark.gpu

CASES = []          # every case of this file, in the order the child gets them
GROUPS = {}         # group -> [(label, position in CASES, extra)]


def add(group, label, case, **extra):
    CASES.append(case)
    GROUPS.setdefault(group, []).append((label, len(CASES) - 1, extra))


def add_methods(group, label, make, methods=METHODS, **extra):
    for m in methods:
        add(group, f"{label} {m}", make(m), **extra)


# ------------------------------------------------------------------------------------------------ resize (csrc/vrg_resize.hip)
_seed = iter(range(7000, 9000))
for tw in (255, 256, 257, 513):        # the tile in x: the last lane of a workgroup, the first of the next, a third workgroup; 3.6x up in y
    add_methods("resize", f"tile width {tw}", lambda m, tw=tw: RS.fit_case(next(_seed), (2, 9, 11, 4), (tw, 33), STRETCH, m))
for th in (31, 32, 33, 65):            # the strip in y: 40 rows to 31, 32, 33 (1.25x down: shifted and gathered afresh) and up to 65
    add_methods("resize", f"strip height {th}", lambda m, th=th: RS.fit_case(next(_seed), (1, 40, 13, 3), (17, th), STRETCH, m))
add_methods("resize", "march 7x up", lambda m: RS.fit_case(next(_seed), (1, 5, 6, 3), (42, 35), STRETCH, m))          # same window for rows on end
add_methods("resize", "march 1:1", lambda m: RS.fit_case(next(_seed), (1, 35, 37, 4), (37, 35), STRETCH, m))          # shifted by one every row
add_methods("resize", "march 1.5x down", lambda m: RS.fit_case(next(_seed), (1, 51, 45, 3), (30, 34), STRETCH, m))    # shifted by one or two
add_methods("resize", "march 4x down", lambda m: RS.fit_case(next(_seed), (1, 132, 64, 3), (16, 33), STRETCH, m))     # gathered afresh every row
add_methods("resize", "crop over the tile", lambda m: RS.fit_case(next(_seed), (2, 30, 50, 3), (257, 33), CROP, m))   # 257 x 154 resampled, top 60
add_methods("resize", "crop RGBA", lambda m: RS.fit_case(next(_seed), (1, 50, 30, 4), (40, 33), CROP, m))
add_methods("resize", "letterbox bars left and right", lambda m: RS.fit_case(next(_seed), (1, 30, 50, 4), (300, 70), LETTERBOX, m))   # 117 x 70 at x 91
add_methods("resize", "letterbox bars above and below", lambda m: RS.fit_case(next(_seed), (1, 50, 30, 3), (40, 100), LETTERBOX, m))  # 40 x 67 at y 16
add_methods("resize", "crop hanging over on both axes",
            lambda m: RS.rect_case(next(_seed), (1, 21, 23, 3), (0, 0, 23, 21), (300, 90), m, window=(19, 27, 257, 34)))
add_methods("resize", "source rectangle off the origin on both axes",
            lambda m: RS.rect_case(next(_seed), (2, 40, 57, 4), (5, 7, 31, 22), (257, 33), m))
add_methods("resize", "letterbox undone", lambda m: RS.undo_case(next(_seed), (1, 40, 57, 3), (300, 33), LETTERBOX, m))              # src (0, 17, 57, 6)
add_methods("resize", "bilinear sum 128", lambda m: RS.fit_case(next(_seed), (1, 34, 36, 3), (64, 64), STRETCH, m))
add_methods("resize", "bilinear sum 129", lambda m: RS.fit_case(next(_seed), (1, 34, 36, 4), (65, 64), STRETCH, m))
add_methods("resize", "frame past 128, rectangle 120", lambda m: RS.fit_case(next(_seed), (1, 20, 60, 3), (90, 90), LETTERBOX, m))
add_methods("resize", "frame 100, rectangle 200", lambda m: RS.fit_case(next(_seed), (1, 20, 60, 3), (50, 50), CROP, m))

# ------------------------------------------------------------------------------------------------ restore
for strength in (0.0, 0.35, 1.0):
    # content rectangle (0, 8, 31, 4) of the working frames to 257 x 33 RGBA originals; 5 originals for 3 working frames: a tail of 2
    add_methods("restore", f"letterbox undone, tail of 2, strength {strength}", lambda m, s=strength: RS.restore_case(
        next(_seed), (3, 20, 31, 3), next(_seed), (5, 33, 257, 4), LETTERBOX, m, s, 5))
    # content rectangle (5, 0, 9, 31); fewer originals than working frames, RGBA working frames, RGB originals of more than two strips
    add_methods("restore", f"letterbox undone, fewer originals, strength {strength}", lambda m, s=strength: RS.restore_case(
        next(_seed), (4, 31, 20, 4), next(_seed), (2, 65, 19, 3), LETTERBOX, m, s, 2))
add_methods("restore", "stretch back", lambda m: RS.restore_case(next(_seed), (2, 13, 17, 3), next(_seed), (2, 40, 300, 3), STRETCH, m, 0.35, 2))
add_methods("restore", "crop to fill back", lambda m: RS.restore_case(next(_seed), (2, 13, 17, 4), next(_seed), (3, 33, 40, 4), CROP, m, 0.35, 3))
# the copy route past one sweep of its grid: 10 tail frames of 750 x 750 x 3 = 16,875,000 elements against 16,777,216
add("restore", "tail past one sweep of the copy grid", RS.restore_case(next(_seed), (1, 8, 8, 3), next(_seed), (11, 750, 750, 3), STRETCH, BICUBIC, 0.35, 11))

# ------------------------------------------------------------------------------------------------ Prepare (csrc/vrg_prepare.hip)
# Read from k_prepare_bicubic and vrg_prepare_math.hpp; every case runs the four methods (the direct kernel shares bands, segments, the
# frame pick and the byte rows), the seams of the staged ring are the bicubic kernel's.
FRAMES = 5
PICKS = (None, [FRAMES - 1, 0, 0, 3], [2])                               # frame pick: every frame, a list with a repeat out of order, one frame
for th in (1, 7, 8, 9, 17):            # band of PREP_BAND = 8 output rows: less than one, one short of one, one, one more, a third band
    add_methods("prepare", f"band height {th}", lambda m, th=th: RS.fit_case(next(_seed), (FRAMES, 11, 13, 3), (10, th), STRETCH, m), picks=PICKS)
for tw in (255, 256, 257, 513):        # segment of PREP_THREADS = 256 columns per workgroup, sources 3 rows tall
    add_methods("prepare", f"segment width {tw}", lambda m, tw=tw: RS.fit_case(next(_seed), (2, 3, 100, 3), (tw, 4), STRETCH, m))
# ring shift (prep_ring_shift): 0 for rows on end at 7x up, 1 at 1:1, 1 and 2 at 1.5x, 2 and 3 at 2.7x, 4 at 4x, and at 5.3x source rows
# are skipped between the windows of two output rows; 4 as well on the first row of every band
RING = {"7x up": ((5, 6, 3), (42, 35)), "1.5x up": ((12, 14, 4), (21, 18)), "1:1": ((19, 23, 4), (23, 19)), "1.5x down": ((30, 45, 3), (30, 20)),
        "2.7x down": ((54, 81, 3), (30, 20)), "4x down": ((80, 120, 3), (30, 20)), "5.3x down": ((106, 159, 4), (30, 20))}
for name, (src, target) in RING.items():
    add_methods("prepare", f"ring {name}", lambda m, src=src, target=target: RS.fit_case(next(_seed), (1, *src), target, STRETCH, m), ring=True)
for h in (1, 2, 3):                    # taps clamped onto their neighbour at both edges: every tap of a 1-wide source is the same pixel
    for w in (1, 2, 3):
        add_methods("prepare", f"clamped taps {h} x {w}", lambda m, h=h, w=w: RS.fit_case(next(_seed), (2, h, w, 3 + (h + w) % 2), (7, 9), STRETCH, m))
# alignment phase of the staged row (prep_stage): in_c = 3 and widths 53, 54, 55, 57 give row strides of 159, 162, 165 and 171 floats
for w in (53, 54, 55, 57):
    add_methods("prepare", f"phase width {w}", lambda m, w=w: RS.fit_case(next(_seed), (2, 9, w, 3), (31, 7), STRETCH, m), phase=True)
# ... and a staged row that does not start at the frame's left edge: a source rectangle with sx0 > 0 and sy0 > 0, as the letterbox undo
# yields on one axis (ops.resize_geometry always gives src == (0, 0, w, h)), up and down
add_methods("prepare", "off-origin source up", lambda m: RS.rect_case(next(_seed), (2, 17, 55, 3), (6, 3, 41, 11), (97, 19), m), phase=True)
add_methods("prepare", "off-origin source down", lambda m: RS.rect_case(next(_seed), (2, 40, 57, 3), (5, 7, 50, 31), (13, 9), m), phase=True)
add_methods("prepare", "off-origin source RGBA", lambda m: RS.rect_case(next(_seed), (1, 17, 55, 4), (7, 2, 40, 12), (33, 10), m))
add_methods("prepare", "letterbox undone", lambda m: RS.undo_case(next(_seed), (2, 40, 57, 3), (300, 33), LETTERBOX, m))
# stage buffer of PREP_STAGE_FLOATS = 4096 floats: a span of 2063 px of RGB = 6189 floats, cut into segments of fewer than 97 / 300 columns
for tw in (97, 300):
    add_methods("prepare", f"stage buffer to {tw}", lambda m, tw=tw: RS.fit_case(next(_seed), (2, 6, 2063, 3), (tw, 3), STRETCH, m), wide=True)
# fit modes with bars and overhang across bands and segments
add_methods("prepare", "letterbox", lambda m: RS.fit_case(next(_seed), (2, 30, 50, 4), (300, 70), LETTERBOX, m))
add_methods("prepare", "crop to fill", lambda m: RS.fit_case(next(_seed), (2, 30, 50, 3), (257, 33), CROP, m))
add_methods("prepare", "crop hanging over on both axes",
            lambda m: RS.rect_case(next(_seed), (1, 21, 23, 3), (0, 0, 23, 21), (300, 90), m, window=(19, 27, 257, 34)))


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def yardstick(tmp_path_factory):
    """the one child of this file; it never opens the GPU"""
    got = RS.torch_results(CASES, tmp_path_factory.mktemp("torch_yardstick"))
    print(f"\nyardstick: {got.describe()}")
    return got


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def host(t):
    return t.detach().cpu().contiguous().numpy()


def f32(v):
    return np.float32(v)


def bicubic_rows(d, n_in, n_out):
    """rs_taps' four source indices of destination index d, in fp32 as csrc/vrg_resize_math.hpp forms them"""
    real = (f32(n_in) / f32(n_out)) * (f32(d) + f32(0.5)) - f32(0.5)
    i = min(int(np.floor(real)), n_in - 1)
    return [min(max(i - 1 + j, 0), n_in - 1) for j in range(4)]


def test_no_case_has_the_excluded_form(ops):
    for c in CASES:
        g = RS.geometry_of(ops, c)
        assert not (c["method"] == AREA and g.dst[2:] == (1, 1)), c
    both = [RS.geometry_of(ops, c) for c in CASES if c["kind"] == "rect" and c["window"]]
    assert both and all(g.dst[0] < 0 and g.dst[1] < 0 and g.dst[0] + g.dst[2] > g.out_w and g.dst[1] + g.dst[3] > g.out_h for g in both)
    sums = {RS.geometry_of(ops, c).dst[2] + RS.geometry_of(ops, c).dst[3] for c in CASES if c["method"] == BILINEAR}
    assert {128, 129} <= sums


def test_resize_equals_live_torch(ops, yardstick):
    for label, i, _ in GROUPS["resize"]:
        c = yardstick.cases[i]
        x = yardstick.inputs(i)[0].to(dev())
        got = ops.resize_geometry_frames(x, RS.geometry_of(ops, c), c["method"])
        assert RS.mismatches(host(got), yardstick[i]) == 0, label
        if c["kind"] == "fit":                                            # the entry point that works the geometry out itself
            got = ops.resize_frames(x, c["target"][0], c["target"][1], c["fit"], c["method"])
            assert RS.mismatches(host(got), yardstick[i]) == 0, label


def test_restore_equals_live_torch(ops, yardstick):
    for label, i, _ in GROUPS["restore"]:
        c = yardstick.cases[i]
        work, originals = (t.to(dev()) for t in yardstick.inputs(i))
        got = ops.restore_frames(work, originals, c["originals_shape"][2], c["originals_shape"][1], c["fit"], c["method"], c["strength"],
                                 c["frame_count"])
        assert RS.mismatches(host(got), yardstick[i]) == 0, label
        del work, originals, got


def test_the_restore_cases_cross_their_seams(ops):
    tails = []
    for label, i, _ in GROUPS["restore"]:
        c = CASES[i]
        usable = min(c["frame_count"], c["shape"][0])
        tails.append((c["originals_shape"][0] - usable) * int(np.prod(c["originals_shape"][1:])))
    sweep = 65536 * 256
    assert 0 in tails and any(0 < t < sweep for t in tails) and any(t > sweep for t in tails)
    off = {RS.geometry_of(ops, CASES[i]).src[:2] for _, i, _ in GROUPS["restore"] if CASES[i]["fit"] == LETTERBOX}
    assert off == {(0, 8), (5, 0)}


def test_prepare_equals_live_torch(ops, yardstick):
    for label, i, extra in GROUPS["prepare"]:
        c = yardstick.cases[i]
        x = yardstick.inputs(i)[0].to(dev())
        assert x.data_ptr() % 16 == 0                                     # the phases below are counted from an aligned batch
        g = RS.geometry_of(ops, c)
        for pick in extra.get("picks", (None,)):
            want = yardstick[i] if pick is None else yardstick[i][pick]
            got_f32, got_u8 = ops.prepare_frames(x, g, c["method"], pick)
            assert got_f32.dtype == torch.float32 and got_u8.dtype == torch.uint8
            assert RS.mismatches(host(got_f32), want) == 0, (label, pick)
            assert np.array_equal(host(got_u8), PS.quantise(want)), (label, pick)


def test_the_prepare_cases_cross_their_seams(ops):
    """the staged kernel's seams, worked out from the geometry as k_prepare_bicubic walks it: every ring shift 0 ... 4, source rows skipped
    between two windows, every alignment phase of a staged row (the float index of the row's first staged value mod 4), rows that do not
    start at the frame's left edge, more than one segment where the span passes the stage buffer"""
    shifts, phases, skipped, inner_starts = set(), set(), False, 0
    for label, i, extra in GROUPS["prepare"]:
        c = CASES[i]
        if c["method"] != BICUBIC:
            continue
        g = RS.geometry_of(ops, c)
        frames, in_h, in_w, in_c = c["shape"]
        (sx0, sy0, sw, sh), (dx0, dy0, dw, dh) = g.src, g.dst
        if extra.get("ring"):
            for r0 in range(0, g.out_h, 8):
                have = [-1] * 4
                for oy in range(r0, min(r0 + 8, g.out_h)):
                    want = bicubic_rows(oy - dy0, sh, dh)
                    s = next(s for s in range(5) if all(have[j + s] == want[j] for j in range(4 - s)))
                    shifts.add(s)
                    skipped = skipped or (have[3] >= 0 and want[0] > have[3] + 1)
                    have = want
        if extra.get("phase"):
            assert g.out_w <= 256 and dx0 >= 0                            # one segment: the staged span starts at the first column's first tap
            lo = sx0 + bicubic_rows(0, sw, dw)[0]
            assert (sx0 + bicubic_rows(dw - 1, sw, dw)[3] + 1 - lo) * in_c <= 4096
            rows = {sy0 + y for dy in range(dh) for y in bicubic_rows(dy, sh, dh)}
            mine = {(f * in_h * in_w * in_c + (y * in_w + lo) * in_c) % 4 for f in range(frames) for y in rows}
            print(f"{label}: staged rows start at column {lo}, phases {sorted(mine)}")
            phases |= mine
            inner_starts += lo > 0
        if extra.get("wide"):
            assert in_w * in_c > 4096 and sw == in_w
    assert shifts == {0, 1, 2, 3, 4} and skipped
    assert phases == {0, 1, 2, 3} and inner_starts >= 2

"""csrc/vrg_resize_math.hpp compiled for the host against torch ITSELF, run live: one child process evaluates every case of this file with
torch's plain CPU kernels (resize_support.torch_results: ATEN_CPU_CAPABILITY=default, at least two threads), and the host build of the
header (tests/host_math/resize_check.cpp, the arithmetic the kernels call) must equal it in every element.  No GPU, no fixture: the
expected values come from the torch that is installed where the test runs.

The rule is resize_support.mismatches == 0.  The one exclusion is the form the header documents as not restated: area with a resampled
rectangle of exactly 1 x 1, where torch takes its mean() reduction.  Such cases are excluded BY THEIR FORM, before anything is compared,
counted, and may be at most 2 in 1,000 of the sweep; every other case is compared.

The sweep (seeded): 312 geometries x 4 methods with sides 1 ... 140, RGB and RGBA, the three fit modes in turn; every third triple of
them is aimed at a resampled height + width of 126 ... 130, where torch changes its bilinear kernel (at most 128: channels-last
kernel, above: the generic separable one).  By hand: letterboxes whose frame is past 128 while the resampled rectangle is not, crops
the other way round (the choice follows the RESAMPLED size), a dozen larger cases with sides up to 700, and the restore direction.
Geometries whose resampled frame would pass 80,000 pixels are redrawn: torch resamples the whole frame before a crop cuts it, and the
file has to stay quick."""
import random
import shutil

import pytest

import resize_support as RS
from resize_support import AREA, BICUBIC, BILINEAR, CROP, FITS, LETTERBOX, METHODS, NEAREST, STRETCH

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

SWEEP_GEOMETRIES = 312
MAX_RESAMPLED_PIXELS = 80000


def _resampled(ops, h, w, tw, th, fit):
    g = ops.resize_geometry(h, w, tw, th, fit)
    return g.dst[2], g.dst[3]


def _draw(rng, ops, fit, aimed):
    """(h, w, tw, th) with every side in 1 ... 140; aimed: the resampled width + height lands in 126 ... 130"""
    while True:
        h, w = rng.randint(1, 140), rng.randint(1, 140)
        if not aimed:
            tw, th = rng.randint(1, 140), rng.randint(1, 140)
        elif fit == STRETCH:
            total = rng.randint(126, 130)
            tw = rng.randint(1, total - 1)
            th = total - tw
        else:
            # the resampled rectangle keeps the aspect of the source: scale it to the sum, then give the target another aspect so that
            # the letterbox gets bars and the crop cuts something off
            scale = rng.randint(126, 130) / (h + w)
            tw, th = max(1, round(w * scale)), max(1, round(h * scale))
            extra = rng.randint(1, 12)
            if rng.random() < 0.5:
                th = th + extra if fit == LETTERBOX else th - extra
            else:
                tw = tw + extra if fit == LETTERBOX else tw - extra
        if not (1 <= tw <= 140 and 1 <= th <= 140):
            continue
        rw, rh = _resampled(ops, h, w, tw, th, fit)
        if rw * rh > MAX_RESAMPLED_PIXELS or (aimed and not 126 <= rw + rh <= 130):
            continue
        return h, w, tw, th


def sweep_cases(ops):
    rng = random.Random(20261020)
    cases, aimed_count = [], 0
    for i in range(SWEEP_GEOMETRIES):
        fit, aimed = FITS[i % 3], i % 9 < 3
        h, w, tw, th = _draw(rng, ops, fit, aimed)
        aimed_count += aimed
        shape = (2 if i % 7 == 0 else 1, h, w, 3 + (i // 3) % 2)
        cases += [RS.fit_case(1000 + i, shape, (tw, th), fit, m) for m in METHODS]
    assert 3 * aimed_count >= SWEEP_GEOMETRIES
    return cases


# letterbox: the frame's height + width is past 128, the resampled rectangle's is not -- (source h, w), (target w, h), resampled (w, h)
LETTERBOX_SMALL_INSIDE_LARGE = (((20, 60), (90, 90), (90, 30)), ((60, 20), (100, 96), (32, 96)), ((33, 31), (140, 64), (60, 64)),
                                ((16, 48), (96, 100), (96, 32)), ((10, 30), (96, 140), (96, 32)))
# crop to fill: the frame's height + width is at most 128, the resampled rectangle's is past it
CROP_LARGE_AROUND_SMALL = (((20, 60), (50, 50), (150, 50)), ((60, 20), (40, 60), (40, 120)), ((33, 31), (64, 64), (64, 68)),
                           ((16, 48), (32, 33), (99, 33)), ((30, 10), (43, 85), (43, 129)))
LARGE = ((431, 700, 233, 129, STRETCH), (700, 433, 301, 700, STRETCH), (257, 311, 700, 513, STRETCH), (150, 699, 141, 143, STRETCH),
         (523, 301, 640, 360, CROP), (181, 641, 257, 700, CROP), (602, 397, 199, 211, CROP), (145, 149, 700, 651, CROP),
         (431, 700, 233, 229, LETTERBOX), (160, 283, 700, 417, LETTERBOX), (700, 700, 255, 513, LETTERBOX), (299, 167, 512, 700, LETTERBOX))


def hand_cases():
    cases = []
    for k, ((h, w), target, _) in enumerate(LETTERBOX_SMALL_INSIDE_LARGE):
        cases += [RS.fit_case(3000 + k, (1, h, w, 3 + k % 2), target, LETTERBOX, m) for m in METHODS]
    for k, ((h, w), target, _) in enumerate(CROP_LARGE_AROUND_SMALL):
        cases += [RS.fit_case(3100 + k, (1, h, w, 3 + k % 2), target, CROP, m) for m in METHODS]
    for k, (h, w, tw, th, fit) in enumerate(LARGE):                     # a dozen larger cases, the methods in turn
        cases.append(RS.fit_case(3200 + k, (1, h, w, 3 + k % 2), (tw, th), fit, METHODS[k % 4]))
    cases.append(RS.fit_case(3300, (1, 9, 7, 3), (1, 1), STRETCH, AREA))  # the excluded form, so that the exclusion is seen to work
    return cases


def restore_cases():
    """the restore direction.  Working frames 20 x 31 for a 37 x 11 source: the letterbox content is (0, 5, 31, 9), off the origin in y;
    31 x 20 for 11 x 37: (5, 0, 9, 31), off the origin in x.  Strengths 0, 0.35 and 1, RGB and RGBA originals, more and fewer original
    frames than working frames."""
    cases, k = [], 0
    for (wh, ww), (sw, sh) in (((20, 31), (37, 11)), ((31, 20), (11, 37))):
        for m in METHODS:
            for strength in (0.0, 0.35, 1.0):
                work_frames, frame_count = ((3, 5), (4, 2), (2, 2))[k % 3]
                cases.append(RS.restore_case(4000 + 2 * k, (work_frames, wh, ww, 3 + (k // 3) % 2), 4001 + 2 * k, (frame_count, sh, sw, 3 + k % 2),
                                             LETTERBOX, m, strength, frame_count))
                k += 1
            cases.append(RS.undo_case(4500 + k, (1, wh, ww, 4), (sw, sh), LETTERBOX, m))
    for j, (fit, m) in enumerate(((STRETCH, BICUBIC), (CROP, BILINEAR), (STRETCH, AREA), (CROP, NEAREST))):   # no letterbox: the whole frame
        cases.append(RS.restore_case(4800 + 2 * j, (2, 13, 17, 3), 4801 + 2 * j, (3, 29, 23, 4), fit, m, 0.35, 3))
    return cases


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return RS.build_host_lib(tmp_path_factory.mktemp("resize_check"))


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def yardstick(ops, tmp_path_factory):
    """the one child of this file"""
    got = RS.torch_results(sweep_cases(ops) + hand_cases() + restore_cases(), tmp_path_factory.mktemp("torch_yardstick"))
    print(f"\nyardstick: {got.describe()}")
    return got


def excluded_form(ops, case):
    """area with a resampled rectangle of exactly 1 x 1: torch's mean(), which csrc/vrg_resize_math.hpp documents as not restated"""
    g = RS.geometry_of(ops, case)
    return case["method"] == AREA and g.dst[2] == 1 and g.dst[3] == 1


def host_value(hm, ops, yardstick, i):
    c = yardstick.cases[i]
    g = RS.geometry_of(ops, c)
    xs = yardstick.inputs(i)
    if c["kind"] == "restore":
        usable = min(c["frame_count"], c["shape"][0])
        return RS.host_restore(hm, ops, xs[0].numpy(), xs[1].numpy(), g, c["method"], c["strength"], usable)
    return RS.host_resize(hm, ops, xs[0].numpy(), g, c["method"])


def test_the_sweep_is_what_the_docstring_says(ops):
    cases = sweep_cases(ops)
    assert len(cases) == SWEEP_GEOMETRIES * 4 >= 1200
    geoms = [RS.geometry_of(ops, c) for c in cases[::4]]
    near = sum(126 <= g.dst[2] + g.dst[3] <= 130 for g in geoms)
    assert 3 * near >= len(geoms)
    for fit in FITS:                                                      # each fit mode on both sides of the kernel choice
        sums = {g.dst[2] + g.dst[3] for g, c in zip(geoms, cases[::4]) if c["fit"] == fit}
        assert {126, 127, 128, 129, 130} <= sums, (fit, sorted(sums))
    assert {c["shape"][3] for c in cases} == {3, 4} and {c["fit"] for c in cases} == set(FITS)
    sides = [s for c in cases for s in (*c["shape"][1:3], *c["target"])]
    assert min(sides) == 1 and max(sides) == 140
    for (h, w), (tw, th), resampled in LETTERBOX_SMALL_INSIDE_LARGE:
        g = ops.resize_geometry(h, w, tw, th, LETTERBOX)
        assert g.dst[2:] == resampled and g.out_h + g.out_w > 128 >= g.dst[2] + g.dst[3]
    for (h, w), (tw, th), resampled in CROP_LARGE_AROUND_SMALL:
        g = ops.resize_geometry(h, w, tw, th, CROP)
        assert g.dst[2:] == resampled and g.out_h + g.out_w <= 128 < g.dst[2] + g.dst[3]
    assert len(LARGE) == 12 and max(max(c[:4]) for c in LARGE) == 700
    restores = [c for c in restore_cases() if c["kind"] == "restore"]
    assert {c["strength"] for c in restores} == {0.0, 0.35, 1.0} and {c["originals_shape"][3] for c in restores} == {3, 4}
    assert {(c["frame_count"] > c["shape"][0]) - (c["frame_count"] < c["shape"][0]) for c in restores} == {-1, 0, 1}
    off = {RS.geometry_of(ops, c).src[:2] for c in restores if c["fit"] == LETTERBOX}
    assert off == {(0, 5), (5, 0)}


def test_host_arithmetic_equals_live_torch_in_every_element(hm, ops, yardstick):
    excluded, differing = [], []
    for i, c in enumerate(yardstick.cases):
        if excluded_form(ops, c):
            excluded.append(c)
            continue
        bad = RS.mismatches(host_value(hm, ops, yardstick, i), yardstick[i])
        if bad:
            differing.append((bad, c))
    print(f"\nyardstick: {yardstick.describe()}; excluded (area, resampled rectangle 1 x 1): {len(excluded)} of {len(yardstick)}; "
          f"differing: {len(differing)}")
    assert not differing, differing[:8]
    assert all(c["method"] == AREA and RS.geometry_of(ops, c).dst[2:] == (1, 1) for c in excluded)
    assert 1 <= len(excluded) and 1000 * len(excluded) <= 2 * len(yardstick)


"""The stand-alone 3x3 stencil (`vrg_stencil3x3_f32`, csrc/vrg_stencil.hip) at every seam of its three routes: a plain-Python
restatement of the entry point's route decision and of `launch_stencil_flat`'s geometry (`route`), the shapes that reach every class of
that geometry (`SWEEP`; tests/test_stencil_host.py asserts that they do), seeded inputs, the expected values from the oracle
(`expected`: oracle/restated.py, bit-pinned to the reference's own nodes by tests/test_oracle_golden.py) and the same operators in
float64 (`truth64`), against which tests/test_stencil_host.py holds the oracle at these shapes and channel counts."""
import functools
import os
import re
from collections import namedtuple

import numpy as np
import torch

from oracle import restated as R
from conftest import PKG_DIR

SOURCE = os.path.join(PKG_DIR, "csrc", "vrg_stencil.hip")
WAVE = 64                                 # vectors per strip: one per lane of a wave64


def _flat_rows():
    with open(SOURCE, "r", encoding="utf-8") as fh:
        m = re.search(r"^#define\s+VRG_FLAT_ROWS\s+(\d+)", fh.read(), re.M)
    assert m, "VRG_FLAT_ROWS not found in csrc/vrg_stencil.hip"
    return int(m.group(1))


FLAT_ROWS = _flat_rows()                  # rows per strip segment of the flat march

Route = namedtuple("Route", "route general n4 strips segments strip_overlap strip_ragged segment_overlap segment_ragged last_rows "
                            "waves_mod4 groups_mod8 straddles")


def route(frames, H, W, C, aligned=True):
    """What `vrg_stencil3x3_f32` does with `frames` x H x W x C floats whose two base pointers are (`aligned`) or are not both on a
    16-byte boundary.  route: 'flat' (k_stencil_flat), 'tile' (the fused chain's LDS tile kernel, stencil stage only) or 'generic'
    (k_stencil3x3); the other fields describe the flat march's launch and are None elsewhere."""
    row = W * C
    if C in (3, 4) and row % 4 == 0 and row // 4 <= 0x7FFFFFFF // 64 and aligned:
        n4 = row // 4
        strips = (n4 + WAVE - 1) // WAVE
        segments = (H + FLAT_ROWS - 1) // FLAT_ROWS
        general = n4 < WAVE or H < FLAT_ROWS
        waves = strips * segments * frames
        groups = (waves + 3) // 4
        return Route("flat", general, n4, strips, segments,
                     strip_overlap=not general and n4 % WAVE != 0, strip_ragged=general and n4 % WAVE != 0,
                     segment_overlap=not general and H % FLAT_ROWS != 0, segment_ragged=general and H % FLAT_ROWS != 0,
                     last_rows=H - (segments - 1) * FLAT_ROWS if general else FLAT_ROWS,
                     waves_mod4=waves % 4, groups_mod8=groups % 8, straddles=(strips * segments) % 4 != 0 and frames > 1)
    if C == 3 and H * W <= 0x7FFFFFFF // 3:
        return Route("tile", *([None] * 12))
    return Route("generic", *([None] * 12))


Case = namedtuple("Case", "shape arrangement")       # arrangement: 'aligned', or which of input / out= is a view one float into a buffer

_SHAPES = [
    # flat march, C = 3, steady form (GENERAL = false)
    (3, 36, 88, 3),        # n4 = 66: overlapped last strip, exactly one segment, a workgroup straddles two frames
    (3, 37, 88, 3),        # overlapped strip and overlapped segment
    (2, 73, 172, 3),       # n4 = 129: 3 x 3 waves a frame, both overlaps, an interior strip with halo loads on both sides
    (1, 72, 256, 3),       # n4 = 192: no overlap either way
    (5, 37, 132, 3),       # five frames: the wave -> (strip, segment, frame) decode
    # flat march, C = 3, GENERAL: row counts 1, 2, 3, 4, 5, 35 against the three-rows-per-trip loop
    (3, 35, 88, 3), (2, 5, 172, 3),
    (2, 100, 8, 3),        # n4 = 6, segments of 36, 36 and 28 rows
    (3, 1, 4, 3), (1, 2, 256, 3),
    (2, 4, 84, 3),         # n4 = 63
    (1, 3, 88, 3),
    # flat march, C = 4, steady form
    (3, 36, 64, 4),        # n4 = 64: exactly one full strip
    (3, 37, 65, 4),        # overlap of 63 columns and of 35 rows
    (2, 73, 129, 4), (1, 72, 128, 4),
    # flat march, C = 4, GENERAL
    (2, 35, 66, 4), (2, 100, 7, 4), (3, 1, 1, 4), (2, 4, 63, 4),
    (1, 3, 66, 4),         # a last segment of 3 rows: rows % 3 == 0 for C = 4 too (the four above give 2, 1, 1, 1)
    # LDS tile kernel
    (2, 37, 87, 3), (1, 1, 1, 3),
    # k_stencil3x3
    (2, 37, 65, 1), (2, 9, 13, 2), (1, 37, 21, 5), (3, 1, 1, 1), (1, 1, 9, 6),
]
#: contiguous views one float into a larger buffer: C = 4 -> k_stencil3x3, C = 3 -> the tile kernel
MISALIGNED_SHAPES = [(2, 37, 65, 4), (2, 37, 88, 3)]
ARRANGEMENTS = ("in", "out", "both")

SWEEP = [Case(s, "aligned") for s in _SHAPES] + [Case(s, a) for s in MISALIGNED_SHAPES for a in ARRANGEMENTS]
SHAPES = list(dict.fromkeys(c.shape for c in SWEEP))          # every shape once, in sweep order

#: (op, strength, zero_border): the runs of every sweep case
RUNS = [("unsharp", 0.5, False), ("unsharp", 0.5, True), ("unsharp", 3.75, False), ("unsharp", 3.75, True),
        ("laplacian", 0.8, False), ("laplacian", 0.8, True), ("sobel", 0.8, False), ("sobel", 0.8, True)]


def case_id(case):
    return "x".join(str(v) for v in case.shape) + ("" if case.arrangement == "aligned" else f"-misaligned-{case.arrangement}")


def case_route(case):
    return route(*case.shape, aligned=case.arrangement == "aligned")


@functools.lru_cache(maxsize=None)
def frames(shape):
    """The seeded input of a shape: uniform in [-0.1, 1.1), so that both clamps act.  One seed per shape.  Shared: do not write to it."""
    g = torch.Generator().manual_seed(4100 + SHAPES.index(shape))
    return torch.rand(*shape, generator=g) * 1.2 - 0.1


def expected(x, op, strength, zero_border):
    """The oracle's value of ops.stencil3x3(x, op, strength, zero_border): the pairing of
    test_fused_chain_equals_sequential_operators_and_oracle (tests/test_gpu_parity.py)."""
    with np.errstate(invalid="ignore", over="ignore"):
        if op == "unsharp":
            return R.unsharp(x, strength, zero_border).contiguous()
        if zero_border:
            return (R.laplacian_zero_raster if op == "laplacian" else R.sobel_zero_raster)(x, strength)
        return (R.laplacian if op == "laplacian" else R.sobel)(x, strength, False)


@functools.lru_cache(maxsize=None)
def expected_of(shape, op, strength, zero_border):
    """`expected` of the seeded frames of a shape, computed once for all tests of a process."""
    return expected(frames(shape), op, strength, zero_border)


def truth64(x, op, strength, zero_border):
    """The same operators in numpy float64, in no particular order: what the formulas mean.  The constants are the fp32 numbers the
    fp32 operators see (a Python scalar is rounded to fp32 when it meets an fp32 tensor): strength, and the 1e-6 under the zero-border
    sobel's root.  -> float64 array."""
    a = np.asarray(x, dtype=np.float64)
    s = float(np.float32(strength))
    p = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="constant" if zero_border else "edge")
    H, W = a.shape[1], a.shape[2]
    t = lambda dy, dx: p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    if op == "unsharp":
        blur = sum(t(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
        out = a + s * (a - blur)
    elif op == "laplacian":
        lap = t(0, -1) + t(-1, 0) + t(1, 0) + t(0, 1) - 4.0 * a
        out = a + s * (-lap if zero_border else lap)           # the use_gpu path convolves with the negated kernel
    else:
        gx = (t(-1, 1) + 2.0 * t(0, 1) + t(1, 1)) - (t(-1, -1) + 2.0 * t(0, -1) + t(1, -1))
        gy = (t(1, -1) + 2.0 * t(1, 0) + t(1, 1)) - (t(-1, -1) + 2.0 * t(-1, 0) + t(-1, 1))
        out = a + s * np.sqrt(gx * gx + gy * gy + (float(np.float32(1e-6)) if zero_border else 0.0))
    return np.clip(out, 0.0, 1.0)


def ulps(got, want64):
    """largest distance in units of ulp(1.0) = 2^-23"""
    return float(np.abs(np.asarray(got, dtype=np.float64) - want64).max()) * 2.0 ** 23


def first_difference(got, want):
    """-> (number of differing elements, (frame, y, x, c) of the first) of two [F, H, W, C] arrays; NaN equals NaN, -0.0 equals 0.0"""
    got, want = np.asarray(got), np.asarray(want)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    n = int(bad.sum())
    return n, (tuple(int(v) for v in np.argwhere(bad)[0]) if n else None)


def describe(case, where):
    """Names the seam of a differing element: its vector, and the strips / lanes / segments / rows of the waves that store it."""
    r = case_route(case)
    if r.route != "flat":
        return f"route {r.route}"
    f, y, x, c = where
    C, H = case.shape[3], case.shape[1]
    vec = (x * C + c) // 4
    cols = []
    for s in range(r.strips):
        c0 = s * WAVE if r.general else min(s * WAVE, r.n4 - WAVE)
        if c0 <= vec < min(c0 + WAVE, r.n4):
            cols.append(f"strip {s} lane {vec - c0}")
    rows = []
    for g in range(r.segments):
        y0 = g * FLAT_ROWS if r.general else min(g * FLAT_ROWS, H - FLAT_ROWS)
        if y0 <= y < min(y0 + FLAT_ROWS, H):
            rows.append(f"segment {g} row {y - y0}")
    return (f"route flat ({'GENERAL' if r.general else 'steady'}, n4 {r.n4}, {r.strips} strips x {r.segments} segments), vector {vec} float {(x * C + c) % 4}: "
            f"{' and '.join(cols)}; {' and '.join(rows)}")

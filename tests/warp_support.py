"""Shared by tests/test_warp_host.py, tests/test_gpu_landmark.py and tools/make_golden_landmark.py.

``restated``: OpenCV 4.x's uint8 warpAffine(..., INTER_LANCZOS4, BORDER_REFLECT101) restated in numpy from the text of the specification
(the matrix inverted in Python doubles, the 1-D weights with math.sin / math.cos, everything after them in integers; the border by
repeating the reflection until the coordinate is in range) -- written independently of csrc/vrg_warp_math.hpp, which must give the same
bytes on the host (tests/host_math/warp_check.cpp) and on the GPU.
``yardstick64``: the mathematical filter in float64 at the SAME quantised 1/32-pixel coordinates -- weights sinc(x) * sinc(x / 4) over the
same 8 x 8 taps, normalised per axis, the same reflected border, ONE final rounding.  What is left between the two are the 15-bit weights
and their fix-up."""
import ctypes as C
import hashlib
import json
import math
import os
import subprocess

import numpy as np

from lanczos_support import differences, random_frames, smooth_frames  # noqa: F401 -- the frame makers and the level / share count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "comfyui-vrgamedevgirl_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")

U8P = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
F32P = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
I16P = np.ctypeslib.ndpointer(dtype=np.int16, flags="C_CONTIGUOUS")
FLT_EPSILON = float(np.finfo(np.float32).eps)
S45 = 0.70710678118654752440084436210485
CS = ((1.0, 0.0), (-S45, -S45), (0.0, 1.0), (S45, -S45), (-1.0, 0.0), (S45, S45), (0.0, -1.0), (-S45, S45))
SAMPLES = 2048

# The float64 yardstick, measured with the restatement on the CPU over CASES of tests/test_warp_host.py (printed by
# test_float64_yardstick).  Levels: 1 is what 15-bit weights allow -- the 64 rounded weights of a phase are each within half a unit of
# 2^-15 (the one fixed-up entry within a few units), so the integer sum is within 64 * 0.5 * 255 / 32768 = 0.25 level (+ the fix-up's
# few * 255 / 32768 < 0.05) of the float64 sum: the two roundings land at most one level apart.  Measured: 1.
# Share: the worst case measured is 0.744 % of the bytes (50 of 6720: random 40 x 56 frame, rotation 4 degrees, scale 1.03); 1.5 x
# headroom, as the Lanczos yardstick.  Far below the resize's 15 %: a 15-bit weight against an 11-bit one, one rounding against two.
YARDSTICK_MAX_LEVELS = 1                # measured: 1
YARDSTICK_MAX_SHARE = 0.01116           # measured worst: 0.00744; x 1.5


def weights_1d(t):
    """the eight float32 weights of fractional position t (float32)"""
    f32 = np.float32
    t = f32(t)
    if float(t) < FLT_EPSILON:
        return [f32(0)] * 3 + [f32(1)] + [f32(0)] * 4
    y0 = -float(f32(t + f32(3.0))) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    coeffs, total = [], f32(0.0)
    for i in range(8):
        y = -float(f32(f32(t + f32(3.0)) - f32(i))) * math.pi * 0.25
        c = f32((CS[i][0] * s0 + CS[i][1] * c0) / (y * y))
        coeffs.append(c)
        total = f32(total + c)
    inv = f32(f32(1.0) / total)
    return [f32(c * inv) for c in coeffs]


_TABLE = None


def phase_table():
    """[1024, 8, 8] int16: phase = fy * 32 + fx, then tap row, tap column"""
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    f32 = np.float32
    one = [weights_1d(f32(k) * f32(1.0 / 32.0)) for k in range(32)]
    table = np.zeros((1024, 8, 8), dtype=np.int64)
    for fy in range(32):
        for fx in range(32):
            t = table[fy * 32 + fx]
            for k1 in range(8):
                for k2 in range(8):
                    v = f32(f32(one[fy][k1] * one[fx][k2]) * f32(32768.0))
                    t[k1, k2] = min(32767, max(-32768, int(np.rint(v))))
            diff = int(t.sum()) - 32768
            if diff:
                small = large = (4, 4)
                for k1 in (4, 5):
                    for k2 in (4, 5):
                        if t[k1, k2] < t[small]:
                            small = (k1, k2)
                        elif t[k1, k2] > t[large]:
                            large = (k1, k2)
                if diff < 0:
                    t[large] -= diff
                else:
                    t[small] -= diff
    assert table.min() >= -32768 and table.max() <= 32767
    _TABLE = table.astype(np.int16)
    return _TABLE


def inverted(transform):
    """the six Python doubles of the inverted matrix"""
    M = [float(np.float32(v)) for v in np.asarray(transform, dtype=np.float32).reshape(6)]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0], M[1], M[3], M[4] = A11, M[1] * -D, M[3] * -D, A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return M


def _terms(transform, out_w, out_h):
    """(adelta [w], bdelta [w], X0 [h], Y0 [h]) as float64 (exact integers), before any int32 question"""
    M = inverted(transform)
    xs, ys = np.arange(out_w, dtype=np.float64), np.arange(out_h, dtype=np.float64)
    with np.errstate(all="ignore"):
        return (np.rint(M[0] * xs * 1024.0), np.rint(M[3] * xs * 1024.0),
                np.rint((M[1] * ys + M[2]) * 1024.0) + 16.0, np.rint((M[4] * ys + M[5]) * 1024.0) + 16.0)


def refused(transform, out_w, out_h):
    """the specification's refusal, by brute force over every column and row: a non-finite entry, or a scaled term (or the sum of a row
    and a column term) that leaves int32"""
    t = np.asarray(transform, dtype=np.float32)
    if not np.isfinite(t).all():
        return True
    a, b, x0, y0 = _terms(t, out_w, out_h)
    lo, hi = -2.0 ** 31, 2.0 ** 31 - 1
    for col, row in ((a, x0), (b, y0)):
        if not (np.isfinite(col).all() and np.isfinite(row).all()):
            return True
        if col.min() < lo or col.max() > hi or (row - 16).min() < lo or row.max() > hi:
            return True
        s = row[:, None] + col[None, :] if row.size * col.size <= 1 << 22 else np.array([row.min() + col.min(), row.max() + col.max()])
        if s.min() < lo or s.max() > hi:
            return True
    return False


def _fold(p, n):
    """BORDER_REFLECT101 by repetition"""
    p = np.array(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * (n - 1) - p, p))


def positions(transform, out_w, out_h):
    """(sx [h, w], sy, phase x, phase y) int64"""
    a, b, x0, y0 = (v.astype(np.int64) for v in _terms(transform, out_w, out_h))
    X = (x0[:, None] + a[None, :]) >> 5
    Y = (y0[:, None] + b[None, :]) >> 5
    return np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767), X & 31, Y & 31


def restated(image, transform, out_w, out_h):
    """[H, W, 3] uint8, 2 x 3 float32 -> [out_h, out_w, 3] uint8"""
    img = np.ascontiguousarray(image, dtype=np.uint8).astype(np.int64)
    H, W, _ = img.shape
    assert not refused(transform, out_w, out_h)
    sx, sy, fx, fy = positions(transform, out_w, out_h)
    tab = phase_table().astype(np.int64)[fy * 32 + fx]                       # [h, w, 8, 8]
    acc = np.zeros((out_h, out_w, 3), dtype=np.int64)
    xs = [_fold(sx - 3 + k, W) for k in range(8)]
    for k1 in range(8):
        yy = _fold(sy - 3 + k1, H)
        for k2 in range(8):
            acc += img[yy, xs[k2]] * tab[:, :, k1, k2, None]
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def yardstick64(image, transform, out_w, out_h):
    img = np.asarray(image, dtype=np.float64)
    H, W, _ = img.shape
    sx, sy, fx, fy = positions(transform, out_w, out_h)
    offs = np.arange(-3, 5, dtype=np.float64)

    def weights(frac):
        d = frac[..., None].astype(np.float64) / 32.0 - offs
        w = np.sinc(d) * np.sinc(d / 4.0)
        return w / w.sum(axis=-1, keepdims=True)

    wx, wy = weights(fx), weights(fy)
    acc = np.zeros((out_h, out_w, 3))
    xs = [_fold(sx - 3 + k, W) for k in range(8)]
    for k1 in range(8):
        yy = _fold(sy - 3 + k1, H)
        for k2 in range(8):
            acc += img[yy, xs[k2]] * (wy[:, :, k1] * wx[:, :, k2])[..., None]
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def quantise(values):
    """uint8(clip(rint(v * 255), 0, 255)) in float32; NaN gives 0"""
    v = np.asarray(values, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(v * np.float32(255.0)), 0, 255)
    return np.where(np.isnan(r), np.float32(0), r).astype(np.uint8)


def similarity(scale, degrees, tx, ty, centre=(0.0, 0.0)):
    """2 x 3 float32: rotation by `degrees` and `scale` about `centre`, then a shift"""
    c, s = scale * math.cos(math.radians(degrees)), scale * math.sin(math.radians(degrees))
    cx, cy = centre
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty]], dtype=np.float32)


def frames_of(shape_hw, kind, seed):
    make = random_frames if kind == "random" else smooth_frames
    return make((1, shape_hw[0], shape_hw[1], 3), seed)[0]


def build_host_lib(directory):
    out = os.path.join(str(directory), "libwarp_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "warp_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_warp_desc_bytes.argtypes, lib.hm_warp_desc_bytes.restype = [], C.c_int64
    lib.hm_warp_phase_table.argtypes, lib.hm_warp_phase_table.restype = [I16P], None
    lib.hm_warp_record.argtypes = [F32P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p]
    lib.hm_warp_record.restype = C.c_int
    lib.hm_warp_affine.argtypes = [U8P, U8P, F32P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.hm_warp_affine.restype = C.c_int
    lib.hm_warp_quantise.argtypes, lib.hm_warp_quantise.restype = [F32P, U8P, C.c_int64], None
    return lib


def host_warp(lib, image, transform, out_w, out_h):
    x = np.ascontiguousarray(image, dtype=np.uint8)
    out = np.zeros((int(out_h), int(out_w), 3), dtype=np.uint8)
    ok = lib.hm_warp_affine(x, out, np.ascontiguousarray(transform, dtype=np.float32).reshape(6), x.shape[0], x.shape[1], int(out_h), int(out_w))
    return out if ok else None


# ------------------------------------------------------------------------------------------------ the recorded reference (landmark.*)
def meta():
    with open(os.path.join(GOLDEN, "landmark.json")) as fh:
        return json.load(fh)


def arrays():
    return np.load(os.path.join(GOLDEN, "landmark.npz"))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def sample_positions(numel, seed):
    return np.random.Generator(np.random.PCG64(int(seed) + 1)).integers(0, int(numel), SAMPLES)


def case_inputs(case):
    """(originals, work) float32 of a fixture case, generated as the tool generated them: originals dyadic in [-0.1, 1.1], work frames
    uniform in [-0.1, 1.1)"""
    rng = np.random.Generator(np.random.PCG64(int(case["seed"])))
    originals = (rng.integers(-102, 1127, size=tuple(case["originals_shape"])).astype(np.float32) / np.float32(1024.0))
    work = rng.random(tuple(case["work_shape"]), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    return np.ascontiguousarray(originals), np.ascontiguousarray(work)


def case_entries(case):
    return [dict(e, box=tuple(e["box"]) if e.get("box") is not None else None) for e in case["entries"]]


class ScriptedEstimator:
    """The estimator seam fed from a case's script: call k returns script[k] (a 2 x 3 list or None) and records what it was given."""

    def __init__(self, script):
        self.script, self.calls, self.seen = list(script), 0, []

    def __call__(self, source_u8, generated_u8):
        item = self.script[self.calls]
        self.calls += 1
        self.seen.append((np.array(source_u8, copy=True), np.array(generated_u8, copy=True)))
        return None if item is None else np.array(item, dtype=np.float64)


def cv2_fixture_path():
    return os.path.join(GOLDEN, "warp_lanczos4_cv2.npz")

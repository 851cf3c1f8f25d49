"""Shared by tests/test_detect_host.py, tests/test_gpu_detect.py and tools/make_golden_detect.py.

``quantise_bgr`` / ``warp_linear`` / ``resize_linear`` / ``blob``: the detector's input restated in numpy from the text of the specification
(OpenCV 4.x's classic fixed-point paths: warpAffine INTER_LINEAR BORDER_REPLICATE on bytes, resize INTER_LINEAR on bytes, blobFromImage) --
written independently of csrc/vrg_detect_math.hpp, which must give the same values on the host (tests/host_math/detect_check.cpp) and on the
GPU.  The warp and the resize are two separate whole-image functions and the blob is their composition: the rotated frame EXISTS here,
while the header and the kernels never form it.
``warp_yardstick64`` / ``resize_yardstick64``: float64 bilinear filters at the same coordinates.
``CASES``: the geometries of the issue."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from conftest import GOLDEN, PKG_DIR, ROOT
from cut_support import smooth_frames, uniform_frames

F32 = np.float32
MEAN = (104.0, 177.0, 123.0)
BLOB = 300

# The share of bytes of resize_linear that differ from resize_yardstick64 (by one level: cv2's 11-bit coefficients and its two truncating
# shifts), the worst over the regions of CASES on uniform frames -- measured on the CPU by
#   python -c "import sys; sys.path.insert(0, 'tests'); import detect_support as D; print(D.measure_resize_share())"
# which printed 0.13163703703703702 (numpy on x86-64; integer and IEEE arithmetic only, so every machine gives this).  The test caps the
# header's share at 1.5 x this.
RESIZE_WORST_SHARE = 0.13163703703703702
RESIZE_MAX_LEVELS = 1

# key -> (shape [F, H, W, C], dtype, rotation mode, builder regions or None)
CASES = {
    "light_640x420": ((2, 420, 640, 3), "f32", "Light: ±15°", None),
    "strong_600x600_c4": ((1, 600, 600, 4), "f32", "Strong: ±15° and ±30°", None),
    "strong_97x61": ((2, 61, 97, 3), "f32", "Strong: ±15° and ±30°", None),
    "off_600x400": ((1, 400, 600, 3), "f32", "Off (fastest)", None),
    "builder_u8": ((2, 330, 500, 3), "u8", "light", [(17, 23, 25, 31), (100, 20, 400, 320), (381, 241, 500, 330)]),
}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def quantise_bgr(frames):
    """[..., C >= 3] fp32 R,G,B -> [..., 3] uint8 B,G,R: (clamp(x, 0, 1) * 255).round(), half to even, NaN gives 0"""
    x = np.asarray(frames, dtype=F32)[..., :3]
    with np.errstate(invalid="ignore"):
        r = np.rint(np.clip(x, F32(0.0), F32(1.0)) * F32(255.0))
    return np.where(np.isnan(r), F32(0.0), r).astype(np.uint8)[..., ::-1]


def rotation(width, height, angle):
    """(forward, inverse) float64 2 x 3: getRotationMatrix2D((W / 2.0, H / 2.0), angle, 1.0) and cv2's inversion, in its order"""
    a, b = math.cos(angle * math.pi / 180.0), math.sin(angle * math.pi / 180.0)
    cx, cy = width / 2.0, height / 2.0
    M = np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], dtype=np.float64)
    m = M.copy()
    D = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[1, 1] * D, m[0, 0] * D
    m[0, 0] = A11
    m[0, 1] *= -D
    m[1, 0] *= -D
    m[1, 1] = A22
    b1 = -m[0, 0] * m[0, 2] - m[0, 1] * m[1, 2]
    b2 = -m[1, 0] * m[0, 2] - m[1, 1] * m[1, 2]
    m[0, 2], m[1, 2] = b1, b2
    return M, m


def _round_sat(v):
    return np.clip(np.rint(v), -2147483648.0, 2147483647.0).astype(np.int64)


def warp_coordinates(inverse, width, height):
    """(sx, sy, fx, fy) int64 [H, W] of warpAffine's fixed-point walk"""
    m = np.asarray(inverse, dtype=np.float64).reshape(2, 3)
    x = np.arange(width, dtype=np.float64)
    y = np.arange(height, dtype=np.float64)
    adelta, bdelta = _round_sat(m[0, 0] * x * 1024.0), _round_sat(m[1, 0] * x * 1024.0)
    X0 = _round_sat((m[0, 1] * y + m[0, 2]) * 1024.0) + 16
    Y0 = _round_sat((m[1, 1] * y + m[1, 2]) * 1024.0) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    return np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767), X & 31, Y & 31


def _warp_taps(u8, inverse):
    H, W, _ = u8.shape
    sx, sy, fx, fy = warp_coordinates(inverse, W, H)
    x0, x1 = np.clip(sx, 0, W - 1), np.clip(sx + 1, 0, W - 1)
    y0, y1 = np.clip(sy, 0, H - 1), np.clip(sy + 1, 0, H - 1)
    S = u8.astype(np.int64)
    return (S[y0, x0], S[y0, x1], S[y1, x0], S[y1, x1]), fx[..., None], fy[..., None]


def warp_linear(u8, inverse):
    """cv2.warpAffine(u8, M, (W, H), INTER_LINEAR, BORDER_REPLICATE) of one [H, W, 3] byte image; `inverse` = the inverted M"""
    (p00, p01, p10, p11), fx, fy = _warp_taps(u8, inverse)
    total = (32 - fx) * (32 - fy) * 32 * p00 + fx * (32 - fy) * 32 * p01 + (32 - fx) * fy * 32 * p10 + fx * fy * 32 * p11
    return ((total + 16384) >> 15).astype(np.uint8)


def warp_yardstick64(u8, inverse):
    """the float64 bilinear filter at the same 1/32-pixel coordinates, rounded half up: the weights are exact, so this is what the
    fixed-point sum must give"""
    (p00, p01, p10, p11), fx, fy = _warp_taps(u8, inverse)
    ax, ay = fx.astype(np.float64) / 32.0, fy.astype(np.float64) / 32.0
    v = (1 - ay) * ((1 - ax) * p00 + ax * p01) + ay * ((1 - ax) * p10 + ax * p11)
    return np.floor(v + 0.5).astype(np.uint8)


def axis_taps(n_in, n_out, horizontal):
    """(s int64 [n_out], f float32 [n_out], c0, c1 int64 [n_out]) of one axis of resize(INTER_LINEAR, 8U)"""
    scale = 1.0 / (float(n_out) / float(n_in))
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    if horizontal:
        low = s < 0
        f, s = np.where(low, F32(0), f), np.where(low, 0, s)
        high = s >= n_in - 1
        f, s = np.where(high, F32(0), f).astype(F32), np.where(high, n_in - 1, s)
    c0 = np.rint((F32(1.0) - f) * F32(2048.0)).astype(np.int64)
    c1 = np.rint(f * F32(2048.0)).astype(np.int64)
    return s, f, c0, c1


def resize_linear(u8, n_out=BLOB):
    """cv2.resize(u8, (n_out, n_out)) of one [h, w, 3] byte image"""
    h, w, _ = u8.shape
    S = u8.astype(np.int64)
    if 1.0 / (float(n_out) / w) == 2.0 and 1.0 / (float(n_out) / h) == 2.0:
        return ((S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, _, cx0, cx1 = axis_taps(w, n_out, True)
    sy, _, cy0, cy1 = axis_taps(h, n_out, False)
    rows = S[:, sx] * cx0[None, :, None] + S[:, np.minimum(sx + 1, w - 1)] * cx1[None, :, None]
    r0, r1 = rows[np.clip(sy, 0, h - 1)], rows[np.clip(sy + 1, 0, h - 1)]
    out = (((cy0[:, None, None] * (r0 >> 4)) >> 16) + ((cy1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def resize_yardstick64(u8, n_out=BLOB):
    """float64 bilinear at cv2's float coordinates, rounded once (half to even)"""
    h, w, _ = u8.shape
    S = u8.astype(np.float64)
    sx, fx, _, _ = axis_taps(w, n_out, True)
    sy, fy, _, _ = axis_taps(h, n_out, False)
    fx, fy = fx.astype(np.float64)[None, :, None], fy.astype(np.float64)[:, None, None]
    rows = S[:, sx] * (1 - fx) + S[:, np.minimum(sx + 1, w - 1)] * fx
    v = rows[np.clip(sy, 0, h - 1)] * (1 - fy) + rows[np.clip(sy + 1, 0, h - 1)] * fy
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def to_blob(u8):
    """[300, 300, 3] B,G,R bytes -> fp32 [3, 300, 300]"""
    return (u8.astype(F32) - np.array(MEAN, dtype=F32)).transpose(2, 0, 1).copy()


def blob(bgr, inverse, region):
    """the composition: resize(warp(frame)[top:bottom, left:right]) as a blob; `inverse` None = no rotation"""
    left, top, right, bottom = region
    rotated = bgr if inverse is None else warp_linear(bgr, inverse)
    return to_blob(resize_linear(rotated[top:bottom, left:right]))


def regions_of(width, height, builder=False):
    regions = [(0, 0, width, height)]
    if width >= 600 and height >= 400:
        tw, th = (int(round(width * 0.60)), int(round(height * 0.70))) if builder else (int(width * 0.60), int(height * 0.70))
        regions += [(0, 0, tw, th), (width - tw, 0, width, th), (0, height - th, tw, height), (width - tw, height - th, width, height)]
    return regions


ANGLES = {"Off (fastest)": [0], "Light: ±15°": [0, -15, 15], "Strong: ±15° and ±30°": [0, -15, 15, -30, 30],
          "off": [0], "light": [0, -15, 15], "strong": [0, -15, 15, -30, 30]}


def as_bgr(frames):
    x = np.asarray(frames)
    return x if x.dtype == np.uint8 else quantise_bgr(x)


def restated_blobs(frames, mode, builder_regions=None):
    """[F, A, R, 3, 300, 300] fp32 of the restatement (a slot that is not scanned is zeros), and the rotated frames [F, A, H, W, 3]"""
    bgr = as_bgr(frames)
    F, H, W, _ = bgr.shape
    angles = ANGLES[mode]
    builder = builder_regions is not None
    per_angle = [list(builder_regions) if (builder and a == 0) else regions_of(W, H, builder) for a in angles]
    slots = max(len(r) for r in per_angle)
    out = np.zeros((F, len(angles), slots, 3, BLOB, BLOB), dtype=F32)
    rotated = np.zeros((F, len(angles), H, W, 3), dtype=np.uint8)
    for f in range(F):
        for a, angle in enumerate(angles):
            inverse = None if angle == 0 else rotation(W, H, angle)[1]
            rotated[f, a] = bgr[f] if inverse is None else warp_linear(bgr[f], inverse)
            for r, (left, top, right, bottom) in enumerate(per_angle[a]):
                if right - left < 8 or bottom - top < 8:
                    continue
                out[f, a, r] = to_blob(resize_linear(rotated[f, a][top:bottom, left:right]))
    return out, rotated


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def special_frames(shape, seed):
    """NaN, +-inf, the 0.5 / 255 ties of the quantisation, values outside [0, 1], k / 255 one ulp up and down, and a constant frame"""
    F, H, W, Cn = shape
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    k = rng.integers(0, 256, shape).astype(F32) / F32(255.0)
    pick = rng.integers(0, 10, shape)
    half = (rng.integers(0, 255, shape).astype(F32) + F32(0.5)) / F32(255.0)
    x = k.copy()
    for value, replacement in ((0, np.nextafter(k, F32(2.0))), (1, np.nextafter(k, F32(-1.0))), (2, half), (3, F32(np.nan)), (4, F32(np.inf)),
                               (5, F32(-np.inf)), (6, F32(-0.37)), (7, F32(1.6))):
        x = np.where(pick == value, replacement, x).astype(F32)
    x[0, : H // 2] = F32(0.5)                                                      # a constant half (tie: 127.5 -> 128)
    return x


FRAME_KINDS = {"uniform": uniform_frames, "smooth": smooth_frames, "special": special_frames}


def make_frames(kind, shape, dtype, seed):
    """the frames of a case: fp32 R,G,B of the kind, or -- dtype "u8" -- their quantised B,G,R bytes"""
    x = FRAME_KINDS[kind](tuple(shape), seed)
    return np.ascontiguousarray(quantise_bgr(x)) if dtype == "u8" else np.ascontiguousarray(x, dtype=F32)


def case_frames(key, kind="uniform"):
    shape, dtype, _, _ = CASES[key]
    return make_frames(kind, shape, dtype, 900 + sum(map(ord, key)))


def differences(got, want):
    """(largest difference in levels, share of differing values)"""
    d = np.abs(np.asarray(got, dtype=np.int16) - np.asarray(want, dtype=np.int16))
    return (int(d.max()), float((d != 0).mean())) if d.size else (0, 0.0)


def case_regions(key):
    """every (h, w) region the case resizes"""
    shape, _, mode, regions = CASES[key]
    _, H, W, _ = shape
    out = set((b - t, r - l) for l, t, r, b in regions_of(W, H, regions is not None))
    if regions:
        out |= set((b - t, r - l) for l, t, r, b in regions if r - l >= 8 and b - t >= 8)
    return sorted(out)


def measure_resize_share():
    """the worst share of bytes that differ between resize_linear and resize_yardstick64 over the regions of CASES"""
    worst = 0.0
    for key in sorted(CASES):
        bgr = as_bgr(case_frames(key))[0]
        for h, w in case_regions(key):
            levels, share = differences(resize_linear(bgr[:h, :w]), resize_yardstick64(bgr[:h, :w]))
            assert levels <= RESIZE_MAX_LEVELS, (key, h, w, levels)
            worst = max(worst, share)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------------
# the header on the host
# ---------------------------------------------------------------------------------------------------------------------------------------
def build_host_lib(directory):
    out = os.path.join(str(directory), "libdetect_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "detect_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    P = C.c_void_p
    lib.hm_detect_taps.argtypes = [C.c_int32, C.c_int32, P, P]
    lib.hm_detect_taps.restype = None
    lib.hm_detect_rotation.argtypes = [C.c_double, C.c_double, C.c_int32, C.c_int32, P, P]
    lib.hm_detect_rotation.restype = None
    lib.hm_detect_quantise.argtypes = [P, P, C.c_int32, C.c_int32, C.c_int32]
    lib.hm_detect_quantise.restype = None
    lib.hm_detect_warp.argtypes = [P, P, P, C.c_int32, C.c_int32]
    lib.hm_detect_warp.restype = None
    lib.hm_detect_resize.argtypes = [P, P, C.c_int32, C.c_int32, C.c_int32]
    lib.hm_detect_resize.restype = None
    lib.hm_detect_blob.argtypes = [P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, P, C.c_int64, P, P]
    lib.hm_detect_blob.restype = C.c_int
    return lib


def host_quantise(lib, frame):
    x = np.ascontiguousarray(frame, dtype=F32)
    out = np.empty(x.shape[:2] + (3,), dtype=np.uint8)
    lib.hm_detect_quantise(x.ctypes.data, out.ctypes.data, x.shape[0], x.shape[1], x.shape[2])
    return out


def host_warp(lib, u8, inverse):
    x = np.ascontiguousarray(u8)
    m = np.ascontiguousarray(inverse, dtype=np.float64).reshape(6)
    out = np.empty_like(x)
    lib.hm_detect_warp(x.ctypes.data, out.ctypes.data, m.ctypes.data, x.shape[0], x.shape[1])
    return out


def host_resize(lib, u8, n_out=BLOB):
    x = np.ascontiguousarray(u8)
    out = np.empty((n_out, n_out, 3), dtype=np.uint8)
    lib.hm_detect_resize(x.ctypes.data, out.ctypes.data, x.shape[0], x.shape[1], n_out)
    return out


def host_blob(lib, frames, transforms, desc):
    """(fp32 [3, 300, 300], accepted) of one descriptor (six integers) through the fused route of the header"""
    x = np.ascontiguousarray(frames)
    t = np.ascontiguousarray(transforms, dtype=np.float64).reshape(-1, 6)
    d = np.array([int(v) for v in desc], dtype=np.int32)
    out = np.empty((3, BLOB, BLOB), dtype=F32)
    ok = lib.hm_detect_blob(x.ctypes.data, int(x.dtype != np.uint8), x.shape[0], x.shape[1], x.shape[2], x.shape[3], t.ctypes.data if t.size else None,
                            len(t), d.ctypes.data, out.ctypes.data)
    return out, bool(ok)


def host_taps(lib, n_in, n_out=BLOB):
    ofs = np.zeros(2 * n_out, dtype=np.int32)
    coef = np.zeros(4 * n_out, dtype=np.int16)
    lib.hm_detect_taps(n_in, n_out, ofs.ctypes.data, coef.ctypes.data)
    return ofs, coef.reshape(2, n_out, 2)


def golden_path():
    return os.path.join(GOLDEN, "detect_prep.json")


def cv2_fixture_path():
    return os.path.join(GOLDEN, "detect_cv2.npz")

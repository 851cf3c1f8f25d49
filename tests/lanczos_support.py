"""Shared by tests/test_lanczos_host.py and tests/test_gpu_lanczos.py.

``restated``: OpenCV 4.x's uint8 resize(..., INTER_LANCZOS4) restated in numpy from the text of the specification (the weights with
math.sin / math.cos in double, everything after them in integers) -- written independently of csrc/vrg_lanczos_math.hpp, which must give
the same bytes on the host (tests/host_math/lanczos_check.cpp) and on the GPU.
``yardstick64``: the mathematical filter in float64 -- weights sinc(x) * sinc(x / 4) over the same eight taps, normalised, same half-pixel
centres and edge clamp, ONE final rounding.  The bytes may differ from it by at most one level on at most 15 % of the values: the
11-bit weights and the rounding of the intermediate are the only differences."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from conftest import GOLDEN, PKG_DIR, ROOT

U8P = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
FLT_EPSILON = float(np.finfo(np.float32).eps)
S45 = 0.70710678118654752440084436210485
CS = ((1.0, 0.0), (-S45, -S45), (0.0, 1.0), (S45, -S45), (-1.0, 0.0), (S45, S45), (0.0, -1.0), (-S45, S45))
YARDSTICK_MAX_LEVELS = 1
YARDSTICK_MAX_SHARE = 0.15


def axis_table(n_in, n_out):
    """(s [n_out] int64, w [n_out, 8] int32) of one axis"""
    f32 = np.float32
    scale = float(n_in) / float(n_out)
    s = np.empty(n_out, dtype=np.int64)
    w = np.zeros((n_out, 8), dtype=np.int32)
    for d in range(n_out):
        fx = f32((d + 0.5) * scale - 0.5)
        fl = math.floor(float(fx))
        t = f32(fx - f32(fl))
        s[d] = fl
        if float(t) < FLT_EPSILON:
            w[d, 3] = 2048
            continue
        y0 = -float(f32(t + f32(3.0))) * math.pi * 0.25
        s0, c0 = math.sin(y0), math.cos(y0)
        coeffs = []
        total = f32(0.0)
        for i in range(8):
            y = -float(f32(f32(t + f32(3.0)) - f32(i))) * math.pi * 0.25
            c = f32((CS[i][0] * s0 + CS[i][1] * c0) / (y * y))
            coeffs.append(c)
            total = f32(total + c)
        inv = f32(f32(1.0) / total)
        for i in range(8):
            w[d, i] = int(np.rint(f32(f32(coeffs[i] * inv) * f32(2048.0))))
    return s, w


def restated(frames, out_w, out_h):
    """[F, H, W, 3] uint8 -> [F, out_h, out_w, 3] uint8"""
    x = np.ascontiguousarray(frames, dtype=np.uint8)
    F, H, W, _ = x.shape
    if (W, H) == (out_w, out_h):
        return frames
    sx, wx = axis_table(W, out_w)
    sy, wy = axis_table(H, out_h)
    ix = np.clip(sx[:, None] + np.arange(-3, 5)[None, :], 0, W - 1)          # [out_w, 8]
    iy = np.clip(sy[:, None] + np.arange(-3, 5)[None, :], 0, H - 1)          # [out_h, 8]
    src = x.astype(np.int32)
    hor = np.zeros((F, H, out_w, 3), dtype=np.int32)
    for k in range(8):
        hor += src[:, :, ix[:, k], :] * wx[None, None, :, k, None]
    ver = np.zeros((F, out_h, out_w, 3), dtype=np.int32)
    for k in range(8):
        ver += hor[:, iy[:, k], :, :] * wy[None, :, k, None, None]
    return np.clip((ver + np.int32(1 << 21)) >> 22, 0, 255).astype(np.uint8)


def _weights64(n_in, n_out):
    d = np.arange(n_out, dtype=np.float64)
    fx = (d + 0.5) * (n_in / n_out) - 0.5
    s = np.floor(fx)
    t = fx - s
    offs = np.arange(-3, 5, dtype=np.float64)
    xx = t[:, None] - offs[None, :]                                          # distance of tap k from the sample point
    w = np.sinc(xx) * np.sinc(xx / 4.0)
    w /= w.sum(axis=1, keepdims=True)
    idx = np.clip(s[:, None].astype(np.int64) + np.arange(-3, 5)[None, :], 0, n_in - 1)
    return idx, w


def yardstick64(frames, out_w, out_h):
    x = np.asarray(frames, dtype=np.float64)
    F, H, W, _ = x.shape
    ix, wx = _weights64(W, out_w)
    iy, wy = _weights64(H, out_h)
    hor = np.zeros((F, H, out_w, 3))
    for k in range(8):
        hor += x[:, :, ix[:, k], :] * wx[None, None, :, k, None]
    ver = np.zeros((F, out_h, out_w, 3))
    for k in range(8):
        ver += hor[:, iy[:, k], :, :] * wy[None, :, k, None, None]
    return np.clip(np.rint(ver), 0, 255).astype(np.uint8)


def random_frames(shape, seed):
    return np.random.Generator(np.random.PCG64(int(seed))).integers(0, 256, size=tuple(shape), dtype=np.uint8)


def smooth_frames(shape, seed):
    F, H, W, _ = shape
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty(shape, dtype=np.uint8)
    for f in range(F):
        for c in range(3):
            a, b, p = rng.uniform(0.02, 0.12, 3)
            out[f, :, :, c] = np.clip(127.5 + 120.0 * np.sin(a * xx + p) * np.cos(b * yy - p), 0, 255).astype(np.uint8)
    return out


def has_both_column_kinds(column_s, in_w):
    """Of the columns of a table (their ``s``): do some read their eight pixels as one 24-byte window (taps s - 3 .. s + 4 inside the row)
    and some gather them clamped?  With in_w == 8 the only window is s == 3, the row's 24 bytes exactly."""
    s = np.asarray(column_s)
    window = (s >= 3) & (s <= in_w - 5)
    return bool(window.any() and not window.all()) and (in_w != 8 or bool((s[window] == 3).all()))


def build_host_lib(directory):
    out = os.path.join(str(directory), "liblanczos_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "lanczos_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_lanczos4.argtypes = [U8P, U8P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.hm_lanczos4.restype = None
    lib.hm_lanczos4_taps.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.hm_lanczos4_taps.restype = None
    return lib


def host_resize(lib, frames, out_w, out_h):
    x = np.ascontiguousarray(frames, dtype=np.uint8)
    out = np.empty((x.shape[0], int(out_h), int(out_w), 3), dtype=np.uint8)
    lib.hm_lanczos4(x, out, x.shape[0], x.shape[1], x.shape[2], int(out_h), int(out_w))
    return out


def differences(got, want):
    """(largest difference in levels, share of differing values)"""
    d = np.abs(np.asarray(got, dtype=np.int16) - np.asarray(want, dtype=np.int16))
    return int(d.max()) if d.size else 0, float((d != 0).mean()) if d.size else 0.0


def cv2_fixture_path():
    return os.path.join(GOLDEN, "lanczos4_cv2.npz")

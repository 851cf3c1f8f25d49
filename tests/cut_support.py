"""Shared by tests/test_cut_host.py, tests/test_gpu_cut.py and tools/make_golden_cut.py.

``thumbnails`` / ``histograms`` / ``pair_sums``: the cut score's device half restated in numpy from the text of the specification
(OpenCV 4.x: the byte quantisation, resize(..., (64, 64), INTER_AREA) with its tap table, fp32 summation order and integer fast path,
cvtColor's fixed-point RGB2HSV, calcHist's bins) -- written independently of csrc/vrg_area_math.hpp, which must give the same values on the
host (tests/host_math/cut_check.cpp) and on the GPU.
``yardstick64``: the exact area average in float64, rounded once.  The thumbnails may differ from it by at most one level on at most 1 % of
the bytes: the fp32 sums are the only difference.
``make_video``: the seeded synthetic videos of tests/golden/cut_score.json (hard cuts, fades, flashes, identical and single-colour frames)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from conftest import GOLDEN, PKG_DIR, ROOT, load_package

F32 = np.float32
U8P = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
F32P = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
I64P = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
YARDSTICK_MAX_LEVELS = 1
YARDSTICK_MAX_SHARE = 0.01
_hip = load_package()._hip
CELL = _hip.record_dtype(_hip.AreaCell)

# (height, width, channels): the sizes of the issue
SIZES = ((2160, 3840, 3), (1080, 1920, 3), (720, 1280, 3), (480, 854, 3), (512, 512, 3), (128, 128, 3), (64, 64, 3), (65, 67, 3), (64, 4096, 3),
         (96, 130, 4), (1080, 1920, 4))
# rows just past one wave's row buffer (W * C + 4 > CUT_ROW_MAX): k_cut_thumbs stages them 32 cells at a time
SEGMENTED_SIZES = ((64, 4864, 3), (65, 4850, 3), (64, 3640, 4))
CUT_ROW_MAX = ((65536 - 7424) // 4) & ~15          # bytes of one wave's row buffer at most (csrc/vrg_cut.hip)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def quantise(frames):
    """[..., C >= 3] fp32 -> [..., 3] uint8: rint(clamp(x, 0, 1) * 255) in fp32, round half to even"""
    x = np.asarray(frames, dtype=F32)[..., :3]
    return np.rint(np.clip(x, F32(0.0), F32(1.0)) * F32(255.0)).astype(np.uint8)


def axis_taps(n_in, n_out=64):
    """computeResizeAreaTab: [(d, s, alpha fp32)] in table order"""
    scale = n_in / n_out
    out = []
    for d in range(n_out):
        fs1 = d * scale
        fs2 = fs1 + scale
        cell = min(scale, n_in - fs1)
        s1, s2 = math.ceil(fs1), min(math.floor(fs2), n_in - 1)
        s1 = min(s1, s2)
        if s1 - fs1 > 1e-3:
            out.append((d, s1 - 1, F32((s1 - fs1) / cell)))
        for s in range(s1, s2):
            out.append((d, s, F32(1.0 / cell)))
        if fs2 - s2 > 1e-3:
            out.append((d, s2, F32(min(min(fs2 - s2, 1.0), cell) / cell)))
    return out


def cells_per_segment(width, channels):
    """cut_segments of csrc/vrg_cut.hip restated from the tap table: the most cells (64, 32, .. 1) whose samples, for every aligned run of
    that many cells, fit the row buffer with the 4 bytes of the phase; 0: not even one cell does"""
    taps = axis_taps(width)
    first = [min(s for d, s, _ in taps if d == i) for i in range(64)]
    end = [max(s for d, s, _ in taps if d == i) + 1 for i in range(64)]
    cps = 64
    while cps and max((end[d0 + cps - 1] - first[d0]) * channels for d0 in range(0, 64, cps)) + 4 > CUT_ROW_MAX:
        cps >>= 1
    return cps


def _padded(taps, n_out=64):
    per = [[t for t in taps if t[0] == d] for d in range(n_out)]
    depth = max(len(p) for p in per)
    idx = np.zeros((n_out, depth), dtype=np.int64)
    w = np.zeros((n_out, depth), dtype=F32)
    cnt = np.array([len(p) for p in per])
    for d, p in enumerate(per):
        for k, (_, s, a) in enumerate(p):
            idx[d, k], w[d, k] = s, a
    return idx, w, cnt


def _area_general(u8):
    """one [H, W, 3] byte frame through resizeArea_<uchar, float>: fp32, two roundings per term, the sums in table order"""
    H, W, _ = u8.shape
    S = u8.astype(F32)
    ix, wx, cx = _padded(axis_taps(W))
    iy, wy, cy = _padded(axis_taps(H))
    buf = np.zeros((H, 64, 3), dtype=F32)
    for k in range(ix.shape[1]):
        on = cx > k
        buf[:, on, :] = buf[:, on, :] + S[:, ix[on, k], :] * wx[on, k][None, :, None]
    out = np.zeros((64, 64, 3), dtype=F32)
    for k in range(iy.shape[1]):
        on = cy > k
        term = wy[on, k][:, None, None] * buf[iy[on, k]]
        out[on] = term if k == 0 else out[on] + term
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def _area_fast(u8):
    H, W, _ = u8.shape
    sy, sx = H // 64, W // 64
    total = u8.astype(np.int64).reshape(64, sy, 64, sx, 3).sum(axis=(1, 3))
    if (sy, sx) == (2, 2):
        return ((total + 2) >> 2).astype(np.uint8)
    scale = F32(1.0) / F32(sx * sy)
    return np.clip(np.rint(total.astype(F32) * scale), 0, 255).astype(np.uint8)


def resize_area_u8(u8):
    """cv2.resize(u8, (64, 64), interpolation=cv2.INTER_AREA) of one [H >= 64, W >= 64, 3] byte image"""
    H, W, _ = u8.shape
    if H < 64 or W < 64:
        raise ValueError("sides below 64 px take another route in cv2: not restated")
    return _area_fast(u8) if H % 64 == 0 and W % 64 == 0 else _area_general(u8)


def thumbnails(frames):
    """[F, H, W, C >= 3] fp32 -> [F, 64, 64, 3] uint8"""
    x = np.asarray(frames)
    out = np.empty((x.shape[0], 64, 64, 3), dtype=np.uint8)
    for f in range(x.shape[0]):
        out[f] = resize_area_u8(quantise(x[f]))
    return out


SDIV = np.array([0] + [int(np.rint((255 << 12) / float(i))) for i in range(1, 256)], dtype=np.int64)
HDIV = np.array([0] + [int(np.rint((180 << 12) / (6.0 * i))) for i in range(1, 256)], dtype=np.int64)


def hsv(rgb):
    """(h, s) of uint8 R,G,B pixels: cvtColor(COLOR_RGB2HSV), 12-bit fixed point"""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * SDIV[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + 2048) >> 12
    return np.where(h < 0, h + 180, h), s


def histograms(thumbs):
    """[F, 64, 64, 3] uint8 -> int32 [F, 1024]"""
    out = np.zeros((len(thumbs), 1024), dtype=np.int32)
    for f, t in enumerate(thumbs):
        h, s = hsv(t)
        out[f] = np.bincount(((8 * h) // 45 * 32 + (s >> 3)).ravel(), minlength=1024)
    return out


def pair_sums(thumbs, hists):
    """int64 [F - 1, 4] = (D, S11, S22, S12)"""
    n = max(len(thumbs) - 1, 0)
    out = np.zeros((n, 4), dtype=np.int64)
    t, h = thumbs.astype(np.int64), hists.astype(np.int64)
    for i in range(n):
        out[i] = (np.abs(t[i] - t[i + 1]).sum(), (h[i] * h[i]).sum(), (h[i + 1] * h[i + 1]).sum(), (h[i] * h[i + 1]).sum())
    return out


def _overlap(n_in, n_out=64):
    m = np.zeros((n_out, n_in))
    scale = n_in / n_out
    for i in range(n_out):
        a, b = i * scale, (i + 1) * scale
        for s in range(int(math.floor(a)), min(n_in, int(math.ceil(b)))):
            m[i, s] = (min(b, s + 1) - max(a, s)) / scale
    return m


def yardstick64(frames, ties="even"):
    """the exact area average of the quantised frames in float64, rounded once -- half to even as rint does, or (ties="up") half up, which
    is what cv2's (a + b + c + d + 2) >> 2 rule for 128 x 128 sources does with the quarters it can meet exactly"""
    x = np.asarray(frames)
    F, H, W, _ = x.shape
    my, mx = _overlap(H), _overlap(W)
    out = np.empty((F, 64, 64, 3), dtype=np.uint8)
    for f in range(F):
        o = np.einsum("ih,hwc->iwc", my, quantise(x[f]).astype(np.float64))
        o = np.einsum("jw,iwc->ijc", mx, o)
        out[f] = np.clip(np.floor(o + 0.5) if ties == "up" else np.rint(o), 0, 255).astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.PCG64(int(seed)))


def uniform_frames(shape, seed):
    return _rng(seed).random(tuple(shape), dtype=F32)


def _scene(rng, H, W, C):
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    out = np.empty((H, W, C), dtype=F32)
    for c in range(C):
        a, b, p = rng.uniform(0.004, 0.05, 3)
        base, amp = rng.uniform(0.25, 0.75), rng.uniform(0.1, 0.45)
        out[:, :, c] = base + amp * np.sin(a * xx + 40.0 * p) * np.cos(b * yy - 25.0 * p)
    return out


def smooth_frames(shape, seed):
    """video-like: one smooth scene that drifts a little from frame to frame, with sensor noise; values leave [0, 1] here and there"""
    F, H, W, C = shape
    rng = _rng(seed)
    scene = _scene(rng, H, W, C)
    out = np.empty(tuple(shape), dtype=F32)
    for f in range(F):
        out[f] = np.roll(scene, 3 * f, axis=1) + rng.normal(0.0, 0.02, (H, W, C)).astype(F32)
    return out


def special_frames(shape, seed):
    """constant frames and frames made of exact 0, 1, out-of-range values and k / 255 one ulp up and down"""
    F, H, W, C = shape
    rng = _rng(seed)
    k = rng.integers(0, 256, (F, H, W, C)).astype(F32) / F32(255.0)
    pick = rng.integers(0, 7, (F, H, W, C))
    x = np.where(pick == 0, np.nextafter(k, F32(2.0)), np.where(pick == 1, np.nextafter(k, F32(-1.0)), k)).astype(F32)
    x = np.where(pick == 2, F32(0.0), np.where(pick == 3, F32(1.0), np.where(pick == 4, F32(-0.37), np.where(pick == 5, F32(1.6), x)))).astype(F32)
    half = (rng.integers(0, 255, (F, H, W, C)).astype(F32) + F32(0.5)) / F32(255.0)          # near the rounding ties of the quantisation
    x = np.where(pick == 6, half, x).astype(F32)
    x[0] = F32(0.5)                                                                         # a constant frame (tie: 127.5 -> 128)
    if F > 1:
        x[1] = F32(100.0 / 255.0)
    return x


FRAME_KINDS = {"uniform": uniform_frames, "smooth": smooth_frames, "special": special_frames}


def make_video(kind, shape, seed):
    """The seeded videos of the golden cases, [F, H, W, C] fp32."""
    F, H, W, C = shape
    rng = _rng(seed)
    a, b, c = (np.clip(_scene(rng, H, W, C), 0, 1).astype(F32) for _ in range(3))

    def noisy(img):
        return (img + rng.normal(0.0, 0.01, img.shape).astype(F32)).astype(F32)

    if kind == "hard_cuts":                       # three shots
        cut1, cut2 = F // 3, (2 * F) // 3
        frames = [noisy(np.roll(a if f < cut1 else (b if f < cut2 else c), 2 * f, axis=1)) for f in range(F)]
    elif kind == "cut_to_noise":
        frames = [noisy(a) if f < F // 2 else rng.random((H, W, C), dtype=F32) for f in range(F)]
    elif kind == "fade":                          # a slow cross-fade: no cut
        frames = [noisy(a * F32(1.0 - f / (F - 1)) + b * F32(f / (F - 1))) for f in range(F)]
    elif kind == "fast_fade":                     # a cross-fade over three frames in the middle
        t = np.clip((np.arange(F) - (F // 2 - 1)) / 2.0, 0.0, 1.0)
        frames = [noisy(a * F32(1.0 - t[f]) + b * F32(t[f])) for f in range(F)]
    elif kind == "flash":                         # one frame blown out
        frames = [noisy(np.roll(a, f, axis=1)) for f in range(F)]
        frames[F // 2] = (frames[F // 2] * F32(1.5) + F32(0.45)).astype(F32)
    elif kind == "identical":
        frames = [a.copy() for _ in range(F)]
    elif kind == "single_colour":                 # constant frames: the colour changes now and then
        colours = rng.random((F, C), dtype=F32)
        for f in range(1, F):
            if f % 3:
                colours[f] = colours[f - 1]
        frames = [np.broadcast_to(colours[f], (H, W, C)).copy() for f in range(F)]
    elif kind == "black_white":
        frames = [np.full((H, W, C), F32(f % 2), dtype=F32) for f in range(F)]
    elif kind == "drift":                         # one shot, a pan and a slow brightness change
        frames = [noisy(np.roll(a, 5 * f, axis=1) * F32(1.0 - 0.02 * f)) for f in range(F)]
    elif kind == "cut_same_palette":              # the same picture mirrored: same colours, other places
        frames = [noisy(a if f < F // 2 else a[:, ::-1]) for f in range(F)]
    elif kind == "out_of_range":
        frames = [(noisy(a if f < F // 2 else b) * F32(1.8) - F32(0.4)).astype(F32) for f in range(F)]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.stack(frames), dtype=F32)


def restated_sums(frames):
    """(thumbnails, histograms, pair sums) of the restatement"""
    t = thumbnails(frames)
    h = histograms(t)
    return t, h, pair_sums(t, h)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the header on the host
# ---------------------------------------------------------------------------------------------------------------------------------------
def build_host_lib(directory):
    out = os.path.join(str(directory), "libcut_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "cut_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_area_taps.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
    lib.hm_area_taps.restype = None
    lib.hm_area_mode.argtypes = [C.c_int32, C.c_int32]
    lib.hm_area_mode.restype = C.c_int32
    lib.hm_cut_thumbs.argtypes = [F32P, U8P, C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.hm_cut_thumbs.restype = None
    lib.hm_cut_hist.argtypes = [U8P, I32P, C.c_int64]
    lib.hm_cut_hist.restype = None
    lib.hm_cut_pair_sums.argtypes = [U8P, I32P, I64P, C.c_int64]
    lib.hm_cut_pair_sums.restype = None
    lib.hm_cut_hsv.argtypes = [C.c_int32] * 3 + [C.POINTER(C.c_int32)] * 2
    lib.hm_cut_hsv.restype = None
    return lib


def host_sums(lib, frames):
    """(thumbnails, histograms, pair sums) of the host-compiled header"""
    x = np.ascontiguousarray(frames, dtype=F32)
    F, H, W, Cn = x.shape
    t = np.empty((F, 64, 64, 3), dtype=np.uint8)
    lib.hm_cut_thumbs(x, t, F, H, W, Cn)
    h = np.empty((F, 1024), dtype=np.int32)
    lib.hm_cut_hist(t, h, F)
    s = np.zeros((max(F - 1, 0), 4), dtype=np.int64)
    lib.hm_cut_pair_sums(t, h, s, F)
    return t, h, s


def cells_of(lib, H, W):
    cells = np.zeros(128, dtype=CELL)
    lib.hm_area_taps(H, W, cells.ctypes.data)
    return cells


def expand_cells(cells):
    """[(d, s, alpha)] of 64 AreaCell records, in table order"""
    out = []
    for d, c in enumerate(cells):
        for k in range(int(c["count"])):
            w = c["w_first"] if k == 0 else (c["w_last"] if k == int(c["count"]) - 1 else c["w_mid"])
            out.append((d, int(c["first"]) + k, F32(w)))
    return out


def differences(got, want):
    """(largest difference in levels, share of differing values)"""
    d = np.abs(np.asarray(got, dtype=np.int16) - np.asarray(want, dtype=np.int16))
    return int(d.max()) if d.size else 0, float((d != 0).mean()) if d.size else 0.0


def golden_path():
    return os.path.join(GOLDEN, "cut_score.json")


def cv2_fixture_path():
    return os.path.join(GOLDEN, "cut_score_cv2.npz")

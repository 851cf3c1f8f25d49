"""Shared by tests/test_grid_host.py, tests/test_gpu_grid.py and tools/make_golden_grid.py.

``quantise`` / ``resize_area`` / ``fit_tile`` / ``grid_frames``: the Video Folder Grid Plot restated in numpy from the text of the
specification (numpy's truncating quantisation, OpenCV 4.x's resize(..., INTER_AREA) on bytes with its copy, integer, general and -- when an
axis enlarges -- bilinear rules, the tile and grid geometry of the reference node), as whole-image steps: quantise, then the horizontal pass
of every row, then the vertical pass.  Written independently of csrc/vrg_grid_math.hpp, which must give the same bytes on the host
(tests/host_math/grid_check.cpp) and the same floats on the GPU.
``area_yardstick64`` / ``linear_yardstick64``: the exact area average and the bilinear filter at the same (s, f) in float64, rounded once.
``GEOMETRIES``: the (source -> tile) pairs of the GPU sweep."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from conftest import GOLDEN, PKG_DIR, ROOT, load_package
from cut_support import smooth_frames, uniform_frames

F32 = np.float32
COPY, FAST, FAST_2X2, GENERAL, LINEAR = 0, 1, 2, 3, 4
MODE_NAMES = {COPY: "copy", FAST: "fast", FAST_2X2: "fast 2x2", GENERAL: "general", LINEAR: "linear"}
_hip = load_package()._hip
CELL = _hip.record_dtype(_hip.AreaCell)
LABEL_BAND = 40

# source (H, W) -> tile (h, w), the rule it takes
GEOMETRIES = (
    ((48, 64), (48, 64), COPY),
    ((96, 128), (48, 64), FAST_2X2),
    ((96, 192), (32, 64), FAST),
    ((64, 120), (32, 40), FAST),
    ((70, 131), (30, 57), GENERAL),
    ((67, 65), (29, 31), GENERAL),
    ((7, 100), (4, 50), GENERAL),
    ((33, 17), (1, 1), FAST),
    ((12, 20), (38, 64), LINEAR),
    ((5, 3), (64, 37), LINEAR),
    ((48, 20), (48, 64), LINEAR),
    ((600, 64), (320, 34), GENERAL),
    ((4, 20000), (2, 9000), GENERAL),
    ((4, 4000), (2, 64), GENERAL),          # 64 columns need more source values than a wave stages at a time: segments of columns
    ((8, 3840), (4, 120), FAST),            # the same on the integer path
    ((8, 953), (8, 413), GENERAL),          # 1.0 / (413.0 / 953) and 953 / 413.0 give different cells (scale_formations_differ)
)
SEGMENTED = (((4, 4000), (2, 64)), ((8, 3840), (4, 120)))      # the geometries above whose plan has cps < 64
# hm_grid_scale_pairs of tests/host_math/grid_check.cpp: (limit, pairs n_out <= n_in <= limit whose general-rule cells differ between the two
# formations of the scale, the first such pair (n_in, n_out))
SCALE_PAIRS_1024 = (1024, 44, (953, 413))
SCALE_PAIRS_4096 = (4096, 27025, (953, 413))

# The share of bytes that differ (by one level) from the float64 filters, the worst over GEOMETRIES on uniform and smooth frames, measured
# on the restatement by
#   python -c "import sys; sys.path.insert(0, 'tests'); import grid_support as G; print(G.measure_shares())"
# (numpy on x86-64; integer and IEEE arithmetic only, so every machine gives this).  The tests cap the header's share at 1.5 x these.
AREA_WORST_SHARE = 0.02
LINEAR_WORST_SHARE = 0.04454495614035088
YARDSTICK_MAX_LEVELS = 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def quantise(frames):
    """[..., C >= 3] fp32 -> [..., 3] uint8: np.clip(x * 255.0, 0, 255).astype(np.uint8) -- truncation; NaN (undefined in numpy) gives 0"""
    x = np.asarray(frames, dtype=F32)[..., :3]
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.clip(x * F32(255.0), F32(0.0), F32(255.0))
    return np.where(np.isnan(t), F32(0.0), t).astype(np.uint8)


def scales(n_in, n_out):
    inv = float(n_out) / float(n_in)
    return inv, 1.0 / inv


def _is_int(scale):
    i = int(np.rint(scale))
    return abs(scale - i) < np.finfo(np.float64).eps, i


def mode_of(H, W, h, w):
    if (H, W) == (h, w):
        return COPY
    sx, sy = scales(W, w)[1], scales(H, h)[1]
    if not (sx >= 1.0 and sy >= 1.0):
        return LINEAR
    (okx, ix), (oky, iy) = _is_int(sx), _is_int(sy)
    if not (okx and oky):
        return GENERAL
    return FAST_2X2 if (ix, iy) == (2, 2) else FAST


def area_taps(n_in, n_out, scale=None):
    """computeResizeAreaTab with scale = 1.0 / ((double)n_out / n_in) unless another is handed in: [(d, s, alpha fp32)] in table order"""
    scale = scales(n_in, n_out)[1] if scale is None else scale
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


def scale_formations_differ(n_in, n_out):
    """do the general-rule taps change when the scale is formed as n_in / n_out instead of 1.0 / (n_out / n_in)"""
    return area_taps(n_in, n_out) != area_taps(n_in, n_out, scale=n_in / n_out)


def _padded(taps, n_out):
    per = [[] for _ in range(n_out)]
    for t in taps:
        per[t[0]].append(t)
    depth = max(len(p) for p in per)
    idx = np.zeros((n_out, depth), dtype=np.int64)
    w = np.zeros((n_out, depth), dtype=F32)
    cnt = np.array([len(p) for p in per])
    for d, p in enumerate(per):
        for k, (_, s, a) in enumerate(p):
            idx[d, k], w[d, k] = s, a
    return idx, w, cnt


def _area_general(u8, h, w):
    """resizeArea_<uchar, float>: fp32, two roundings per term, the sums in table order: every row horizontally, then vertically"""
    H, W, _ = u8.shape
    S = u8.astype(F32)
    ix, wx, cx = _padded(area_taps(W, w), w)
    iy, wy, cy = _padded(area_taps(H, h), h)
    buf = np.zeros((H, w, 3), dtype=F32)
    for k in range(ix.shape[1]):
        on = cx > k
        buf[:, on, :] = buf[:, on, :] + S[:, ix[on, k], :] * wx[on, k][None, :, None]
    out = np.zeros((h, w, 3), dtype=F32)
    for k in range(iy.shape[1]):
        on = cy > k
        term = wy[on, k][:, None, None] * buf[iy[on, k]]
        out[on] = term if k == 0 else out[on] + term
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def _area_fast(u8, h, w):
    H, W, _ = u8.shape
    sy, sx = int(np.rint(scales(H, h)[1])), int(np.rint(scales(W, w)[1]))
    total = u8[:h * sy, :w * sx].astype(np.int64).reshape(h, sy, w, sx, 3).sum(axis=(1, 3))
    if (sy, sx) == (2, 2):
        return ((total + 2) >> 2).astype(np.uint8)
    return np.clip(np.rint(total.astype(F32) * (F32(1.0) / F32(sx * sy))), 0, 255).astype(np.uint8)


def linear_taps(n_in, n_out):
    """(s, f fp32, c0, c1) of every output index: the bilinear rule with the coefficients of area mode"""
    inv, scale = scales(n_in, n_out)
    s = np.zeros(n_out, dtype=np.int64)
    f = np.zeros(n_out, dtype=F32)
    for d in range(n_out):
        sd = math.floor(d * scale)
        fd = F32((d + 1) - (sd + 1) * inv)
        fd = F32(0.0) if fd <= 0 else F32(fd - np.floor(fd))
        if sd < 0:
            sd, fd = 0, F32(0.0)
        if sd >= n_in - 1:
            sd, fd = n_in - 1, F32(0.0)
        s[d], f[d] = sd, fd
    c0 = np.rint((F32(1.0) - f) * F32(2048.0)).astype(np.int64)
    c1 = np.rint(f * F32(2048.0)).astype(np.int64)
    return s, f, c0, c1


def _linear(u8, h, w):
    """the fixed-point byte resize: rows S[s] * c0 + S[s + 1] * c1 in int32, then (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2"""
    H, W, _ = u8.shape
    S = u8.astype(np.int64)
    sx, _, ax, bx = linear_taps(W, w)
    sy, _, ay, by = linear_taps(H, h)
    rows = S[:, sx, :] * ax[None, :, None] + S[:, np.minimum(sx + 1, W - 1), :] * bx[None, :, None]
    r0, r1 = rows[sy], rows[np.minimum(sy + 1, H - 1)]
    out = (((ay[:, None, None] * (r0 >> 4)) >> 16) + ((by[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def resize_area(u8, new_w, new_h):
    """cv2.resize(u8, (new_w, new_h), interpolation=cv2.INTER_AREA) of one [H, W, 3] byte image"""
    u8 = np.asarray(u8)
    H, W, _ = u8.shape
    mode = mode_of(H, W, new_h, new_w)
    if mode == COPY:
        return u8.copy()
    if mode == LINEAR:
        return _linear(u8, new_h, new_w)
    return _area_general(u8, new_h, new_w) if mode == GENERAL else _area_fast(u8, new_h, new_w)


def tile_geometry(W, H, cell_w, cell_h, band):
    """(new_w, new_h, x_off, y_off) of `_fit_frame_to_tile`"""
    content_h = max(16, int(cell_h) - int(band))
    scale = min(float(cell_w) / max(1, W), float(content_h) / max(1, H))
    new_w, new_h = max(1, int(round(W * scale))), max(1, int(round(H * scale)))
    return new_w, new_h, max(0, (int(cell_w) - new_w) // 2), int(band) + max(0, (content_h - new_h) // 2)


def choose_columns(n):
    return max(1, int(math.ceil(math.sqrt(max(1, int(n))))))


def grid_frames(batches, cell_w, cell_h, columns, band=0, overlays=None):
    """fp32 [max F, rows * cell_h, columns * cell_w, 3]: batches are [F, H, W, C] fp32 arrays; overlays[i] is [band, cell_w, 3] uint8 or None"""
    batches = [np.asarray(b, dtype=F32) for b in batches]
    batches = [b[None] if b.ndim == 3 else b for b in batches]
    frames = max(int(b.shape[0]) for b in batches)
    rows = int(math.ceil(len(batches) / columns))
    out = np.zeros((frames, rows * cell_h, columns * cell_w, 3), dtype=np.uint8)
    for i, b in enumerate(batches):
        new_w, new_h, x_off, y_off = tile_geometry(b.shape[2], b.shape[1], cell_w, cell_h, band)
        if y_off + new_h > cell_h or x_off + new_w > cell_w:
            raise ValueError("the resized frame does not fit the tile")
        y0, x0 = (i // columns) * cell_h, (i % columns) * cell_w
        done = {}
        for f in range(frames):
            src = min(f, int(b.shape[0]) - 1)
            if src not in done:
                done[src] = resize_area(quantise(b[src]), new_w, new_h)
            out[f, y0 + y_off:y0 + y_off + new_h, x0 + x_off:x0 + x_off + new_w] = done[src]
            if overlays is not None and overlays[i] is not None:
                out[f, y0:y0 + band, x0:x0 + cell_w] = overlays[i]
    return out.astype(F32) / F32(255.0)


def tile_floats(frame, tile_hw):
    """one source frame -> the [h, w, 3] fp32 tile the kernel writes (bytes / 255); a uint8 frame is B,G,R"""
    frame = np.asarray(frame)
    u8 = frame[..., ::-1] if frame.dtype == np.uint8 else quantise(frame)
    return resize_area(u8, tile_hw[1], tile_hw[0]).astype(F32) / F32(255.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 filters
# ---------------------------------------------------------------------------------------------------------------------------------------
def _overlap(n_in, n_out):
    m = np.zeros((n_out, n_in))
    scale = n_in / n_out
    for i in range(n_out):
        a, b = i * scale, (i + 1) * scale
        for s in range(int(math.floor(a)), min(n_in, int(math.ceil(b)))):
            m[i, s] = (min(b, s + 1) - max(a, s)) / scale
    return m


def area_yardstick64(u8, h, w, ties="even"):
    """the exact area average in float64, rounded once (ties="up": the rule (a + b + c + d + 2) >> 2 applies to the quarters it meets)"""
    H, W, _ = u8.shape
    o = np.einsum("ih,hwc->iwc", _overlap(H, h), u8.astype(np.float64))
    o = np.einsum("jw,iwc->ijc", _overlap(W, w), o)
    return np.clip(np.floor(o + 0.5) if ties == "up" else np.rint(o), 0, 255).astype(np.uint8)


def linear_yardstick64(u8, h, w):
    """bilinear in float64 at the same (s, f)"""
    H, W, _ = u8.shape
    S = u8.astype(np.float64)
    sx, fx, _, _ = linear_taps(W, w)
    sy, fy, _, _ = linear_taps(H, h)
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)
    rows = S[:, sx, :] * (1.0 - fx)[None, :, None] + S[:, np.minimum(sx + 1, W - 1), :] * fx[None, :, None]
    out = rows[sy] * (1.0 - fy)[:, None, None] + rows[np.minimum(sy + 1, H - 1)] * fy[:, None, None]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def yardstick64(u8, h, w):
    H, W, _ = u8.shape
    mode = mode_of(H, W, h, w)
    if mode == COPY:
        return u8.copy()
    return linear_yardstick64(u8, h, w) if mode == LINEAR else area_yardstick64(u8, h, w, ties="up" if mode == FAST_2X2 else "even")


def differences(got, want):
    """(largest difference in levels, share of differing values)"""
    d = np.abs(np.asarray(got, dtype=np.int16) - np.asarray(want, dtype=np.int16))
    return int(d.max()) if d.size else 0, float((d != 0).mean()) if d.size else 0.0


def measure_shares():
    worst = {"area": 0.0, "linear": 0.0}
    for (H, W), (h, w), mode in GEOMETRIES:
        for kind in ("uniform", "smooth"):
            u8 = quantise(FRAME_KINDS[kind]((1, H, W, 3), 7)[0])
            levels, share = differences(resize_area(u8, w, h), yardstick64(u8, h, w))
            assert levels <= YARDSTICK_MAX_LEVELS
            key = "linear" if mode == LINEAR else "area"
            worst[key] = max(worst[key], share)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def special_frames(shape, seed):
    """NaN, +-Inf, -0.0, out-of-range values and k / 255 with its two neighbours (the truncation steps there)"""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    k = rng.integers(0, 256, shape).astype(F32) / F32(255.0)
    pick = rng.integers(0, 10, shape)
    x = np.where(pick == 0, np.nextafter(k, F32(2.0)), np.where(pick == 1, np.nextafter(k, F32(-1.0)), k)).astype(F32)
    for value, which in ((np.nan, 2), (np.inf, 3), (-np.inf, 4), (-0.0, 5), (-0.37, 6), (1.6, 7)):
        x = np.where(pick == which, F32(value), x).astype(F32)
    return x


FRAME_KINDS = {"uniform": uniform_frames, "smooth": smooth_frames, "special": special_frames}


def bytes_frames(shape, seed):
    return np.random.Generator(np.random.PCG64(int(seed))).integers(0, 256, shape, dtype=np.uint8)


def pattern_label(text, cell_w, cell_h, band):
    """a deterministic stand-in for cv2.putText, confined to the band: [cell_h, cell_w, 3] uint8"""
    canvas = np.zeros((int(cell_h), int(cell_w), 3), dtype=np.uint8)
    seed = sum((i + 1) * ord(ch) for i, ch in enumerate(str(text))) % 251
    yy, xx = np.mgrid[0:int(band), 0:int(cell_w)]
    for c in range(3):
        canvas[:int(band), :, c] = ((xx * 7 + yy * 13 + seed + 29 * c) % 256).astype(np.uint8)
    return canvas


# ---------------------------------------------------------------------------------------------------------------------------------------
# the header on the host
# ---------------------------------------------------------------------------------------------------------------------------------------
HOST_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse"]


def host_source():
    return os.path.join(ROOT, "tests", "host_math", "grid_check.cpp")


def build_host_lib(directory):
    out = os.path.join(str(directory), "libgrid_check.so")
    subprocess.run(["g++", *HOST_FLAGS, "-fPIC", "-shared", "-I", os.path.join(PKG_DIR, "csrc"), host_source(), "-o", out], check=True)
    lib = C.CDLL(out)
    P = C.c_void_p
    lib.hm_grid_mode.argtypes = [C.c_int32] * 4
    lib.hm_grid_mode.restype = C.c_int32
    lib.hm_grid_taps.argtypes = [C.c_int32, C.c_int32, C.c_int32, P]
    lib.hm_grid_taps.restype = None
    lib.hm_grid_cps.argtypes = [C.c_int32] * 4
    lib.hm_grid_cps.restype = C.c_int32
    lib.hm_grid_quant.argtypes = [P, P, C.c_int64]
    lib.hm_grid_quant.restype = None
    lib.hm_grid_unit.argtypes = [P]
    lib.hm_grid_unit.restype = None
    lib.hm_grid_resize.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P]
    lib.hm_grid_resize.restype = None
    lib.hm_grid_scale_pairs.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.hm_grid_scale_pairs.restype = None
    return lib


def scale_pairs(lib, limit, threads=8):
    """(count, first pair) of hm_grid_scale_pairs over n_in = 1 .. limit, the n_in ranges spread over host threads"""
    from concurrent.futures import ThreadPoolExecutor
    edges = [int(round(limit * (k / threads) ** 0.5)) for k in range(threads + 1)]          # the work grows with n_in squared

    def part(k):
        n, a, b = C.c_int64(), C.c_int32(), C.c_int32()
        lib.hm_grid_scale_pairs(edges[k] + 1, edges[k + 1], C.byref(n), C.byref(a), C.byref(b))
        return n.value, (a.value, b.value)

    with ThreadPoolExecutor(max_workers=threads) as pool:
        parts = list(pool.map(part, range(threads)))
    return sum(n for n, _ in parts), next((pair for n, pair in parts if n), (0, 0))


def host_resize(lib, frame, h, w):
    """one [H, W, C] fp32 R,G,B or [H, W, 3] uint8 B,G,R frame through the host-compiled header: [h, w, 3] uint8 R,G,B"""
    x = np.ascontiguousarray(frame)
    out = np.empty((h, w, 3), dtype=np.uint8)
    lib.hm_grid_resize(x.ctypes.data, int(x.dtype == np.uint8), x.shape[0], x.shape[1], x.shape[2], h, w, out.ctypes.data)
    return out


def host_quant(lib, values):
    x = np.ascontiguousarray(values, dtype=F32)
    out = np.empty(x.shape, dtype=np.uint8)
    lib.hm_grid_quant(x.ctypes.data, out.ctypes.data, x.size)
    return out


def host_cells(lib, n_in, n_out, mode):
    cells = np.zeros(n_out, dtype=CELL)
    lib.hm_grid_taps(n_in, n_out, mode, cells.ctypes.data)
    return cells


def golden_paths():
    return os.path.join(GOLDEN, "video_grid.json"), os.path.join(GOLDEN, "video_grid.npz")


def surface_path():
    return os.path.join(GOLDEN, "video_grid_surface.json")


def cv2_fixture_path():
    return os.path.join(GOLDEN, "video_grid_cv2.npz")


def cv2_pin_inputs():
    """the byte images of the cv2 pin and their target sizes: every geometry of the sweep (all five rules, and 953 -> 413, where the two
    formations of the scale part) -- what tools/make_golden_grid.py --cv2 records and test_grid_equals_cv2 compares"""
    out = []
    for i, ((H, W), (h, w), _) in enumerate(GEOMETRIES):
        out.append((f"g{i}_{H}x{W}_to_{h}x{w}", quantise(uniform_frames((1, H, W, 3), 31)[0]), (h, w)))
    return out


def golden_inputs(case):
    """the seeded inputs of one golden case: a list of fp32 arrays ([F, H, W, C] or [H, W, C])"""
    out = []
    for j, (shape, kind) in enumerate(case["inputs"]):
        shape = tuple(shape)
        full = shape if len(shape) == 4 else (1,) + shape
        x = FRAME_KINDS[kind](full, case["seed"] + 17 * j).astype(F32)
        out.append(x if len(shape) == 4 else x[0])
    return out

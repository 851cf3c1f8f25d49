"""Shared by tests/test_facefix_builder_host.py, tests/test_gpu_facefix_builder.py and tools/make_golden_facefix_builder.py.

The pixels of the AI Video Builder's Face Fix restated in numpy from the text of the specification, independently of
csrc/vrg_facefix_math.hpp, which must give the same masks bit for bit and the same bytes on the host (tests/host_math/facefix_check.cpp)
and on the GPU:

``mask_geometry`` / ``ellipse_spans``  the filled cv2.ellipse as one inclusive span per row (OpenCV 4.x's ellipse2Poly and FillConvexPoly
                                       in Python integers; no cv2 is at hand, so equality with cv2 itself is not pinned here);
``gauss_coeffs`` / ``blur``            the separable fp32 blur, BORDER_REFLECT_101 repeated, taps in index order;
``soft_ellipse_mask``                  the two together, clipped;
``yardstick_mask``                     the same blur with double coefficients and double sums: what the fp32 mask is measured against;
``color_match`` / ``blend``            the byte-domain mean shift (exact integer means, rounded once) and the fp32 blend;
``composite``                          a whole frame, with ``lanczos_support.restated`` as the resize.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import lanczos_support as LS
from conftest import GOLDEN, PKG_DIR, ROOT

f32 = np.float32
FIXTURE_JSON = os.path.join(GOLDEN, "facefix_builder.json")
FIXTURE_NPZ = os.path.join(GOLDEN, "facefix_builder.npz")
CV2_FIXTURE = os.path.join(GOLDEN, "facefix_builder_cv2.npz")
MASK_BOUND_FACTOR = 4.0                  # the tests allow 4 x the recorded gap (the factor of tools/make_golden_cut.py)

# ---- the cases of the GPU tests and of the fixture (inputs by recipe: kind, shape, seed) --------------------------------------------------
FRAMES_SHAPE = (5, 90, 160, 3)
FRAMES_SEED = 4101
# crops: per output size, one box or None per frame as (left, top, right, bottom)
CROP_SIZES = (64, 33)
CROP_BOXES = {
    "interior_edges": [(61, 20, 98, 57), (0, 0, 50, 50), None, (110, 40, 160, 90), (35, 0, 125, 90)],
    "copy_and_down": {64: [(10, 5, 74, 69), (70, 0, 160, 90), (96, 26, 160, 90), None, (0, 13, 77, 90)],
                      33: [(10, 5, 43, 38), (70, 0, 160, 90), (127, 57, 160, 90), None, (0, 13, 77, 90)]},
}
# composites: key -> enhanced shape (h, w), enhanced kind, boxes, strengths, feather, color_match
COMPOSITE_CASES = {
    "f18_cm065_64": ((64, 64), "random", [(30, 20, 67, 61), (100, 50, 120, 73), None, (96, 26, 160, 90), (3, 4, 40, 45)],
                     [1.0, 0.65, 1.0, 0.3, 0.65], 18, 0.65),
    "f0_cm0_48x40": ((48, 40), "random", [(30, 20, 67, 61), (100, 50, 105, 55), (7, 9, 8, 16), (96, 26, 160, 90), (3, 4, 40, 45)],
                     [1.0, 0.65, 1.0, 0.3, 0.0], 0, 0.0),
    "f1_cm1_bright_48x40": ((48, 40), "bright", [(30, 20, 67, 61), (100, 50, 105, 55), (7, 9, 8, 16), (96, 26, 160, 90), (30, 20, 67, 61)],
                            [1.0, 0.65, 1.0, 0.3, 0.65], 1, 1.0),
    "f1_cm1_dark_64": ((64, 64), "dark", [(30, 20, 67, 61), None, (7, 9, 8, 16), (96, 26, 160, 90), (3, 4, 40, 45)],
                       [1.0, 0.65, 1.0, 0.3, 0.65], 1, 1.0),
    "f256_64": ((64, 64), "random", [(40, 10, 104, 74), None, None, (96, 26, 160, 90), None], [1.0, 0.0, 0.0, 0.65, 0.0], 256, 0.65),
    "f18_small_48x40": ((48, 40), "random", [(100, 50, 120, 73), (100, 50, 105, 55), (7, 9, 8, 16), (140, 67, 160, 90), None],
                        [1.0, 1.0, 0.65, 0.3, 1.0], 18, 0.65),
}


def make_frames(kind, shape, seed):
    """byte frames by recipe: `random` uniform bytes, `smooth` waves, `bright` 200..255 with one value in seven 0..30 (far brighter than
    a smooth target: the shift is large and negative, the low values clip at 0), `dark` 0..40 with one in seven 225..255 (clip at 255)"""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    if kind == "random":
        return rng.integers(0, 256, size=tuple(shape), dtype=np.uint8)
    if kind in ("bright", "dark"):
        main = rng.integers(200, 256, size=tuple(shape), dtype=np.uint8) if kind == "bright" else rng.integers(0, 41, size=tuple(shape), dtype=np.uint8)
        rare = rng.integers(0, 31, size=tuple(shape), dtype=np.uint8) if kind == "bright" else rng.integers(225, 256, size=tuple(shape), dtype=np.uint8)
        return np.where(rng.integers(0, 7, size=tuple(shape)) == 0, rare, main).astype(np.uint8)
    if kind == "smooth":
        return LS.smooth_frames(tuple(shape), seed)
    raise ValueError(kind)


def case_inputs(key):
    """(originals, enhanced [one per box in order], boxes, strengths, feather, color_match) of a composite case"""
    (eh, ew), kind, boxes, strengths, feather, cm = COMPOSITE_CASES[key]
    originals = make_frames("smooth", FRAMES_SHAPE, FRAMES_SEED)
    n = sum(b is not None for b in boxes)
    enhanced = make_frames(kind, (n, eh, ew, 3), 5000 + sum(map(ord, key)))
    return originals, enhanced, boxes, strengths, feather, cm


# ---- mask ---------------------------------------------------------------------------------------------------------------------------------
def mask_geometry(width, height):
    """(centre, axes) of _soft_ellipse_mask"""
    inset = max(2, int(round(min(width, height) * 0.035)))
    return (width // 2, height // 2), (max(1, width // 2 - inset), max(1, height // 2 - inset))


def gauss_taps(feather):
    return max(3, 4 * int(feather) + 1)


def gauss_coeffs(n, sigma, dtype=np.float32):
    t = [math.exp(-((i - (n - 1) / 2.0) ** 2) / (2.0 * sigma * sigma)) for i in range(n)]
    total = 0.0
    for v in t:
        total += v
    return np.array([v / total for v in t], dtype=np.float64).astype(dtype)


_ONE = 1 << 16
_HALF = 1 << 15


def _sine(degree):
    return float(f32(round(math.sin(math.radians(degree)) * 1e7) / 1e7))


def _polygon(centre, axes):
    cx, cy = centre[0] << 16, centre[1] << 16
    aw, ah = abs(axes[0]) << 16, abs(axes[1]) << 16
    delta = (max(aw, ah) + _HALF) >> 16
    delta = 90 if delta < 3 else 30 if delta < 10 else 18 if delta < 15 else 5
    cos_r, sin_r = _sine(450), _sine(0)
    pts = []
    for i in range(0, 360 + delta, delta):
        a = min(i, 360)
        x, y = aw * _sine(450 - a), ah * _sine(a)
        p = (int(np.rint(cx + x * cos_r - y * sin_r)), int(np.rint(cy + x * sin_r + y * cos_r)))
        if not pts or pts[-1] != p:
            pts.append(p)
    if len(pts) == 1:
        pts = [(cx, cy), (cx, cy)]
    return pts


def _clip(width, height, p1, p2):
    x1, y1 = p1
    x2, y2 = p2
    right, bottom = width - 1, height - 1

    def code(x, y):
        return (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8

    c1, c2 = code(x1, y1), code(x2, y2)
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1, c1 = a, 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2, c2 = a, 0
    return (c1 | c2) == 0, (x1, y1), (x2, y2)


def _idiv(a, b):
    """C's integer division (towards zero)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def ellipse_spans(width, height, centre, axes):
    """[height, 2] int32: inclusive x0, x1 of every row of cv2.ellipse(img, centre, axes, 0, 0, 360, 1, -1); x0 > x1 = empty"""
    rows = {}

    def put(x, y):
        if 0 <= x < width and 0 <= y < height:
            lo, hi = rows.get(y, (x, x))
            rows[y] = (min(lo, x), max(hi, x))

    def outline(p1, p2):
        ok, p1, p2 = _clip(width << 16, height << 16, p1, p2)
        if not ok:
            return
        dx, dy = p2[0] - p1[0], p2[1] - p1[1]
        ax, ay = abs(dx), abs(dy)
        if ax > ay:
            if dx < 0:
                p1, p2, dy = p2, p1, -dy
            x, y = p1[0] + _HALF, p1[1] + _HALF
            step = _idiv(dy << 16, ax | 1)
            count = (p2[0] - p1[0]) >> 16
            put((p2[0] + _HALF) >> 16, (p2[1] + _HALF) >> 16)
            x >>= 16
            for _ in range(count + 1):
                put(x, y >> 16)
                x += 1
                y += step
        else:
            if dy < 0:
                p1, p2, dx = p2, p1, -dx
            x, y = p1[0] + _HALF, p1[1] + _HALF
            step = _idiv(dx << 16, ay | 1)
            count = (p2[1] - p1[1]) >> 16
            put((p2[0] + _HALF) >> 16, (p2[1] + _HALF) >> 16)
            y >>= 16
            for _ in range(count + 1):
                put(x >> 16, y)
                x += step
                y += 1

    v = _polygon(centre, axes)
    n = len(v)
    prev = v[-1]
    for p in v:
        outline(prev, p)
        prev = p
    xmin, xmax = (min(p[0] for p in v) + _HALF) >> 16, (max(p[0] for p in v) + _HALF) >> 16
    ys = [p[1] for p in v]
    imin = ys.index(min(ys))
    ymin, ymax = (min(ys) + _HALF) >> 16, (max(ys) + _HALF) >> 16
    if not (n < 3 or xmax < 0 or ymax < 0 or xmin >= width or ymin >= height):
        ymax = min(ymax, height - 1)
        edges = n
        edge = [dict(idx=imin, di=1, x=-_ONE, dx=0, ye=ymin), dict(idx=imin, di=n - 1, x=-_ONE, dx=0, ye=ymin)]
        y = ymin
        while True:
            for e in edge:
                if y >= e["ye"]:
                    idx0 = e["idx"]
                    idx = (idx0 + e["di"]) % n
                    while True:
                        edges -= 1
                        if edges < 0:
                            break
                        ty = (v[idx][1] + _HALF) >> 16
                        if ty > y:
                            xs, xe = v[idx0][0], v[idx][0]
                            e.update(ye=ty, dx=_idiv((xe - xs) * 2 + (ty - y), 2 * (ty - y)), x=xs, idx=idx)
                            break
                        idx0 = idx
                        idx = (idx + e["di"]) % n
            if edges < 0:
                break
            if y >= 0:
                lo, hi = sorted((edge[0]["x"], edge[1]["x"]))
                x1, x2 = (lo + _HALF) >> 16, (hi + _HALF) >> 16
                if x2 >= 0 and x1 < width:
                    x1, x2 = max(x1, 0), min(x2, width - 1)
                    if x1 <= x2:
                        put(x1, y)
                        put(x2, y)
            for e in edge:
                e["x"] += e["dx"]
            y += 1
            if y > ymax:
                break
    # symmetric under the reflections the centre allows: every filled pixel's mirror image about the centre column and about the centre
    # row is filled too, where it lies inside the plane (the outline alone can miss it by one pixel at the end of a row)
    plane = np.zeros((height, width), dtype=bool)
    for y, (lo, hi) in rows.items():
        plane[y, lo:hi + 1] = True
    ys, xs = np.nonzero(plane)
    mx = 2 * centre[0] - xs
    keep = (mx >= 0) & (mx < width)
    plane[ys[keep], mx[keep]] = True
    ys, xs = np.nonzero(plane)
    my = 2 * centre[1] - ys
    keep = (my >= 0) & (my < height)
    plane[my[keep], xs[keep]] = True
    out = np.empty((height, 2), dtype=np.int32)
    out[:, 0], out[:, 1] = 0, -1
    for y in range(height):
        xs = np.nonzero(plane[y])[0]
        if xs.size:
            assert xs[-1] - xs[0] + 1 == xs.size                              # one span per row
            out[y] = (xs[0], xs[-1])
    return out


def spans_to_plane(spans, width, dtype=np.float32):
    x = np.arange(width)[None, :]
    return ((x >= spans[:, :1]) & (x <= spans[:, 1:])).astype(dtype)


def reflect101(index, n):
    """BORDER_REFLECT_101, repeated until inside"""
    i = np.asarray(index, dtype=np.int64).copy()
    if n == 1:
        return np.zeros_like(i)
    while True:
        low, high = i < 0, i >= n
        if not (low.any() or high.any()):
            return i
        i = np.where(low, -i, i)
        i = np.where(i >= n, 2 * (n - 1) - i, i)


def blur(plane, coeffs):
    """horizontal then vertical, sums in the dtype of `coeffs` (float32: the specification; float64: the yardstick), taps in index order;
    `plane` is [h, w] or a stack [..., h, w] of planes of one size"""
    dt = coeffs.dtype.type
    src = np.asarray(plane, dtype=dt)
    h, w = src.shape[-2:]
    n = len(coeffs)
    r = (n - 1) // 2
    hor = np.zeros(src.shape, dtype=dt)
    for i in range(n):
        hor = hor + coeffs[i] * src[..., reflect101(np.arange(w) + i - r, w)]
    ver = np.zeros(src.shape, dtype=dt)
    for j in range(n):
        ver = ver + coeffs[j] * hor[..., reflect101(np.arange(h) + j - r, h), :]
    return ver


def _mask(width, height, feather, dtype):
    centre, axes = mask_geometry(width, height)
    plane = spans_to_plane(ellipse_spans(width, height, centre, axes), width, dtype)
    feather = max(0, int(feather))
    if feather > 0:
        plane = blur(plane, gauss_coeffs(gauss_taps(feather), max(0.1, feather), dtype))
    return plane.clip(0.0, 1.0)


def soft_ellipse_mask(width, height, feather):
    return _mask(width, height, feather, np.float32)


def yardstick_mask(width, height, feather):
    return _mask(width, height, feather, np.float64)


# ---- bytes --------------------------------------------------------------------------------------------------------------------------------
def color_match(face, target, alpha, strength):
    """(bytes, sums): the mean shift with exact integer means rounded once; sums = count, face B G R, target B G R"""
    strength = max(0.0, min(1.0, float(strength)))
    selected = alpha > f32(0.35)
    count = int(selected.sum())
    sums = [count] + [int(face[..., c][selected].astype(np.int64).sum()) for c in range(3)] + \
        [int(target[..., c][selected].astype(np.int64).sum()) for c in range(3)]
    if strength <= 0 or count < 16:
        return face, sums
    smean = np.array([f32(sums[1 + c] / count) for c in range(3)], dtype=f32)
    tmean = np.array([f32(sums[4 + c] / count) for c in range(3)], dtype=f32)
    shift = ((tmean - smean) * f32(strength)).astype(f32)
    return np.clip(face.astype(f32) + shift, 0, 255).astype(np.uint8), sums


def blend(target, face, base_alpha, composite_strength):
    a = (base_alpha.astype(f32) * f32(composite_strength))[:, :, None]
    v = target.astype(f32) * (f32(1.0) - a) + face.astype(f32) * a
    return np.clip(v, 0, 255).astype(np.uint8)


def composite(originals, enhanced, boxes, strengths, feather, cm):
    """the whole route on a batch: enhanced holds one frame per box, in order"""
    out = originals.copy()
    k = 0
    masks = {}
    for f, box in enumerate(boxes):
        if box is None:
            continue
        e = enhanced[k]
        k += 1
        s = max(0.0, min(1.0, float(strengths[f])))
        if s <= 0.0:
            continue
        left, top, right, bottom = box
        w, h = right - left, bottom - top
        if (w, h) not in masks:
            masks[(w, h)] = soft_ellipse_mask(w, h, feather)
        resized = np.asarray(LS.restated(e[None], w, h))[0]
        target = originals[f, top:bottom, left:right]
        face, _ = color_match(resized, target, masks[(w, h)], cm)
        out[f, top:bottom, left:right] = blend(target, face, masks[(w, h)], s)
    return out


def crops(frames, boxes, size):
    """[n, size, size, 3]: the boxes that are not None, each resized as a view of its own"""
    out = []
    for f, box in enumerate(boxes):
        if box is None:
            continue
        left, top, right, bottom = box
        out.append(np.asarray(LS.restated(np.ascontiguousarray(frames[f:f + 1, top:bottom, left:right]), size, size))[0])
    return np.stack(out) if out else np.zeros((0, size, size, 3), dtype=np.uint8)


# ---- the byte mover: the geometry sweep of far_face_support.MOVER_CASES for k_ff_composite ------------------------------------------------
MOVER_ENHANCED = (9, 7)                  # (h, w) of every repaired frame of the sweep: unlike every box, so each is resized
MOVER_SETTINGS = ((0, 0.0), (0, 0.65), (1, 0.0), (1, 0.65))                  # (feather, color_match)


def mover_inputs(name):
    """-> (originals, enhanced [one per box], boxes, strengths) of a case of the sweep: strengths 1.0 and 0.65 in turn, and 0.0 (the frame
    must come back untouched although it has a box) on the last frame of the first case"""
    import far_face_support as S
    F, H, W, boxes = S.MOVER_CASES[name]
    originals = S.mover_originals(name)
    n = sum(b is not None for b in boxes)
    enhanced = make_frames("random", (n,) + MOVER_ENHANCED + (3,), 8500 + sorted(S.MOVER_CASES).index(name))
    strengths = [(1.0, 0.65)[f % 2] for f in range(F)]
    if name == "a_1x1":
        strengths[-1] = 0.0
    return originals, enhanced, boxes, strengths


# ---- the header on the host ---------------------------------------------------------------------------------------------------------------
F32P = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
I64P = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")


def build_host_lib(directory):
    out = os.path.join(str(directory), "libfacefix_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "facefix_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_ff_spans.argtypes = [C.c_int32, C.c_int32, I32P]
    lib.hm_ff_coeffs.argtypes = [C.c_int32, F32P]
    lib.hm_ff_mask.argtypes = [C.c_int32, C.c_int32, C.c_int32, F32P]
    lib.hm_ff_composite.argtypes = [LS.U8P, LS.U8P, F32P, C.c_int32, C.c_int32, C.c_float, C.c_float, LS.U8P, I64P]
    for fn in (lib.hm_ff_spans, lib.hm_ff_coeffs, lib.hm_ff_mask, lib.hm_ff_composite):
        fn.restype = None
    return lib


def host_spans(lib, width, height):
    out = np.zeros((height, 2), dtype=np.int32)
    lib.hm_ff_spans(width, height, out)
    return out


def host_mask(lib, width, height, feather):
    out = np.zeros((height, width), dtype=np.float32)
    lib.hm_ff_mask(width, height, int(feather), out)
    return out


def host_composite(lib, target, face, mask, cm, strength):
    h, w, _ = target.shape
    out = np.zeros((h, w, 3), dtype=np.uint8)
    sums = np.zeros(7, dtype=np.int64)
    lib.hm_ff_composite(np.ascontiguousarray(target), np.ascontiguousarray(face), np.ascontiguousarray(mask, dtype=np.float32), h, w,
                        float(cm), float(strength), out, sums)
    return out, [int(v) for v in sums]

"""Test scaffolding for the far-face repair composite (comfyui-vrgamedevgirl_amd/far_face_repair.py, csrc/vrg_farface.hip): an independent
numpy restatement of what Pillow and numpy do in ``composite`` of the reference's scripts/far_face_repair_backend.py -- Image.resize(...,
LANCZOS) on RGB / L bytes, ImageFilter.GaussianBlur on L, Image.paste under an L mask, and the sequential fp32 means of
color_match_repaired -- plus the seeded inputs of tests/golden/far_face.{json,npz} and the ctypes face of tests/host_math/farface_check.cpp.
Nothing here imports the package; the ellipse outline alone is taken from Pillow (the rasteriser is not restated anywhere).
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from conftest import GOLDEN, PKG_DIR, ROOT

FIXTURE_JSON = os.path.join(GOLDEN, "far_face.json")
FIXTURE_NPZ = os.path.join(GOLDEN, "far_face.npz")

PRECISION_BITS = 22
COLOR_MATCH = 0.65

# (in_w, in_h) -> (out_w, out_h): the smallest sizes where each rule of the resize bites
RESIZE_CASES = (((33, 47), (90, 71)), ((128, 128), (37, 41)), ((64, 50), (64, 20)), ((17, 9), (200, 3)), ((1, 1), (5, 5)), ((300, 300), (7, 7)))
MASK_SIZES = ((90, 71), (37, 41), (12, 9), (1, 7), (33, 33), (300, 280))
FEATHERS = (0, 1, 2, 18, 40, 300)


# ------------------------------------------------------------------------------------------------
# Image.resize(size, LANCZOS)
# ------------------------------------------------------------------------------------------------
def _lanczos(t):
    if not -3.0 <= t < 3.0:
        return 0.0
    if t == 0.0:
        return 1.0
    a, b = t * math.pi, t / 3.0 * math.pi
    return (math.sin(a) / a) * (math.sin(b) / b if b != 0.0 else 1.0)


def lanczos_ksize(n_in, n_out):
    return int(math.ceil(3.0 * max(n_in / n_out, 1.0))) * 2 + 1


def lanczos_table(n_in, n_out):
    """-> (bounds [n_out, 2] int32: first source index and tap count, weights [n_out, ksize] int32: 22-bit fixed point)"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 3.0 * fs, 1.0 / fs
    ksize = lanczos_ksize(n_in, n_out)
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    weights = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = min(int(c + support + 0.5), n_in) - xmin
        w = [_lanczos((x + xmin - c + 0.5) * ss) for x in range(xmax)]
        total = 0.0
        for v in w:
            total += v
        for x, v in enumerate(w):
            if total != 0.0:
                v = v / total
            f = v * (1 << PRECISION_BITS)
            weights[xx, x] = int(f - 0.5) if v < 0 else int(f + 0.5)
        bounds[xx] = (xmin, xmax)
    return bounds, weights


def _pass(img, n_out, axis):
    """one byte pass of the resize along `axis` of an [h, w, c] uint8 array"""
    img = np.moveaxis(img, axis, 0)
    bounds, weights = lanczos_table(img.shape[0], n_out)
    out = np.empty((n_out,) + img.shape[1:], dtype=np.uint8)
    for xx in range(n_out):
        x0, n = bounds[xx]
        acc = np.tensordot(weights[xx, :n].astype(np.int64), img[x0:x0 + n].astype(np.int64), axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, size):
    """``Image.fromarray(img).resize(size, LANCZOS)`` for [h, w, 3] (RGB) or [h, w] (L) uint8; size = (width, height)"""
    img = np.asarray(img)
    flat = img.ndim == 2
    x = img[:, :, None] if flat else img
    ow, oh = size
    if x.shape[1] != ow:
        x = _pass(x, ow, 1)                                                  # the horizontal pass first, rounded to bytes
    if x.shape[0] != oh:
        x = _pass(x, oh, 0)
    x = np.ascontiguousarray(x)
    return x[:, :, 0] if flat else x


# ------------------------------------------------------------------------------------------------
# ImageFilter.GaussianBlur(radius) on L: three box passes per direction, every one rounded to bytes
# ------------------------------------------------------------------------------------------------
def box_parameters(sigma):
    """(r, ww, fw) of one box pass: Pillow computes the box radius and the weight of a full tap in C `float`"""
    f = np.float32
    s2 = f(f(sigma) * f(sigma)) / f(3)
    big = f(np.sqrt(np.float64(12.0) * np.float64(s2) + 1.0))
    l = f(np.floor((np.float64(big) - 1.0) / 2.0))
    a = f(f(f(2) * l + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * s2)))
    a = f(a / f(f(6) * f(s2 - f(f(l + f(1)) * f(l + f(1))))))
    radius = f(l + a)
    r = int(radius)
    ww = int(f(f(1 << 24) / f(radius * f(2) + f(1))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def _box_lines(x, r, ww, fw):
    """one box pass along the last axis of a uint8 array, border replicated"""
    n = x.shape[-1]
    idx = np.arange(n)
    v = x.astype(np.int64)
    acc = np.zeros_like(v)
    for i in range(-r, r + 1):
        acc += v[..., np.clip(idx + i, 0, n - 1)]
    far = v[..., np.clip(idx - r - 1, 0, n - 1)] + v[..., np.clip(idx + r + 1, 0, n - 1)]
    return (((ww * acc + fw * far) & 0xffffffff) + (1 << 23) >> 24).astype(np.uint8)


def _box_lines_prefix(x, r, ww, fw):
    """the same from a prefix sum (what the kernel does): much faster for large radii"""
    n = x.shape[-1]
    idx = np.arange(n)
    v = x.astype(np.int64)
    p = np.concatenate([np.zeros(v.shape[:-1] + (1,), dtype=np.int64), np.cumsum(v, axis=-1)], axis=-1)
    lo, hi = np.clip(idx - r, 0, n), np.clip(idx + r + 1, 0, n)
    acc = p[..., hi] - p[..., lo] + v[..., :1] * np.maximum(0, r - idx) + v[..., -1:] * np.maximum(0, idx + r - (n - 1))
    far = v[..., np.clip(idx - r - 1, 0, n - 1)] + v[..., np.clip(idx + r + 1, 0, n - 1)]
    return (((ww * acc + fw * far) & 0xffffffff) + (1 << 23) >> 24).astype(np.uint8)


def gaussian_blur(mask, sigma, lines=_box_lines_prefix):
    r, ww, fw = box_parameters(sigma)
    x = np.asarray(mask, dtype=np.uint8)
    for _ in range(3):
        x = lines(x, r, ww, fw)
    x = np.ascontiguousarray(x.T)
    for _ in range(3):
        x = lines(x, r, ww, fw)
    return np.ascontiguousarray(x.T)


def ellipse_spans(width, height, shrink=0.12):
    """[height, 2] int32 (first and last set column; first > last: an empty row) of the ellipse soft_face_mask draws, from Pillow"""
    from PIL import Image, ImageDraw
    inset_x, inset_y = int(round(width * shrink)), int(round(height * shrink))
    mask = Image.new("L", (width, height), 0)
    ImageDraw.Draw(mask).ellipse((inset_x, inset_y, width - inset_x, height - inset_y), fill=255)
    plane = np.asarray(mask) != 0
    spans = np.zeros((height, 2), dtype=np.int32)
    for y in range(height):
        cols = np.flatnonzero(plane[y])
        spans[y] = (cols[0], cols[-1]) if cols.size else (1, 0)
        assert cols.size == 0 or cols.size == cols[-1] - cols[0] + 1, "a row of the ellipse is not one run"
    return spans


def spans_to_mask(spans, width):
    x = np.arange(width)[None, :]
    return (((x >= spans[:, :1]) & (x <= spans[:, 1:])) * 255).astype(np.uint8)


def soft_face_mask(size, feather, shrink=0.12):
    width, height = size
    mask = spans_to_mask(ellipse_spans(width, height, shrink), width)
    return gaussian_blur(mask, float(feather)) if feather > 0 else mask


# ------------------------------------------------------------------------------------------------
# color_match_repaired and Image.paste
# ------------------------------------------------------------------------------------------------
def sequential_means(pixels_u8, mask_u8):
    """numpy's ``x[selected].mean(axis=0)`` of float32 rows: the fp32 sum in row-major order (adding 0.0 for an unselected pixel changes
    nothing), divided by the count in fp32 -> (count, [3] float32)"""
    sel = (np.asarray(mask_u8).reshape(-1) >= 64)
    count = int(sel.sum())
    v = (np.asarray(pixels_u8).reshape(-1, 3) * sel[:, None]).astype(np.float32)
    sums = np.add.accumulate(v, axis=0, dtype=np.float32)[-1] if len(v) else np.zeros(3, np.float32)
    return count, (sums / np.float32(max(count, 1))).astype(np.float32)


def exact_means(pixels_u8, mask_u8):
    sel = (np.asarray(mask_u8).reshape(-1) >= 64)
    count = int(sel.sum())
    sums = (np.asarray(pixels_u8).reshape(-1, 3).astype(np.int64) * sel[:, None]).sum(axis=0)
    return count, (sums.astype(np.float64) / max(count, 1)).astype(np.float32)


def color_match(original_u8, repaired_u8, mask_u8, means=sequential_means):
    """-> (adjusted bytes, count, original means, repaired means, shifts); fewer than 16 selected: the repaired bytes themselves"""
    count, om = means(original_u8, mask_u8)
    _, rm = means(repaired_u8, mask_u8)
    shift = ((om - rm).astype(np.float32) * np.float32(COLOR_MATCH)).astype(np.float32)
    if count < 16:
        return repaired_u8, count, om, rm, shift
    adjusted = np.clip(repaired_u8.astype(np.float32) + shift, 0, 255).astype(np.uint8)
    return adjusted, count, om, rm, shift


def paste(original_u8, repaired_u8, mask_u8):
    """``Image.paste(repaired, box, mask)`` on the box: ONE rounded division by 255 of the sum"""
    m = mask_u8.astype(np.int64)[:, :, None]
    t = original_u8.astype(np.int64) * (255 - m) + repaired_u8.astype(np.int64) * m + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def composite(originals, repaired, boxes, feather=18, color_match_on=False, masks=None, means=sequential_means):
    """``composite`` of the reference for a batch: originals [F, H, W, 3]; repaired / masks: one array per frame that has a box"""
    out = np.array(originals, copy=True)
    k = 0
    for f, box in enumerate(boxes):
        if box is None:
            continue
        left, top, right, bottom = box
        size = (right - left, bottom - top)
        rep = resize(repaired[k], size)
        mask = soft_face_mask(size, feather) if feather >= 0 else resize(masks[k], size)
        k += 1
        target = originals[f, top:bottom, left:right]
        if color_match_on:
            rep = color_match(target, rep, mask, means)[0]
        out[f, top:bottom, left:right] = paste(target, rep, mask)
    return out


# ------------------------------------------------------------------------------------------------
# seeded inputs (the fixture stores seeds, not inputs)
# ------------------------------------------------------------------------------------------------
def random_image(seed, h, w, c=3, lo=0, hi=256):
    rng = np.random.Generator(np.random.PCG64(seed))
    shape = (h, w, c) if c else (h, w)
    return rng.integers(lo, hi, size=shape, dtype=np.uint8)


def smooth_image(seed, h, w, c=3):
    """a smooth field plus noise: the kind of picture a crop is"""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for _ in range(max(c, 1)):
        a, b, p, q = rng.uniform(0.02, 0.2, 4)
        planes.append(127.5 + 90.0 * np.sin(a * xx + p * 9) * np.cos(b * yy + q * 7) + rng.normal(0, 12, (h, w)))
    img = np.clip(np.stack(planes, axis=-1), 0, 255).astype(np.uint8)
    return img if c else img[:, :, 0]


FRAME_H, FRAME_W = 96, 128
# 5 frames of 96 x 128: a corner, touching two edges, 1 x 1, the full frame, no box
COMPOSITE_BOXES = [(0, 0, 40, 33), (75, 50, 128, 96), (64, 31, 65, 32), (0, 0, 128, 96), None]
COMPOSITE_REPAIRED = [(64, 64), (37, 80), (9, 9), (64, 48)]                 # (w, h) of the repaired crops, all unlike their boxes
COMPOSITE_VARIANTS = [(18, False), (18, True), (0, False), (0, True), (-1, False), (-1, True)]


def composite_inputs():
    originals = np.stack([smooth_image(4100 + f, FRAME_H, FRAME_W) for f in range(len(COMPOSITE_BOXES))])
    repaired = [smooth_image(4200 + k, h, w) for k, (w, h) in enumerate(COMPOSITE_REPAIRED)]
    masks = []
    for k, (w, h) in enumerate(COMPOSITE_REPAIRED):                          # saved masks of the crop's size: a soft ellipse, perturbed
        m = soft_face_mask((w, h), 3).astype(np.int16) if min(w, h) > 1 else np.full((h, w), 200, np.int16)
        m = np.clip(m + random_image(4300 + k, h, w, 0, 0, 9).astype(np.int16) - 4, 0, 255).astype(np.uint8)
        masks.append(m)
    return originals, repaired, masks


def means_inputs(key):
    """-> (original crop, repaired crop, mask) of the named means case"""
    if key in ("sel15", "sel16"):
        n = 15 if key == "sel15" else 16
        mask = np.full(36, 63, np.uint8)
        mask[:n] = 64
        return random_image(5001, 6, 6), random_image(5002, 6, 6, 3, 0, 60), mask.reshape(6, 6)
    if key == "400_ge200":                                                    # above 2^24 in its first binade
        return random_image(5011, 400, 400, 3, 200, 256), random_image(5012, 400, 400, 3, 200, 256), np.full((400, 400), 255, np.uint8)
    if key == "560_random":
        return random_image(5021, 560, 560), random_image(5022, 560, 560), np.full((560, 560), 255, np.uint8)
    if key == "560_ge128":                                                    # crosses two binades: 2^24 and 2^25
        return random_image(5031, 560, 560, 3, 128, 256), random_image(5032, 560, 560, 3, 128, 256), random_image(5033, 560, 560, 0, 60, 256)
    raise KeyError(key)


MEANS_CASES = ("sel15", "sel16", "400_ge200", "560_random", "560_ge128")
LARGE_FRAME, LARGE_BOX, LARGE_REPAIRED = 576, (8, 8, 568, 568), 512


def large_inputs():
    return smooth_image(6001, LARGE_FRAME, LARGE_FRAME)[None], [smooth_image(6002, LARGE_REPAIRED, LARGE_REPAIRED)]


def bits(x):
    return [int(v) for v in np.asarray(x, dtype=np.float32).view(np.uint32)]


# ------------------------------------------------------------------------------------------------
# csrc/vrg_pil_math.hpp on the host
# ------------------------------------------------------------------------------------------------
U8P = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
U32P = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
I64P = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")


def build_host_lib(directory):
    out = os.path.join(str(directory), "libfarface_check.so")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host_math", "farface_check.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_pil_ksize.restype = C.c_int32
    lib.hm_pil_ksize.argtypes = [C.c_int32, C.c_int32]
    lib.hm_pil_table.argtypes = [C.c_int32, C.c_int32, I32P, I32P]
    lib.hm_pil_resize.argtypes = [U8P, C.c_int32, C.c_int32, C.c_int32, U8P, C.c_int32, C.c_int32]
    lib.hm_pil_box.argtypes = [C.c_float, I32P]
    lib.hm_pil_mask.argtypes = [I32P, C.c_int32, C.c_int32, C.c_int32, U8P]
    lib.hm_pil_means.argtypes = [U8P, U8P, U8P, C.c_int64, C.c_int32, U32P]
    lib.hm_pil_paste.argtypes = [U8P, U8P, U8P, C.c_int64, C.c_int32, U32P, U8P]
    lib.hm_byte_piece_hits.restype = C.c_int32
    lib.hm_byte_piece_hits.argtypes = [C.c_int32] * 6
    lib.hm_span_fits.restype = C.c_int32
    lib.hm_span_fits.argtypes = [C.c_int64] * 3
    lib.hm_launch_chunks.restype = C.c_int32
    lib.hm_launch_chunks.argtypes = [C.c_int64, C.c_int32, C.c_int32, I64P, C.c_int32, I32P]
    lib.hm_launch_chunks_aligned.restype = C.c_int32
    lib.hm_launch_chunks_aligned.argtypes = [C.c_int64, C.c_int64, I64P, C.c_int32, I32P]
    lib.hm_chunk_lcm.restype = C.c_int64
    lib.hm_chunk_lcm.argtypes = [C.c_int64, C.c_int64]
    return lib


def host_table(lib, n_in, n_out):
    k = lib.hm_pil_ksize(n_in, n_out)
    bounds, weights = np.zeros((n_out, 2), np.int32), np.zeros((n_out, k), np.int32)
    lib.hm_pil_table(n_in, n_out, bounds, weights)
    return bounds, weights


def host_resize(lib, img, size):
    img = np.ascontiguousarray(img)
    c = 1 if img.ndim == 2 else img.shape[2]
    out = np.zeros((size[1], size[0]) + (() if img.ndim == 2 else (c,)), np.uint8)
    lib.hm_pil_resize(img, img.shape[0], img.shape[1], c, out, size[1], size[0])
    return out


def host_box(lib, sigma):
    out = np.zeros(3, np.int32)
    lib.hm_pil_box(sigma, out)
    return tuple(int(v) for v in out.view(np.uint32))


def host_mask(lib, size, feather):
    w, h = size
    out = np.zeros((h, w), np.uint8)
    lib.hm_pil_mask(np.ascontiguousarray(ellipse_spans(w, h)), w, h, feather, out)
    return out


def host_means(lib, original, repaired, mask, parallel):
    """-> uint32[12]: count, original mean bits x3, repaired mean bits x3, shift bits x3, matched, 0"""
    out = np.zeros(12, np.uint32)
    lib.hm_pil_means(np.ascontiguousarray(original), np.ascontiguousarray(repaired), np.ascontiguousarray(mask), mask.size, int(parallel), out)
    return out


def host_paste(lib, original, repaired, mask, stats=None):
    out = np.zeros_like(original)
    st = np.zeros(12, np.uint32) if stats is None else np.ascontiguousarray(stats, dtype=np.uint32)
    lib.hm_pil_paste(np.ascontiguousarray(original), np.ascontiguousarray(repaired), np.ascontiguousarray(mask), mask.size,
                     0 if stats is None else 1, st, out)
    return out


# ------------------------------------------------------------------------------------------------
# the steered case: a box whose exact-mean shift and numpy-mean shift truncate differently
# ------------------------------------------------------------------------------------------------
STEERED_FRAME, STEERED_BOX = 416, (8, 8, 408, 408)


def steered_inputs(k):
    """416 x 416 frame of bytes >= 200 with a 400 x 400 box, a crop of the box's size and a saved mask of 255; `k` pixels of channel 0 of
    the box are moved by one level (the sign of k) -- the generator picks k so that an integer lies between the two routes' shifts"""
    frame = random_image(7001, STEERED_FRAME, STEERED_FRAME, 3, 200, 256)
    rep = random_image(7002, 400, 400, 3, 200, 256)
    left, top, right, bottom = STEERED_BOX
    plane = frame[top:bottom, left:right, 0].copy()
    flat = plane.reshape(-1)
    eligible = np.flatnonzero(flat < 255) if k > 0 else np.flatnonzero(flat > 200)
    if k:
        pick = eligible[np.linspace(0, len(eligible) - 1, abs(int(k))).astype(np.int64)]
        flat[pick] = (flat[pick].astype(np.int16) + (1 if k > 0 else -1)).astype(np.uint8)
    frame[top:bottom, left:right, 0] = plane
    return frame[None], [rep], [np.full((400, 400), 255, np.uint8)]


# ------------------------------------------------------------------------------------------------
# the byte movers (k_pil_paste of csrc/vrg_farface.hip, k_ff_composite of csrc/vrg_facefix.hip): one geometry sweep for both, and a model
# of how the kernels split the flat batch into 16-byte pieces.  The model restates the geometry; it calls no kernel.
# ------------------------------------------------------------------------------------------------
PIECE = 16
MOVER_OFFSETS = (0, 1, 4)                                                    # where the batch starts in its device buffer, in bytes


def _d_boxes(k):
    """case d: an interior 6 x 5 box per frame whose `left` is 4 k + f, so that the four cases take every value 0 .. 15"""
    return [(4 * k + f, 9 + 3 * f, 4 * k + f + 6, 14 + 3 * f) for f in range(4)]


# name -> (F, H, W, one (left, top, right, bottom) or None per frame)
MOVER_CASES = {
    # one 16-byte piece crosses five seams; the records alternate box / no box
    "a_1x1": (5, 1, 1, [(0, 0, 1, 1), None, (0, 0, 1, 1), None, (0, 0, 1, 1)]),
    # pitch 15 < 16: every piece spans two or three rows; 315 bytes leave a tail of 11
    "b_7x5": (3, 7, 5, [(0, 0, 5, 7), (4, 6, 5, 7), None]),
    # box edges against the frame edges: the four corners, a single column at x = 10, a single row at y = 8
    "c_corners": (3, 9, 11, [(7, 0, 11, 4), (0, 0, 4, 3), (0, 6, 3, 9)]),
    "c_lines": (3, 9, 11, [(8, 5, 11, 9), (10, 0, 11, 9), (0, 8, 11, 9)]),
    # 3663 bytes per frame, pitch 111: the box's first byte lands on every offset within a piece
    "d_left0": (4, 33, 37, _d_boxes(0)),
    "d_left4": (4, 33, 37, _d_boxes(1)),
    "d_left8": (4, 33, 37, _d_boxes(2)),
    "d_left12": (4, 33, 37, _d_boxes(3)),
    # 2115 pixels: more than one chunk of the means and no multiple of it, beside a box of width 1
    "d_47x45": (3, 64, 48, [(0, 10, 47, 55), (5, 3, 6, 43), None]),
    # the seam-free size of the older tests: the control
    "e_96x128": (2, 96, 128, [(30, 20, 70, 60), None]),
}


def mover_originals(name):
    F, H, W, _ = MOVER_CASES[name]
    rng = np.random.Generator(np.random.PCG64(8000 + sorted(MOVER_CASES).index(name)))
    return rng.integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)


def mover_inputs(name, other_sizes=False):
    """-> (originals, repaired crops, saved masks, boxes) of a case for the far-face paste: crops and masks of the box's own size (the
    resize is then a copy and the paste sees arbitrary mask bytes), the mask's first row forced to 0 and its last to 255;
    `other_sizes`: crops and masks of sizes unlike their boxes"""
    F, H, W, boxes = MOVER_CASES[name]
    seed = 8100 + 10 * sorted(MOVER_CASES).index(name)
    repaired, masks = [], []
    for f, box in enumerate(boxes):
        if box is None:
            continue
        w, h = box[2] - box[0], box[3] - box[1]
        cw, ch = (w + 3 + f, max(1, h - 2)) if other_sizes else (w, h)
        repaired.append(random_image(seed + f, ch, cw))
        m = random_image(seed + 5 + f, ch, cw, 0, 1, 256)
        if ch > 1:
            m[0], m[-1] = 0, 255
        masks.append(m)
    return mover_originals(name), repaired, masks, boxes


def first_difference(got, want):
    """(number of differing bytes, the first differing (frame, y, x, c) or None) of two [F, H, W, 3] batches"""
    diff = np.argwhere(np.asarray(got) != np.asarray(want))
    return len(diff), (tuple(int(v) for v in diff[0]) if len(diff) else None)


def piece_hits(box, W, r):
    """`byte_piece_hits` of csrc/vrg_byte_mover.hpp restated (tests/test_byte_movers_host.py holds the two equal): may bytes r .. r + 15 of a
    frame touch the (left, top, right, bottom) box?"""
    left, top, right, bottom = box
    pitch = W * 3
    y0, y1 = r // pitch, (r + 15) // pitch
    if y1 < top or y0 >= bottom:
        return False
    if y0 != y1:
        return True
    xs, xe = (r - y0 * pitch) // 3, (r + 15 - y0 * pitch) // 3
    return xe >= left and xs < right


def classify_pieces(name):
    """One record per 16-byte piece of the flat batch of a case, as the movers see it when the batch lies on the 16-byte grid:
    seams (frame boundaries inside the piece), tail (the batch ends inside it), walk (the kernel goes byte by byte: seams or tail),
    rows (1 or more, of an in-frame piece, from y0 to y1), asked (the `byte_piece_hits` answer for an in-frame piece whose frame has a box, else None),
    touches (a byte of the piece lies in a box), first_col / last_col (a byte in the box's first / last column),
    ends_before / starts_after (a one-row piece inside the box's rows that ends one byte before the box / starts one byte after it),
    later_box_touched / later_frame_without_box (of a seam-crossing piece: a frame it enters has a box it touches / has no box)."""
    F, H, W, boxes = MOVER_CASES[name]
    pitch, fb = W * 3, H * W * 3
    total = F * fb
    b = np.arange(total)
    f, r = b // fb, b % fb
    y, x = r // pitch, (r % pitch) // 3
    has = np.array([bx is not None for bx in boxes])
    geo = np.array([bx if bx is not None else (0, 0, 0, 0) for bx in boxes])
    left, top, right, bottom = (geo[f, i] for i in range(4))
    inside = has[f] & (x >= left) & (x < right) & (y >= top) & (y < bottom)
    out = []
    for b0 in range(0, total, PIECE):
        sl = slice(b0, min(b0 + PIECE, total))
        f0, r0 = int(f[b0]), int(r[b0])
        rec = dict(case=name, b0=b0, frame=f0, seams=int(f[sl][-1]) - f0, tail=b0 + PIECE > total)
        rec["walk"] = r0 + PIECE > fb
        rec["touches"] = bool(inside[sl].any())
        rec["first_col"] = bool((inside[sl] & (x[sl] == left[sl])).any())
        rec["last_col"] = bool((inside[sl] & (x[sl] == right[sl] - 1)).any())
        rec["rows"] = rec["asked"] = None
        rec["ends_before"] = rec["starts_after"] = False
        if not rec["walk"]:
            y0, y1 = r0 // pitch, (r0 + 15) // pitch
            rec["rows"], rec["y0"], rec["y1"] = y1 - y0 + 1, y0, y1
            if boxes[f0] is not None:
                bl, bt, br, bb = boxes[f0]
                rec["asked"] = piece_hits(boxes[f0], W, r0)
                if y0 == y1 and bt <= y0 < bb:
                    rec["ends_before"] = r0 + 15 - y0 * pitch == bl * 3 - 1
                    rec["starts_after"] = r0 - y0 * pitch == br * 3
        later = sorted(set(int(v) for v in f[sl]) - {f0})
        rec["later_box_touched"] = any(bool((inside[sl] & (f[sl] == g)).any()) for g in later)
        rec["later_frame_without_box"] = any(boxes[g] is None for g in later)
        out.append(rec)
    return out


def box_first_byte_offsets(name):
    """where in its 16-byte piece the first byte of every box of a case lies"""
    F, H, W, boxes = MOVER_CASES[name]
    return [(f * H * W * 3 + (bx[1] * W + bx[0]) * 3) % PIECE for f, bx in enumerate(boxes) if bx is not None]

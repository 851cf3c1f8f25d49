"""Shared by tests/test_landmark_input_host.py, tests/test_gpu_landmark_input.py, tools/make_golden_landmark_input.py and
tools/bench_landmark_input.py.

The landmark estimator's input is ``cv2.cvtColor(cv2.resize(rgb, (320, 320), interpolation=cv2.INTER_AREA), cv2.COLOR_RGB2BGR)`` of a
face box.  ``restated``: that, from the independent numpy restatement of cv2's INTER_AREA in tests/grid_support.py and a channel flip.
``GEOMETRIES``: the boxes of the sweep with the rule each takes.  ``recorded_detector``: a stand-in for YuNet whose rows are a fixed
function of the bytes it is shown (the golden fixture).  ``steady_detector`` / ``similarity_fit``: a detector whose landmarks move a little
with the picture and a least-squares similarity, for the node's two routes."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np

import grid_support as G
from conftest import GOLDEN, PKG_DIR, ROOT

F32 = np.float32
SIDE = 320
THUMB_BYTES = SIDE * SIDE * 3

# box (h, w) -> the rule cv2 takes to 320 x 320; `node`: does the node ever ask for it (the reference resizes nothing below 2 x 2)
GEOMETRIES = (
    ((320, 320), G.COPY, True),
    ((640, 640), G.FAST_2X2, True),
    ((960, 1280), G.FAST, True),
    ((321, 321), G.GENERAL, True),
    ((333, 517), G.GENERAL, True),
    ((1080, 700), G.GENERAL, True),
    ((2160, 2160), G.GENERAL, True),
    ((319, 319), G.LINEAR, True),
    ((40, 40), G.LINEAR, True),
    ((2, 2), G.LINEAR, True),
    ((2, 500), G.LINEAR, True),
    ((200, 400), G.LINEAR, True),           # one axis shrinks, the other enlarges
    ((1, 1), G.LINEAR, False),              # ABI only
)
# beyond the list above: rows so wide that 64 columns need more source bytes than a wave stages at a time (cps < 64: segments of columns)
SEGMENTED = (
    ((321, 7000), G.GENERAL, True),
    ((2, 7000), G.LINEAR, True),
)
KINDS = ("uniform", "checker", "ramp")

# The share of bytes that differ (by one level) from the float64 filters, measured on the numpy restatement ALONE at the geometries above
# on the three frame kinds (measure_shares(); DESIGN.md section 4 has the table).  grid_support's caps (1.5 x AREA_WORST_SHARE = 3 %,
# 1.5 x LINEAR_WORST_SHARE = 6.68 %) were measured on other geometries and on uniform / smooth frames; a (geometry, kind) whose restatement
# alone passes its cap is listed here, left out of the share assertion (not of the one-level bound, not of any byte equality) and named in
# 319 x 319 shows 12.7 .. 12.9 % on all three kinds, 200 x 400 6.84 % on the ramp (6.41 % on uniform bytes).
SHARE_EXEMPT = ((319, 319), (200, 400))


def mode_name(mode):
    return G.MODE_NAMES[mode]


def make_box(kind, h, w, seed):
    """one [h, w, 3] uint8 R,G,B image: uniform random bytes, a 0 / 255 checker of single pixels (shifted per channel), or ramps"""
    if kind == "uniform":
        return G.bytes_frames((h, w, 3), seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((h, w, 3), dtype=np.uint8)
    for c in range(3):
        if kind == "checker":
            out[:, :, c] = np.where((yy + xx + c + seed) % 2 == 0, 0, 255)
        elif kind == "ramp":
            out[:, :, c] = ((xx * (3 + c) + yy * (5 - c) + 37 * c + seed) % 256)
        else:
            raise ValueError(kind)
    return out


def restated(u8):
    """[h, w, 3] uint8 R,G,B -> [320, 320, 3] uint8 B,G,R"""
    return np.ascontiguousarray(G.resize_area(np.asarray(u8), SIDE, SIDE)[..., ::-1])


def yardstick(u8):
    return np.ascontiguousarray(G.yardstick64(np.asarray(u8), SIDE, SIDE)[..., ::-1])


def sha(array):
    return hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()


def measure_shares():
    """{(h, w, kind): (levels, share)} of the restatement alone against the float64 filters"""
    out = {}
    for (h, w), _, _ in GEOMETRIES:
        for kind in KINDS:
            u8 = make_box(kind, h, w, 7)
            out[(h, w, kind)] = G.differences(restated(u8), yardstick(u8))
    return out


def share_cap(mode):
    return 1.5 * (G.LINEAR_WORST_SHARE if mode == G.LINEAR else G.AREA_WORST_SHARE)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the header on the host
# ---------------------------------------------------------------------------------------------------------------------------------------
class ThumbDesc(C.Structure):
    """vrg_thumb_desc"""
    _fields_ = [("xtab", C.c_void_p), ("ytab", C.c_void_p), ("offset", C.c_int64), ("which", C.c_int32),
                ("box_w", C.c_int32), ("box_h", C.c_int32), ("mode", C.c_int32), ("cps", C.c_int32), ("inv", C.c_float)]


def host_source():
    return os.path.join(ROOT, "tests", "host_math", "thumbs_check.cpp")


def build_host_lib(directory):
    out = os.path.join(str(directory), "libthumbs_check.so")
    subprocess.run(["g++", *G.HOST_FLAGS, "-fPIC", "-shared", "-I", os.path.join(PKG_DIR, "csrc"), host_source(), "-o", out], check=True)
    lib = C.CDLL(out)
    P = C.c_void_p
    lib.hm_thumb.argtypes = [P, C.c_int32, C.c_int32, P]
    lib.hm_thumb.restype = None
    lib.hm_thumb_plan.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    lib.hm_thumb_plan.restype = C.c_int32
    lib.hm_thumb_desc_ok.argtypes = [C.POINTER(ThumbDesc), C.c_int64, C.c_int32]
    lib.hm_thumb_desc_ok.restype = C.c_int32
    lib.hm_thumb_desc_bytes.argtypes = []
    lib.hm_thumb_desc_bytes.restype = C.c_int32
    return lib


def host_thumb(lib, u8):
    x = np.ascontiguousarray(u8, dtype=np.uint8)
    out = np.empty((SIDE, SIDE, 3), dtype=np.uint8)
    lib.hm_thumb(x.ctypes.data, x.shape[0], x.shape[1], out.ctypes.data)
    return out


def host_plan(lib, h, w):
    mode, cps, inv = C.c_int32(), C.c_int32(), C.c_float()
    assert lib.hm_thumb_plan(h, w, C.byref(mode), C.byref(cps), C.byref(inv)) == 1
    return mode.value, cps.value, inv.value


# ---------------------------------------------------------------------------------------------------------------------------------------
# stand-ins for the network and the fit
# ---------------------------------------------------------------------------------------------------------------------------------------
def recorded_detector(bgr):
    """`[n, 15]` float32 rows that are a fixed function of the bytes shown (n = 1 .. 3, sometimes two rows share the best score: the first
    wins), or None for an all-black picture"""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.shape == (SIDE, SIDE, 3), (bgr.dtype, bgr.shape)
    if not bgr.any():
        return None
    digest = hashlib.sha256(np.ascontiguousarray(bgr).tobytes()).digest()
    rng = np.random.Generator(np.random.PCG64(int.from_bytes(digest[:8], "little")))
    n = 1 + digest[8] % 3
    rows = rng.uniform(0.0, float(SIDE), (n, 15)).astype(F32)
    rows[:, -1] = rng.uniform(0.1, 1.0, n).astype(F32)
    if n > 1 and digest[9] % 2:
        rows[:, -1] = rows[:, -1].max()                       # ties
    return rows


CANONICAL = np.array([[112.0, 128.0], [208.0, 128.0], [160.0, 184.0], [120.0, 236.0], [200.0, 236.0]], dtype=np.float64)


def steady_detector(bgr):
    """a face whose five landmarks sit near their usual places and move by a few pixels with the picture's channel and quadrant means; a
    picture darker than 8 on average has no face; a second, weaker row comes first so that the choice of the best row takes part"""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.shape == (SIDE, SIDE, 3), (bgr.dtype, bgr.shape)
    x = bgr.astype(np.float64)
    if x.mean() < 8.0:
        return np.zeros((0, 15), dtype=F32)
    q = np.array([x[:160, :160].mean(), x[:160, 160:].mean(), x[160:, :160].mean(), x[160:, 160:].mean(), x[80:240, 80:240].mean()])
    c = x.reshape(-1, 3).mean(axis=0)
    points = CANONICAL.copy()
    points[:, 0] += (q - q.mean()) / 6.0 + (c[0] - c[2]) / 8.0
    points[:, 1] += (q[::-1] - q.mean()) / 7.0 + (c[1] - 128.0) / 16.0
    best = np.concatenate([[60.0, 60.0, 200.0, 220.0], points.reshape(-1), [0.9]]).astype(F32)
    weak = np.concatenate([[10.0, 10.0, 50.0, 50.0], points.reshape(-1)[::-1], [0.4]]).astype(F32)
    return np.stack([weak, best])


def similarity_fit(generated_points, source_points):
    """the least-squares similarity (scale, rotation, shift) that carries the generated points onto the source points: float64 2 x 3"""
    g, s = np.asarray(generated_points, dtype=np.float64), np.asarray(source_points, dtype=np.float64)
    a = np.zeros((10, 4))
    a[0::2] = np.stack([g[:, 0], -g[:, 1], np.ones(5), np.zeros(5)], axis=1)
    a[1::2] = np.stack([g[:, 1], g[:, 0], np.zeros(5), np.ones(5)], axis=1)
    (p, r, tx, ty), *_ = np.linalg.lstsq(a, s.reshape(-1), rcond=None)
    return np.array([[p, -r, tx], [r, p, ty]], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the golden fixture (tools/make_golden_landmark_input.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
def golden_paths():
    return os.path.join(GOLDEN, "landmark_input.json"), os.path.join(GOLDEN, "landmark_input.npz")


def cv2_fixture_path():
    return os.path.join(GOLDEN, "landmark_input_cv2.npz")


def case_image(case):
    h, w = case["box"]
    if case["kind"] == "black":
        return np.zeros((h, w, 3), dtype=np.uint8)
    return make_box(case["kind"], h, w, case["seed"])


def golden():
    with open(golden_paths()[0]) as fh:
        return json.load(fh), np.load(golden_paths()[1])


def cv2_pin_inputs():
    """the byte images of the cv2 pin: every geometry the node can ask for, uniform bytes"""
    return [(f"t{i}_{h}x{w}", make_box("uniform", h, w, 31)) for i, ((h, w), _, node) in enumerate(GEOMETRIES) if node and h * w <= 1280 * 960]

"""Shared by tests/test_anchor_host.py and tests/test_gpu_anchor.py: the cases of the anchor kernels, their expected values from the LIVE
libraries (Pillow and numpy -- no test reads the reference tree), the stand-in for VideoHelperSuite's batch manager, the fixture recorded
from the reference's five node classes (tests/golden/anchor_roundtrip.*, tools/record_anchor_golden.py) and the host build of
csrc/vrg_anchor_math.hpp."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import torch

from conftest import GOLDEN, PKG_DIR, ROOT

with open(os.path.join(GOLDEN, "anchor_roundtrip.json")) as _fh:
    FIXTURE = json.load(_fh)
ARRAYS = dict(np.load(os.path.join(GOLDEN, "anchor_roundtrip.npz")))

# (width, height).  The first picture of a call gives the size; the others of the issue's list: the copy route, a shrink with more than
# one tap a side, an enlargement, 1 x 1, one axis equal, a long thin one -- and, added, its transpose, whose 16 output rows take taps from
# more source rows than one LDS chunk (ANC_SLOTS = 128) holds
FIRST = (40, 24)
OTHERS = ((40, 24), (97, 61), (17, 9), (1, 1), (41, 24), (333, 7), (7, 333))
# further first pictures: 1 x 1, a row length off the 16-byte grid, a whole tile, and two ragged tile columns
FIRSTS = ((1, 1), (13, 5), (64, 64), (70, 20))
BATCHES = (1, 2, 7)
LAUNCH_RECORDS = 32768

STORE_SHAPES = ((1, 1), (5, 13), (24, 40))          # (height, width)
STORE_FRAMES = (1, 5)
STORE_CHANNELS = (3, 4)


def picture(seed, size):
    """[h, w, 3] uint8: a ramp plus seeded noise, so that a shifted or transposed result cannot pass"""
    w, h = size
    rng = np.random.default_rng(seed)
    ramp = (np.arange(h)[:, None, None] * 7 + np.arange(w)[None, :, None] * 3 + np.arange(3)[None, None, :] * 50) % 256
    return ((ramp + rng.integers(0, 128, (h, w, 3))) % 256).astype(np.uint8)


def load_expected(pictures, size=None):
    """what the reference's loader yields, from live Pillow and numpy"""
    from PIL import Image
    w, h = size if size is not None else (pictures[0].shape[1], pictures[0].shape[0])
    return np.stack([np.asarray(Image.fromarray(a).resize((w, h), Image.Resampling.LANCZOS), dtype=np.float32) / 255.0 for a in pictures])


def store_expected(x, bgr=False):
    """what the reference's store writes, from live numpy (NaN: whatever this numpy yields; the cast warns)"""
    with np.errstate(invalid="ignore"):
        out = (np.asarray(x)[..., :3].clip(0, 1) * 255).round().astype("uint8")
    return np.ascontiguousarray(out[..., ::-1]) if bgr else out


def load_pictures(first, n, seed=0):
    """n pictures: `first`, then OTHERS in turn"""
    sizes = [first] + [OTHERS[i % len(OTHERS)] for i in range(n - 1)]
    return [picture(seed * 100 + i, s) for i, s in enumerate(sizes)]


def tie_table():
    """fp32: every k / 255 and (k +- 0.5) / 255 with its two float neighbours, values below 0 and above 1, -0.0, subnormals, the
    infinities and NaN"""
    k = np.arange(256, dtype=np.float64)
    base = np.concatenate([k / 255.0, (k + 0.5) / 255.0, (k - 0.5) / 255.0]).astype(np.float32)
    near = np.concatenate([base, np.nextafter(base, np.float32(2)), np.nextafter(base, np.float32(-2))])
    special = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, -0.1, -300.0, 1.0000001, 1.1, 300.0, np.inf, -np.inf, np.nan, -np.nan, 0.999999],
                       dtype=np.float32)
    return np.concatenate([near, special])


def seam_batch(channels=3):
    """the tie table as [2, 1, w, channels] frames whose 3 w bytes are no multiple of 16: the frame seam falls inside a 16-byte piece"""
    values = tie_table()
    w = (values.size + 5) // 6
    while (3 * w) % 16 == 0:
        w += 1
    flat = np.full(2 * w * 3, 0.25, dtype=np.float32)
    flat[:values.size] = values
    x = flat.reshape(2, 1, w, 3)
    if channels > 3:
        x = np.concatenate([x, np.full((2, 1, w, channels - 3), 7.0, dtype=np.float32)], axis=3)
    return np.ascontiguousarray(x)


def store_batch(n, hw, channels, seed):
    rng = np.random.default_rng(seed)
    x = (rng.random((n, hw[0], hw[1], channels), dtype=np.float32) * 1.2 - 0.1).astype(np.float32)
    return np.ascontiguousarray(np.round(x * 510) / 510 if seed % 2 else x)          # odd seeds: every value a k / 255 or a tie


class MetaBatch:
    """what the nodes touch of VideoHelperSuite's batch manager"""

    def __init__(self, frames_per_batch, total_frames):
        self.inputs, self.frames_per_batch, self.total_frames, self.has_closed_inputs = {}, frames_per_batch, total_frames, False

    def state(self):
        return {"inputs": sorted(self.inputs), "sizes": {k: [v[1], v[2]] for k, v in self.inputs.items()}, "total_frames": self.total_frames,
                "has_closed_inputs": self.has_closed_inputs}


def write_sources(folder):
    """the fixture's input pictures and its two non-image files under `folder`, as the recorder laid them out"""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i, rec in enumerate(FIXTURE["pictures"]):
        Image.fromarray(ARRAYS[f"picture.{i}"], "RGB").save(os.path.join(folder, rec["name"]), format="BMP" if rec["name"].endswith(".bmp") else "PNG")
    for name in FIXTURE["ignored"]:
        with open(os.path.join(folder, name), "wb") as fh:
            fh.write(b"not an image")
    return folder


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    view = {4: np.uint32, 1: np.uint8}[got.dtype.itemsize]
    return int((got.view(view) != want.view(view)).sum())


def build_host_lib(directory):
    out = os.path.join(str(directory), "libanchor_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "anchor_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
    lib.hm_anchor_check.argtypes = [P, I64, P, I64, I64, I32, I32]
    lib.hm_anchor_frames.argtypes = [P, I64, P, I64, P, I64, P, I32, I32, P]
    lib.hm_anchor_store.argtypes = [P, I64, I32, I32, P]
    lib.hm_anchor_store.restype = None
    lib.hm_anchor_constant.argtypes = [I32]
    for fn in (lib.hm_anchor_check, lib.hm_anchor_frames, lib.hm_anchor_constant):
        fn.restype = C.c_int
    return lib


def host_frames(ops, lib, pictures, size=None, calls=None):
    """ops.anchor_frames with the host-compiled header in place of the launch: the package's own plan and host check, then plain loops"""
    pics = [np.ascontiguousarray(p) for p in pictures]
    desc, tables, src_bytes, (h, w) = ops.anchor_plan([p.shape[:2] for p in pics], size)
    ops.anchor_check(desc, tables, src_bytes, h, w)
    src = np.concatenate([p.reshape(-1) for p in pics])
    out = np.full((len(pics), h, w, 3), -7.0, dtype=np.float32)
    tables = np.ascontiguousarray(tables, dtype=np.int32)
    count = np.zeros(1, dtype=np.int32) if calls is None else calls
    rc = lib.hm_anchor_frames(src.ctypes.data, src_bytes, desc.ctypes.data, len(desc), tables.ctypes.data if tables.size else None, tables.size,
                              out.ctypes.data, h, w, count.ctypes.data)
    assert rc == 0, rc
    return out


def host_store(lib, x, bgr=False):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros(x.shape[:3] + (3,), dtype=np.uint8)
    lib.hm_anchor_store(x.ctypes.data, x.size // x.shape[3], x.shape[3], int(bgr), out.ctypes.data)
    return out


@contextlib.contextmanager
def nodes_on_host(monkeypatch, pkg_name, ops, lib):
    """the node modules with the two launches replaced by the host-compiled header: everything else -- the protocol, the folders, the
    seams -- runs as it is.  Yields (video enhance module, face fix module, launches)."""
    import importlib
    anchors = importlib.import_module(pkg_name + "._anchors")
    ve = importlib.import_module(pkg_name + ".VRGDG_VideoEnhanceNodes")
    ff = importlib.import_module(pkg_name + ".VRGDG_StandaloneFaceFixNodes")
    launches = []

    def frames(pictures, out=None, size=None):
        launches.append(("load", len(pictures)))
        return torch.from_numpy(host_frames(ops, lib, pictures, size))

    def stored(images, bgr=False):
        launches.append(("store", int(images.shape[0])))
        return host_store(lib, images.detach().cpu().numpy(), bgr)

    with monkeypatch.context() as m:
        m.setattr(anchors.ops, "anchor_frames", frames)
        m.setattr(anchors, "stored_bytes", stored)
        m.setattr(ve, "_log", lambda message: None)
        m.setattr(ff, "_log", lambda message: None)
        yield ve, ff, launches


@contextlib.contextmanager
def output_directory(monkeypatch, path):
    stub = types.ModuleType("folder_paths")
    stub.get_output_directory = lambda: str(path)
    with monkeypatch.context() as m:
        m.setitem(sys.modules, "folder_paths", stub)
        yield


def run_schedule(node, context, schedule, frames, to_numpy):
    """the calls of one recorded schedule against `node`; asserts every return, every state and every error"""
    mb = MetaBatch(schedule["frames_per_batch"], schedule["total_frames"])
    for call in schedule["calls"]:
        if "error" in call:
            try:
                node.load(context, mb, schedule["unique_id"])
                raise AssertionError("loaded where the reference raised")
            except FileNotFoundError as exc:
                assert type(exc).__name__ == call["error"] and str(exc) == call["text"]
        else:
            images, masks, count, ctx = node.load(context, mb, schedule["unique_id"])
            assert ctx is context and count == call["count"] and isinstance(count, int)
            assert list(images.shape) == call["shape"] and str(images.dtype) == call["dtype"]
            assert list(masks.shape) == call["mask_shape"] and str(masks.dtype) == call["mask_dtype"] and not masks.any()
            assert same_bits(to_numpy(images), frames[call["first"]:call["first"] + call["count"]]) == 0
        assert mb.state() == call["state"], (call, mb.state())

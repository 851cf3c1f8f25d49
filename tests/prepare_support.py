"""Shared by tests/test_prepare_host.py and tests/test_gpu_prepare.py: the recorded run of the reference's VRGDGVideoEnhancePrepare
(tests/golden/prepare.json + prepare.npz, made by tools/record_prepare_golden.py under ATEN_CPU_CAPABILITY=default), the seeded inputs of
its cases, the geometry sweep of the GPU test and csrc/vrg_prepare_math.hpp compiled for the host."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import torch

from conftest import GOLDEN, PKG_DIR, ROOT

F32P = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
I64P = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
U8P = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")

BICUBIC, BILINEAR, AREA, NEAREST = "Bicubic (recommended)", "Bilinear", "Area", "Nearest"
METHODS = (BICUBIC, BILINEAR, AREA, NEAREST)
STRETCH, CROP, LETTERBOX = "Stretch to dimensions", "Crop to fill", "Fit with letterbox (preserve all)"
FITS = (STRETCH, CROP, LETTERBOX)

with open(os.path.join(GOLDEN, "prepare.json")) as _fh:
    META = json.load(_fh)


def arrays():
    return np.load(os.path.join(GOLDEN, "prepare.npz"))


def seeded_frames(seed, shape):
    """The input of a recorded case (tools/record_prepare_golden.py: seeded_frames)"""
    g = torch.Generator().manual_seed(int(seed))
    return (torch.rand(tuple(shape), generator=g) * 1.2 - 0.1).contiguous()


def anchor_list(frame_count, interval):
    """every `interval`-th frame and the last one, stated on its own"""
    out = [i for i in range(frame_count) if i % interval == 0]
    return out if out[-1] == frame_count - 1 else out + [frame_count - 1]


# The sweep of the GPU test, (source height, width, channels) -> (target width, height): a 4x shrink, a shrink of about 2.7x, 1:1 and a
# 1.5x enlargement, on a 5 x 7 source, an RGBA source whose width is no multiple of 4, a source of more than one band and segment, and
# one wider than the stage buffer (2063 px of RGB = 6189 floats against 4096), which also goes to 97 columns: the plan cuts those into
# segments of fewer than 97 columns, so the seam the stage size makes lies inside the picture.
SOURCES = ((5, 7, 3), (37, 53, 4), (136, 241, 3), (6, 2063, 3))
WIDE_TARGET = (97, 3)
RATIOS = (4.0, 2.7, 1.0, 1.0 / 1.5)


def targets(source):
    h, w = source[0], source[1]
    return [(max(1, round(w / r)), max(1, round(h / r))) for r in RATIOS]


def geometries(ops, source):
    """every (fit mode, target) of a source: the stretch hits the ratio exactly, crop to fill and letterbox get a target of another
    aspect so that the rectangle hangs over / lies inside the frame"""
    out = []
    for tw, th in targets(source):
        out.append(ops.resize_geometry(source[0], source[1], tw, th, STRETCH))
        out.append(ops.resize_geometry(source[0], source[1], tw + 3, max(1, th - 1), CROP))
        out.append(ops.resize_geometry(source[0], source[1], tw + 5, th + 2, LETTERBOX))
    if source[1] * source[2] > 4096:
        out.append(ops.resize_geometry(source[0], source[1], *WIDE_TARGET, STRETCH))
    return out


def special_frames(shape, seed):
    """Seeded frames with the values the byte rounding can trip over sprinkled in: exact 0 and 1, k / 255, (k + 0.5) / 255 and its two
    fp32 neighbours, negatives and values above 1."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g) * 1.2 - 0.1).contiguous()
    k = np.arange(256, dtype=np.float32)
    half = ((k + np.float32(0.5)) / np.float32(255)).astype(np.float32)
    pool = np.concatenate([np.array([0.0, 1.0, -0.25, 1.5, -0.0], dtype=np.float32), k / np.float32(255), half,
                           np.nextafter(half, np.float32(2)), np.nextafter(half, np.float32(-1))]).astype(np.float32)
    flat = x.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[:min(flat.numel() // 2, 4 * pool.size)]
    flat[where] = torch.from_numpy(pool)[torch.arange(where.numel()) % pool.size]
    return x


def quantise(frames_f32):
    """numpy's (x * 255).round().astype("uint8") of an already clamped fp32 array: the bytes of the reference's PNG files"""
    return np.round(np.asarray(frames_f32, dtype=np.float32) * np.float32(255)).astype(np.uint8)


def geom13(shape, g):
    return np.array([shape[1], shape[2], shape[3], *g.src, g.out_h, g.out_w, *g.dst], dtype=np.int32)


def build_host_lib(directory):
    out = os.path.join(str(directory), "libprepare_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "prepare_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_prepare_constants.argtypes, lib.hm_prepare_constants.restype = [C.c_int32], C.c_int32
    lib.hm_prepare_plan.argtypes, lib.hm_prepare_plan.restype = [I32P, C.c_int32, I32P], C.c_int32
    lib.hm_prepare_cover.argtypes, lib.hm_prepare_cover.restype = [I32P, C.c_int32, I32P, I32P, I64P], C.c_int64
    lib.hm_prepare_bicubic.argtypes, lib.hm_prepare_bicubic.restype = [F32P, C.c_void_p, C.c_int64, I32P, C.c_void_p, C.c_void_p], None
    lib.hm_prepare_byte.argtypes, lib.hm_prepare_byte.restype = [C.c_float], C.c_uint8
    return lib


class stub_folder_paths:
    """``with stub_folder_paths(directory):`` -- a `folder_paths` module in sys.modules whose output directory is `directory`"""

    def __init__(self, directory):
        self.directory = str(directory)

    def __enter__(self):
        self.saved = sys.modules.get("folder_paths")
        mod = types.ModuleType("folder_paths")
        mod.get_output_directory = lambda: self.directory
        sys.modules["folder_paths"] = mod
        return mod

    def __exit__(self, *exc):
        if self.saved is None:
            sys.modules.pop("folder_paths", None)
        else:
            sys.modules["folder_paths"] = self.saved
        return False

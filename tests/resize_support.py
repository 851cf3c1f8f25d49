"""Shared by tests/test_resize_host.py and tests/test_gpu_resize.py: the recorded reference results (tests/golden/resize.npz + .json,
made by tools/make_golden_resize.py under ATEN_CPU_CAPABILITY=default) and csrc/vrg_resize_math.hpp compiled for the host."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from conftest import GOLDEN, PKG_DIR, ROOT

F32P = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")

with open(os.path.join(GOLDEN, "resize.json")) as _fh:
    META = json.load(_fh)


def arrays():
    return np.load(os.path.join(GOLDEN, "resize.npz"))


def build_host_lib(directory):
    out = os.path.join(str(directory), "libresize_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "resize_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_resize.argtypes = [F32P, F32P, C.c_int64, I32P, C.c_int32]
    lib.hm_resize.restype = None
    lib.hm_restore.argtypes = [F32P, F32P, F32P, C.c_int64, C.c_int64, I32P, C.c_int32, C.c_int32, C.c_float, C.c_float]
    lib.hm_restore.restype = None
    return lib


def geom13(shape, g):
    """in_h, in_w, in_c, src rectangle, out_h, out_w, dst rectangle: the 13 integers of the C entry points"""
    return np.array([shape[1], shape[2], shape[3], *g.src, g.out_h, g.out_w, *g.dst], dtype=np.int32)


def host_resize(lib, ops, x, geometry, resize_method):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty((x.shape[0], geometry.out_h, geometry.out_w, 3), dtype=np.float32)
    lib.hm_resize(x, out, x.shape[0], geom13(x.shape, geometry), ops.RESIZE_METHODS[ops.interpolation_mode(resize_method)])
    return out


def host_restore(lib, ops, work, originals, geometry, resize_method, strength, usable):
    work = np.ascontiguousarray(work, dtype=np.float32)
    originals = np.ascontiguousarray(originals, dtype=np.float32)
    out = np.empty_like(originals)
    lib.hm_restore(work, originals, out, usable, originals.shape[0], geom13(work.shape, geometry), originals.shape[3],
                   ops.RESIZE_METHODS[ops.interpolation_mode(resize_method)], np.float32(strength), np.float32(1.0 - float(strength)))
    return out


def mismatches(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((got.view(np.uint32) != want.view(np.uint32)).sum())

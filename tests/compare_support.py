"""Shared by tests/test_compare_host.py and tests/test_gpu_compare.py: the value sweep of the rgb24 rule, its expected bytes from LIVE
numpy (no test reads the reference tree), the fixture recorded from the reference's VRGDG_VideoCompareNode.py
(tests/golden/compare_paths.json, tools/make_golden_compare.py) and the host build of csrc/vrg_compare_math.hpp."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from conftest import GOLDEN, PKG_DIR, ROOT

with open(os.path.join(GOLDEN, "compare_paths.json")) as _fh:
    FIXTURE = json.load(_fh)

NAN_BYTE = 0            # numpy's conversion of NaN to uint8 is undefined (and warns); x86 numpy yields 0, the pack's convention


def levels():
    """k / 255 for k = 0 .. 255, the division in fp32: what a decoded byte is as an IMAGE value"""
    return np.arange(256, dtype=np.float32) / np.float32(255.0)


def sweep():
    """fp32: every k / 255 with its neighbours on both sides, (k + 0.5) / 255, 1.0 with its upper neighbour and 256 / 255, +-0.0, the
    smallest subnormal, -1e-30, -3, the infinities and NaN"""
    k = levels()
    half = ((np.arange(256, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)
    one = np.float32(1.0)
    special = np.array([one, np.nextafter(one, np.float32(2)), np.float32(256.0) / np.float32(255.0), 0.0, -0.0, 1e-45, -1e-30, -3.0, np.inf, -np.inf,
                        np.nan], dtype=np.float32)
    return np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-2)), half, special])


def expected(x):
    """the reference's expression, run live by numpy on the first three channels; NaN written out as NAN_BYTE"""
    rgb = np.asarray(x, dtype=np.float32)[..., :3]
    with np.errstate(invalid="ignore"):
        out = np.clip(rgb * 255.0, 0, 255).astype(np.uint8)
    out[np.isnan(rgb)] = NAN_BYTE
    return np.ascontiguousarray(out)


def rounded(x):
    """the rule of ops.anchor_store_bytes, from live numpy: what this kernel must NOT compute"""
    return (np.asarray(x, dtype=np.float32).clip(0, 1) * 255).round().astype(np.uint8)


def sweep_batch(channels=3, alpha=np.nan):
    """the sweep laid into [1, 16, 64, channels] (repeated to fill it); further channels hold `alpha`"""
    values = np.resize(sweep(), 16 * 64 * 3).reshape(1, 16, 64, 3)
    if channels > 3:
        values = np.concatenate([values, np.full((1, 16, 64, channels - 3), alpha, dtype=np.float32)], axis=3)
    return np.ascontiguousarray(values)


def batch(shape, seed):
    """fp32 frames of `shape`: levels, their neighbours and values beyond [0, 1], seeded"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, 256, shape)
    x = levels()[pick] + (rng.integers(-1, 2, shape) * np.float32(2.0 ** -24)).astype(np.float32)
    wild = rng.random(shape) < 0.1
    x[wild] = (rng.random(shape, dtype=np.float32) * 1.4 - 0.2)[wild]
    return np.ascontiguousarray(x.astype(np.float32))


def build_host_lib(directory):
    out = os.path.join(str(directory), "libcompare_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "compare_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_rgb24_frames.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    lib.hm_rgb24_frames.restype = None
    lib.hm_anchor_bytes.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.hm_anchor_bytes.restype = None
    lib.hm_rgb24_nan_byte.restype = C.c_int
    return lib


def host_rgb24(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.full(x.shape[:-1] + (3,), 0xA5, dtype=np.uint8)
    lib.hm_rgb24_frames(x.ctypes.data, x.size // x.shape[-1], x.shape[-1], out.ctypes.data)
    return out


def host_anchor(lib, values):
    values = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros(values.shape, dtype=np.uint8)
    lib.hm_anchor_bytes(values.ctypes.data, values.size, out.ctypes.data)
    return out


def decoded(value, tmp):
    """a recorded VHS_FILENAMES value as the node receives it ({"tuple": [...]} is a tuple, {tmp} the temporary root)"""
    if isinstance(value, str):
        return value.replace("{tmp}", tmp)
    if isinstance(value, dict) and set(value) == {"tuple"}:
        return tuple(decoded(v, tmp) for v in value["tuple"])
    if isinstance(value, dict):
        return {k: decoded(v, tmp) for k, v in value.items()}
    if isinstance(value, list):
        return [decoded(v, tmp) for v in value]
    return value


def lay_out(tmp, files):
    """the recorded folders and files under `tmp`"""
    for folder in FIXTURE["folders"]:
        os.makedirs(os.path.join(tmp, folder), exist_ok=True)
    for name in files:
        path = os.path.join(tmp, name)
        if name.endswith("/"):
            os.makedirs(path, exist_ok=True)
            continue
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as fh:
            fh.write(b"video")


class Folders:
    """what the node touches of ComfyUI's folder_paths, over `tmp`"""

    def __init__(self, tmp):
        self.tmp = str(tmp)

    def get_output_directory(self):
        return os.path.join(self.tmp, "output")

    def get_temp_directory(self):
        return os.path.join(self.tmp, "temp")

    def get_input_directory(self):
        return os.path.join(self.tmp, "input")

"""Shared by tests/test_crop_host.py and tests/test_gpu_crop.py: the recorded results of the reference's two Face Fix Prepare nodes
(tests/golden/crop.npz + crop.json, made by tools/make_golden_crop.py under ATEN_CPU_CAPABILITY=default) and the crop arithmetic of
csrc/vrg_resize_math.hpp compiled for the host (tests/host_math/crop_check.cpp).  The fixture holds no frames: the inputs are rebuilt
from a seed, the reference's 512 x 512 batches are recorded as SHA-256 digests plus the values at seeded positions."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np

from conftest import GOLDEN, PKG_DIR, ROOT

F32P = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
I64P = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
SAMPLES = 2048


def meta():
    with open(os.path.join(GOLDEN, "crop.json")) as fh:
        return json.load(fh)


def arrays():
    return np.load(os.path.join(GOLDEN, "crop.npz"))


def make_frames(shape, seed):
    """The input frames of a case: uniform in [-0.25, 1.25) from numpy's PCG64, so that the clamp of the crop matters."""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    return rng.random(tuple(shape), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)


def sample_positions(numel, seed):
    return np.random.Generator(np.random.PCG64(int(seed) + 1)).integers(0, int(numel), SAMPLES)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def frame_shas(batch):
    return [sha(f) for f in batch]


def entries_of(case):
    """the reference's entries as recorded: boxes as tuples"""
    return [dict(e, box=tuple(e["box"]) if e["box"] is not None else None) for e in case["entries"]]


def build_host_lib(directory):
    out = os.path.join(str(directory), "libcrop_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "crop_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_crop.argtypes = [F32P, C.c_int64, F32P, I64P, C.c_int64, C.c_int32, C.c_int32]
    lib.hm_crop.restype = None
    return lib


def plan_records(plan, channels):
    """one (src_offset, row_pitch, pixel_stride, box_w, box_h) per output frame of a plan, for frames [F][H][W][channels]"""
    h, w, c = plan.height, plan.width, int(channels)
    return np.array([(((f * h + t) * w + l) * c, w * c, c, r - l, b - t) for f, (l, t, r, b) in plan.sources], dtype=np.int64).reshape(-1, 5)


def host_crop(lib, frames, records, size=(512, 512)):
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    records = np.ascontiguousarray(records, dtype=np.int64).reshape(-1, 5)
    out = np.empty((records.shape[0], int(size[0]), int(size[1]), 3), dtype=np.float32)
    lib.hm_crop(frames.reshape(-1), frames.size, out, records, records.shape[0], int(size[0]), int(size[1]))
    return out


def mismatches(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((got.view(np.uint32) != want.view(np.uint32)).sum())


def describe_difference(case, batch, samples):
    """a readable account of where a batch leaves the recorded reference: frames whose digest differs, sampled values that differ"""
    batch = np.ascontiguousarray(batch, dtype=np.float32)
    frames = [k for k, (a, b) in enumerate(zip(frame_shas(batch), case["frame_sha256"])) if a != b]
    pos = sample_positions(batch.size, case["seed"])
    got = batch.reshape(-1)[pos]
    bad = np.nonzero(got.view(np.uint32) != samples.view(np.uint32))[0]
    worst = float(np.abs(got - samples).max()) if bad.size else 0.0
    return f"{case['key']}: frames with another digest {frames}; {bad.size} of {SAMPLES} sampled values differ, largest difference {worst:.3g}"

"""Shared by the resize tests: the recorded reference results (tests/golden/resize.npz + .json, made by tools/make_golden_resize.py
under ATEN_CPU_CAPABILITY=default), csrc/vrg_resize_math.hpp compiled for the host, and the LIVE yardstick of
tests/test_resize_torch_host.py and tests/test_gpu_resize_torch.py: torch's own F.interpolate, run in one child process per test file
with its plain CPU kernels (torch_results)."""
import ctypes as C
import json
import os
import subprocess
import sys
import zlib

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


# ------------------------------------------------------------------------------------------------
# The live yardstick: torch itself, in a child process that runs its plain CPU kernels
# ------------------------------------------------------------------------------------------------
# A case is a JSON-able dict.  `seed` + `shape` name its input frames (seeded_frames), the rest says what is done with them:
#   fit      _resize_batch of the node pack's contract: `target` (width, height), `fit`, `method`
#   undo     _restore_batch: back to `source` (width, height); under letterbox the content rectangle is cut out first
#   rect     a rectangle `src` (x0, y0, w, h) of the frames resampled to `size` (width, height), of which `window` (left, top, width,
#            height) is kept (None: all of it) -- the geometries ops.resize_geometry / restore_geometry never hand out: a source
#            rectangle off the origin on both axes, a crop that hangs over the frame on both axes
#   restore  the Restore node: `undo` of the working frames blended over `originals` (seeded_frames(originals_seed, originals_shape))
#            with `strength`, the first min(frame_count, working frames) frames, everything clamped
BICUBIC, BILINEAR, AREA, NEAREST = "Bicubic (recommended)", "Bilinear", "Area", "Nearest"
METHODS = (BICUBIC, BILINEAR, AREA, NEAREST)
STRETCH, CROP, LETTERBOX = "Stretch to dimensions", "Crop to fill", "Fit with letterbox (preserve all)"
FITS = (STRETCH, CROP, LETTERBOX)


def fit_case(seed, shape, target, fit, method):
    return {"kind": "fit", "seed": int(seed), "shape": list(shape), "target": list(target), "fit": fit, "method": method}


def undo_case(seed, shape, source, fit, method):
    return {"kind": "undo", "seed": int(seed), "shape": list(shape), "source": list(source), "fit": fit, "method": method}


def rect_case(seed, shape, src, size, method, window=None):
    return {"kind": "rect", "seed": int(seed), "shape": list(shape), "src": list(src), "size": list(size), "method": method,
            "window": None if window is None else list(window)}


def restore_case(seed, shape, originals_seed, originals_shape, fit, method, strength, frame_count):
    return {"kind": "restore", "seed": int(seed), "shape": list(shape), "originals_seed": int(originals_seed),
            "originals_shape": list(originals_shape), "fit": fit, "method": method, "strength": float(strength), "frame_count": int(frame_count)}


def seeded_frames(seed, shape):
    """the input frames of a case, here and in the child: values in [-0.1, 1.1), so that the clamp has something to do"""
    import torch
    g = torch.Generator().manual_seed(int(seed))
    return (torch.rand(tuple(shape), generator=g) * 1.2 - 0.1).contiguous()


def geometry_of(ops, case):
    """the ResizeGeometry the kernels get for a case: from the package's own helpers, which the child does not see"""
    h, w = case["shape"][1], case["shape"][2]
    if case["kind"] == "fit":
        return ops.resize_geometry(h, w, case["target"][0], case["target"][1], case["fit"])
    if case["kind"] == "undo":
        return ops.restore_geometry(h, w, case["source"][0], case["source"][1], case["fit"])
    if case["kind"] == "restore":
        return ops.restore_geometry(h, w, case["originals_shape"][2], case["originals_shape"][1], case["fit"])
    size_w, size_h = case["size"]
    left, top, out_w, out_h = case["window"] or (0, 0, size_w, size_h)
    return ops.ResizeGeometry(out_h, out_w, tuple(case["src"]), (-left, -top, size_w, size_h))


# The child.  Written from torch's public API and the contract of the node pack: F.interpolate on the [..., :3].permute(0, 3, 1, 2) VIEW
# (channels-last memory: this decides which of torch's kernels runs), align_corners=False for bilinear and bicubic, crop to fill as a
# slice of the resampled frame, letterbox as zero F.pad, .permute(0, 2, 3, 1).clamp(0, 1); the restore direction slices the letterbox's
# content rectangle from the working frames before the stretch.  It never touches torch.cuda.
_TORCH_CHILD = r'''
import json, os, sys, zlib
import numpy as np, torch, torch.nn.functional as F
if torch.get_num_threads() < 2:       # one thread: torch always takes its channels-last bilinear kernel (csrc/vrg_resize_math.hpp)
    torch.set_num_threads(2)
MODES = {"Nearest": "nearest", "Bilinear": "bilinear", "Bicubic (recommended)": "bicubic", "Area": "area"}
STRETCH, CROP, LETTERBOX = "Stretch to dimensions", "Crop to fill", "Fit with letterbox (preserve all)"
crcs = []

def frames(seed, shape):
    g = torch.Generator().manual_seed(int(seed))
    x = (torch.rand(tuple(shape), generator=g) * 1.2 - 0.1).contiguous()
    crcs.append(zlib.crc32(x.numpy().tobytes()))
    return x

def resample(x, width, height, method):
    mode = MODES.get(method, "bicubic")
    kw = {"align_corners": False} if mode in ("bilinear", "bicubic") else {}
    return F.interpolate(x[..., :3].permute(0, 3, 1, 2), size=(int(height), int(width)), mode=mode, **kw)

def finish(t):
    return t.permute(0, 2, 3, 1).clamp(0, 1)

def fit(x, width, height, fit_mode, method):
    in_h, in_w = int(x.shape[1]), int(x.shape[2])
    if fit_mode == STRETCH:
        return finish(resample(x, width, height, method))
    ratios = (width / in_w, height / in_h)
    scale = max(ratios) if fit_mode == CROP else min(ratios)
    w, h = max(1, int(round(in_w * scale))), max(1, int(round(in_h * scale)))
    y = resample(x, w, h, method)
    if fit_mode == CROP:
        left, top = max(0, (w - width) // 2), max(0, (h - height) // 2)
        return finish(y[:, :, top:top + height, left:left + width])
    left, top = max(0, (width - w) // 2), max(0, (height - h) // 2)
    return finish(F.pad(y, (left, max(0, width - w - left), top, max(0, height - h - top)), value=0.0))

def undo(x, width, height, fit_mode, method):
    if fit_mode == LETTERBOX:
        work_h, work_w = int(x.shape[1]), int(x.shape[2])
        scale = min(work_w / width, work_h / height)
        w, h = min(work_w, max(1, int(round(width * scale)))), min(work_h, max(1, int(round(height * scale))))
        left, top = max(0, (work_w - w) // 2), max(0, (work_h - h) // 2)
        x = x[:, top:top + h, left:left + w, :]
    return fit(x, width, height, STRETCH, method)

def run(c):
    x = frames(c["seed"], c["shape"])
    if c["kind"] == "fit":
        return fit(x, c["target"][0], c["target"][1], c["fit"], c["method"])
    if c["kind"] == "undo":
        return undo(x, c["source"][0], c["source"][1], c["fit"], c["method"])
    if c["kind"] == "rect":
        x0, y0, w, h = c["src"]
        y = resample(x[:, y0:y0 + h, x0:x0 + w, :], c["size"][0], c["size"][1], c["method"])
        if c["window"] is not None:
            left, top, ww, wh = c["window"]
            y = y[:, :, top:top + wh, left:left + ww]
        return finish(y)
    originals = frames(c["originals_seed"], c["originals_shape"])
    restored = undo(x, int(originals.shape[2]), int(originals.shape[1]), c["fit"], c["method"])
    out = originals.clone()
    usable, s = min(int(c["frame_count"]), int(restored.shape[0])), float(c["strength"])
    out[:usable, ..., :3] = originals[:usable, ..., :3] * (1.0 - s) + restored[:usable, ..., :3] * s
    return out.clamp(0, 1)

with open(sys.argv[1]) as fh:
    cases = json.load(fh)
meta, offset = [], 0
with open(sys.argv[2], "wb") as data, torch.no_grad():
    for c in cases:
        del crcs[:]
        out = run(c).contiguous().numpy()
        assert out.dtype == np.float32
        data.write(out.tobytes())
        meta.append({"shape": list(out.shape), "offset": offset, "inputs": list(crcs)})
        offset += out.size
prov = {"torch": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(), "threads": torch.get_num_threads(),
        "ATEN_CPU_CAPABILITY": os.environ.get("ATEN_CPU_CAPABILITY"), "cuda_initialized": bool(torch.cuda.is_initialized())}
with open(sys.argv[3], "w") as fh:
    json.dump({"provenance": prov, "results": meta}, fh)
'''


class TorchResults:
    """torch's result of every case, by its position in the list handed to torch_results, and what the child ran on"""

    def __init__(self, cases, values, meta):
        self.cases, self._values, self._meta, self.provenance = cases, values, meta["results"], meta["provenance"]

    def __len__(self):
        return len(self.cases)

    def __getitem__(self, i):
        m = self._meta[i]
        return self._values[m["offset"]:m["offset"] + int(np.prod(m["shape"]))].reshape(m["shape"])

    def inputs(self, i):
        """the input frames of case i (the working frames; for a restore the originals as well), checked to be the child's bytes"""
        c = self.cases[i]
        xs = [seeded_frames(c["seed"], c["shape"])]
        if c["kind"] == "restore":
            xs.append(seeded_frames(c["originals_seed"], c["originals_shape"]))
        assert [zlib.crc32(x.numpy().tobytes()) for x in xs] == self._meta[i]["inputs"], ("the child drew other input frames", c)
        return xs

    def describe(self):
        p = self.provenance
        return f"torch {p['torch']}, CPU capability {p['cpu_capability']}, {p['threads']} threads, {len(self)} cases"


def torch_results(cases, directory, timeout=600):
    """Start ONE child python with ATEN_CPU_CAPABILITY=default and have torch compute every case.  The comparison means something only
    against torch's plain kernels with at least two threads (the bilinear kernel choice), so both are asserted here."""
    directory = str(directory)
    paths = [os.path.join(directory, n) for n in ("cases.json", "results.f32", "results.json")]
    with open(paths[0], "w") as fh:
        json.dump(list(cases), fh)
    env = dict(os.environ, ATEN_CPU_CAPABILITY="default")
    subprocess.run([sys.executable, "-c", _TORCH_CHILD, *paths], check=True, env=env, cwd=ROOT, timeout=timeout)
    with open(paths[2]) as fh:
        meta = json.load(fh)
    prov = meta["provenance"]
    assert prov["cpu_capability"].upper() in ("DEFAULT", "NO AVX"), prov
    assert prov["threads"] >= 2 and not prov["cuda_initialized"], prov
    assert len(meta["results"]) == len(cases)
    return TorchResults(list(cases), np.fromfile(paths[1], dtype=np.float32), meta)

"""Shared by the First / Last guide tests (tests/test_flf_guide_host.py, tests/test_gpu_flf_guide.py): the cases, their seeded pictures,
csrc/vrg_flf_math.hpp compiled for the host, the recorded fixture (tests/golden/flf_guide.json, tools/make_golden_flf.py) and the LIVE
yardstick -- torch itself, in one child process with its plain CPU kernels, through the mechanism of resize_support.torch_results.

The child knows nothing of the package.  It is written from torch's public API and the reference's contract: the first pictures of two
IMAGE batches; unless the sizes agree, the centre-crop view of ``last.movedim(-1, 1)`` by the published common_upscale rule and
``F.interpolate(view, size=(h, w), mode="bilinear")``; per frame ``first * (1.0 - amount) + last * amount`` with ``amount`` a Python
double from the curve; ``torch.cat``."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import resize_support as rs
from conftest import GOLDEN, PKG_DIR, ROOT

F32P, I32P, mismatches = rs.F32P, rs.I32P, rs.mismatches
CURVES = ("smoothstep", "linear", "ease_in", "ease_out")
CHUNK = 32                      # the kernel's frames per workgroup; the tests assert that the package says the same

with open(os.path.join(GOLDEN, "flf_guide.json")) as _fh:
    FIXTURE = json.load(_fh)


def case(name, first, last, frames, start=0.05, end=0.90, curve="smoothstep", seed=0, first_specials=False, last_specials=False):
    """first = (h, w, c), last = (h, w): pictures of ``seed``; *_specials: -0.0, a subnormal, Inf, -Inf and NaN strewn over that picture"""
    return {"name": name, "first": [1, *first], "last": [1, last[0], last[1], first[2]], "frames": int(frames), "start": float(start),
            "end": float(end), "curve": curve, "seed": int(seed), "first_specials": bool(first_specials), "last_specials": bool(last_specials)}


# the smallest shapes at which the kernel can go wrong (every one runs on the GPU too) ...
SMALL_CASES = (
    # h*w*c = 2220 is a multiple of 4, w*c = 111 is not: lanes straddle rows; `last` is taller: the crop is in y
    [case(f"rows-{c}", (20, 37, 3), (33, 29), 9, curve=c, seed=1) for c in CURVES] +
    # h*w*c = 105: every frame after the first starts off the 16-byte grid and ends in a 1-float remainder; `last` is wider: crop in x
    [case(f"odd-{n}", (7, 5, 3), (5, 13), n, seed=2) for n in (1, 2, CHUNK + 1)] +
    [case("tiny-3", (3, 1, 3), (5, 2), 5, seed=3), case("tiny-4", (1, 1, 4), (3, 2), 5, seed=4), case("tiny-4-plain", (1, 1, 4), (1, 1), 5, seed=5),
     case("down-4x-rgba", (16, 12, 4), (64, 48), 9, seed=6),
     case("up", (24, 40, 3), (3, 2), 9, seed=7),
     case("plain-specials", (7, 5, 3), (7, 5), 9, seed=8, last_specials=True),
     case("plain-specials-grid", (20, 37, 3), (20, 37), 9, start=0.5, seed=9, first_specials=True, last_specials=True),
     case("first-specials", (20, 37, 3), (33, 29), 9, start=0.5, curve="linear", seed=10, first_specials=True),
     case("last-specials-resampled", (7, 5, 3), (5, 13), 9, start=0.5, curve="linear", seed=11, last_specials=True),
     case("half-rect", (3, 3, 3), (4, 9), 5, seed=12)])
HALF_PAIR = (9, 4, 3, 3)          # old_w, old_h, new_w, new_h of "half-rect": half the surplus is 2.5
# ... and the sizes at which torch changes its bilinear kernel: height + width 128 | 129, four channels with a view that stays
# channels-last contiguous (rows cropped, nothing cropped) or does not (columns cropped)
KERNEL_CASES = [case("sum-128", (64, 64, 3), (100, 90), 3, seed=20), case("sum-129", (64, 65, 3), (100, 90), 3, seed=21),
                case("large-rgb", (100, 90, 3), (150, 200), 3, seed=22),
                case("large-rgba-columns", (100, 90, 4), (120, 300), 3, seed=23), case("large-rgba-rows", (100, 90, 4), (300, 120), 3, seed=24),
                case("large-rgba-whole", (100, 90, 4), (200, 180), 3, seed=25),
                case("small-rgba-columns", (16, 12, 4), (20, 60), 3, seed=26)]
CASES = SMALL_CASES + KERNEL_CASES

# the pictures of a case: ONE text, executed here and in the child
_PICTURES = r'''
def flf_pictures(c):
    import torch
    g = torch.Generator().manual_seed(int(c["seed"]))
    first = (torch.rand(tuple(c["first"]), generator=g) * 1.2 - 0.1).contiguous()
    last = (torch.rand(tuple(c["last"]), generator=g) * 1.2 - 0.1).contiguous()
    specials = torch.tensor([-0.0, 1e-40, float("inf"), float("-inf"), float("nan")], dtype=torch.float32)
    for wanted, t in ((c["first_specials"], first), (c["last_specials"], last)):
        if wanted:
            flat = t.view(-1)
            for k in range(15):
                flat[(k * 37 + 5) % flat.numel()] = specials[k % 5]
    return first, last
'''
exec(_PICTURES)

_FLF_CHILD = r'''
import json, os, sys, zlib
import numpy as np, torch, torch.nn.functional as F
if torch.get_num_threads() < 2:       # one thread: torch always takes its channels-last bilinear kernel (csrc/vrg_resize_math.hpp)
    torch.set_num_threads(2)
''' + _PICTURES + r'''
def narrowed(samples, width, height):
    old_width, old_height = samples.shape[-1], samples.shape[-2]
    old_aspect, new_aspect = old_width / old_height, width / height
    x = y = 0
    if old_aspect > new_aspect:
        x = round((old_width - old_width * (new_aspect / old_aspect)) / 2)
    elif old_aspect < new_aspect:
        y = round((old_height - old_height * (old_aspect / new_aspect)) / 2)
    return samples.narrow(-2, y, old_height - y * 2).narrow(-1, x, old_width - x * 2)

def eased(value, name):
    return {"linear": value, "ease_in": value * value, "ease_out": 1.0 - (1.0 - value) * (1.0 - value)}.get(name, value * value * (3.0 - 2.0 * value))

def run(c):
    first, last = flf_pictures(c)
    crcs.extend(zlib.crc32(t.numpy().tobytes()) for t in (first, last))
    first, last = first[:1], last[:1]
    h, w = int(first.shape[1]), int(first.shape[2])
    if int(last.shape[1]) != h or int(last.shape[2]) != w:
        last = F.interpolate(narrowed(last.movedim(-1, 1), w, h), size=(h, w), mode="bilinear").movedim(1, -1)
    start = max(0.0, min(0.95, c["start"]))
    end = max(start + 0.01, min(1.0, c["end"]))
    frames = []
    for index in range(c["frames"]):
        position = index / max(1, c["frames"] - 1)
        amount = eased(max(0.0, min(1.0, (position - start) / (end - start))), c["curve"])
        frames.append(first * (1.0 - amount) + last * amount)
    return torch.cat(frames, dim=0)

crcs = []
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


class FlfResults(rs.TorchResults):
    def inputs(self, i):
        """(first, last) of case i, checked to be the child's bytes"""
        import zlib
        xs = flf_pictures(self.cases[i])                                    # noqa: F821 -- defined by exec(_PICTURES)
        assert [zlib.crc32(x.numpy().tobytes()) for x in xs] == self._meta[i]["inputs"], ("the child drew other pictures", self.cases[i])
        return xs


def torch_results(cases, directory):
    """resize_support.torch_results -- one child under ATEN_CPU_CAPABILITY=default, at least two threads, no GPU touched, all of it
    asserted there -- with this file's child program in place of the resize one."""
    saved = rs._TORCH_CHILD
    rs._TORCH_CHILD = _FLF_CHILD
    try:
        r = rs.torch_results(cases, directory)
    finally:
        rs._TORCH_CHILD = saved
    r.__class__ = FlfResults
    return r


def build_host_lib(directory):
    out = os.path.join(str(directory), "libflf_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "flf_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_flf_guide.argtypes = [F32P, F32P, F32P, F32P, C.c_int64, I32P]
    lib.hm_flf_guide.restype = C.c_int
    return lib


def host_guide(lib, ops, first, last, c):
    """the frames of a case from the host-compiled header, with the package's own plan (rectangle, weights)"""
    first, last = (np.ascontiguousarray(t[:1].numpy()) for t in (first, last))
    rect, weights = ops.flf_plan(first.shape[1:], last.shape[1:], c["frames"], c["start"], c["end"], c["curve"])
    out = np.empty((c["frames"], *first.shape[1:]), dtype=np.float32)
    g9 = np.array([*first.shape[1:], last.shape[1], last.shape[2], *rect], dtype=np.int32)
    assert lib.hm_flf_guide(first, last, np.ascontiguousarray(weights), out, c["frames"], g9) == 0
    return out


def same_bits(got, want):
    """bit for bit, NaN by position (any NaN payload equals any other)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    return int((gn != wn).sum() + ((got.view(np.uint32) != want.view(np.uint32)) & ~gn & ~wn).sum())

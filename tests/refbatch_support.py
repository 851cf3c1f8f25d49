"""Shared by the reference-batch tests (tests/test_refbatch_host.py, tests/test_gpu_refbatch.py): the cases, their seeded pictures,
csrc/vrg_refbatch_math.hpp compiled for the host, the recorded fixture (tests/golden/multi_reference.json, tools/make_golden_refbatch.py)
and the LIVE yardstick -- torch itself, in one child process with its plain CPU kernels, through the mechanism of
resize_support.torch_results.

The child knows nothing of the package.  It is written from torch's public API and the reference's contract.  "scale": every picture to
the size of its megapixel budget by ``F.interpolate(picture.movedim(-1, 1), size, mode)`` -- always, also at an equal size.  "batch": the
later pictures padded with 1.0 to the wider channel count (the base re-padded), then, unless height and width agree, the centre-crop view
by the published common_upscale rule and ``F.interpolate`` over it; ``torch.cat``.  A result is the flat concatenation of its pictures."""
import contextlib
import ctypes as C
import json
import os
import subprocess

import numpy as np
import torch

import resize_support as rs
from conftest import GOLDEN, PKG_DIR, ROOT

F32P = rs.F32P
FILTERS = ("nearest-exact", "bilinear", "area", "bicubic")
METHODS = FILTERS + ("lanczos",)
TILE = 1024                      # the kernel's floats per workgroup; the tests assert that the package says the same

with open(os.path.join(GOLDEN, "multi_reference.json")) as _fh:
    FIXTURE = json.load(_fh)


def scale_case(name, shapes, method, megapixels, steps=1, seed=0, specials=()):
    return {"kind": "scale", "name": name, "shapes": [list(s) for s in shapes], "method": method, "megapixels": float(megapixels),
            "steps": int(steps), "seed": int(seed), "specials": list(specials)}


def batch_case(name, shapes, method, seed=0, specials=()):
    return {"kind": "batch", "name": name, "shapes": [list(s) for s in shapes], "method": method, "seed": int(seed), "specials": list(specials)}


# One call of seven pictures: 1 x 1, one column, 105 floats (every later picture of a dense buffer starts off the 16-byte grid), a row of
# 111 floats, RGBA, and sizes on both sides of every target.  0.008 MP: all grow, the largest target is 159 x 53; 0.0005 MP in steps of
# 4: three of them shrink
RAGGED = ((1, 1, 1, 3), (1, 3, 1, 4), (1, 7, 5, 3), (1, 20, 37, 3), (1, 16, 12, 4), (1, 64, 48, 4), (1, 33, 29, 3))
BUDGETS = ((0.008, 1), (0.0005, 4))
RAGGED_CASES = [scale_case(f"ragged-{m}-{mp}", RAGGED, m, mp, st, seed=1) for m in FILTERS for mp, st in BUDGETS]
FRAMES_CASES = [scale_case(f"frames-{m}", ((2, 9, 7, 4), (3, 4, 6, 3)), m, 0.0003, seed=2) for m in FILTERS]
# 16 x 16 at 256 pixels: the target IS the source, and the filter is evaluated all the same (Inf * 0)
EQUAL_MP = 256.0 / (1024 * 1024)
EQUAL_CASES = [scale_case(f"equal-{m}", ((1, 16, 16, 3), (1, 16, 16, 4)), m, EQUAL_MP, seed=3, specials=(0, 1)) for m in FILTERS]
# the sizes at which torch changes its bilinear kernel (flf_support.KERNEL_CASES as base <- picture), then what is new here: several frames
# (a view narrowed in rows is contiguous for one picture only) and a padded picture (F.pad makes it contiguous RGBA)
KERNEL_PAIRS = (("sum-128", (1, 64, 64, 3), (1, 100, 90, 3)), ("sum-129", (1, 64, 65, 3), (1, 100, 90, 3)),
                ("large-rgb", (1, 100, 90, 3), (1, 150, 200, 3)), ("large-rgba-columns", (1, 100, 90, 4), (1, 120, 300, 4)),
                ("large-rgba-rows", (1, 100, 90, 4), (1, 300, 120, 4)), ("large-rgba-whole", (1, 100, 90, 4), (1, 200, 180, 4)),
                ("small-rgba-columns", (1, 16, 12, 4), (1, 20, 60, 4)), ("frames-rgba-rows", (1, 100, 90, 4), (2, 300, 120, 4)),
                ("frames-rgba-whole", (1, 100, 90, 4), (2, 200, 180, 4)), ("large-pad-whole", (1, 100, 90, 4), (1, 200, 180, 3)))
KERNEL_CASES = [batch_case(name, (base, other), "bilinear", seed=20 + i) for i, (name, base, other) in enumerate(KERNEL_PAIRS)]
KERNEL_CASES += [scale_case("scale-rgba-large", ((1, 40, 30, 4),), "bilinear", 0.012, seed=40),
                 scale_case("scale-rgb-large", ((1, 40, 30, 3),), "bilinear", 0.012, seed=41)]
# the batch rule: the base re-padded to RGBA, a crop in y, a crop in x, and a picture that already fits and passes by `copy`
RULE = ((1, 20, 37, 3), (1, 33, 29, 4), (1, 5, 13, 3), (1, 20, 37, 3))
RULE_CASES = [batch_case(f"rule-{m}", RULE, m, seed=5, specials=(3,)) for m in FILTERS]
HALF_PAIR = (9, 4, 3, 3)          # old_w, old_h, new_w, new_h: half the surplus is 2.5
RULE_CASES += [batch_case(f"half-rect-{m}", ((1, 3, 3, 3), (1, 4, 9, 3)), m, seed=6) for m in FILTERS]
# a crop that leaves exactly the base's size: not the base's shape, so the filter runs, on both of torch's equal-size short-cuts
RULE_CASES += [batch_case(f"cropped-to-equal-{m}", ((1, 12, 16, 3), (2, 20, 16, 3)), m, seed=7, specials=(1,)) for m in FILTERS]
CASES = RAGGED_CASES + FRAMES_CASES + EQUAL_CASES + KERNEL_CASES + RULE_CASES

# the pictures of a case: ONE text, executed here and in the child
_PICTURES = r'''
def ref_pictures(c):
    import torch
    g = torch.Generator().manual_seed(int(c["seed"]))
    pictures = [(torch.rand(tuple(s), generator=g) * 1.2 - 0.1).contiguous() for s in c["shapes"]]
    specials = torch.tensor([-0.0, 1e-40, float("inf"), float("-inf"), float("nan")], dtype=torch.float32)
    for i in c["specials"]:
        flat = pictures[i].view(-1)
        for k in range(15):
            flat[(k * 37 + 5) % flat.numel()] = specials[k % 5]
    return pictures
'''
exec(_PICTURES)

_CHILD = r'''
import json, math, os, sys, zlib
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

def budget_size(h, w, megapixels, steps):
    by = math.sqrt(float(megapixels) * 1024 * 1024 / (w * h))
    steps = max(1, int(steps))
    return max(1, round(h * by / steps) * steps), max(1, round(w * by / steps) * steps)

def scaled(pictures, c):
    out = []
    for p in pictures:
        size = budget_size(p.shape[1], p.shape[2], c["megapixels"], c["steps"])
        out.append(F.interpolate(p.movedim(-1, 1), size=size, mode=c["method"]).movedim(1, -1))
    return out

def batched(pictures, c):
    base = pictures[0]
    kept = [base]
    for p in pictures[1:]:
        if p.shape[-1] != base.shape[-1]:
            most = max(p.shape[-1], base.shape[-1])
            if base.shape[-1] < most:
                base = F.pad(base, (0, most - base.shape[-1]), value=1.0)
                kept[0] = base
            if p.shape[-1] < most:
                p = F.pad(p, (0, most - p.shape[-1]), value=1.0)
        if p.shape[1:] != base.shape[1:]:
            p = F.interpolate(narrowed(p.movedim(-1, 1), base.shape[2], base.shape[1]), size=(base.shape[1], base.shape[2]),
                              mode=c["method"]).movedim(1, -1)
        kept.append(p)
    return [torch.cat(kept, dim=0)]

def run(c):
    pictures = ref_pictures(c)
    crcs.extend(zlib.crc32(t.numpy().tobytes()) for t in pictures)
    out = scaled(pictures, c) if c["kind"] == "scale" else batched(pictures, c)
    shapes.append([list(t.shape) for t in out])
    return torch.cat([t.contiguous().reshape(-1) for t in out])

crcs, shapes = [], []
with open(sys.argv[1]) as fh:
    cases = json.load(fh)
meta, offset = [], 0
with open(sys.argv[2], "wb") as data, torch.no_grad():
    for c in cases:
        del crcs[:], shapes[:]
        out = run(c).contiguous().numpy()
        assert out.dtype == np.float32
        data.write(out.tobytes())
        meta.append({"shape": list(out.shape), "offset": offset, "inputs": list(crcs), "shapes": shapes[0]})
        offset += out.size
prov = {"torch": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(), "threads": torch.get_num_threads(),
        "ATEN_CPU_CAPABILITY": os.environ.get("ATEN_CPU_CAPABILITY"), "cuda_initialized": bool(torch.cuda.is_initialized())}
with open(sys.argv[3], "w") as fh:
    json.dump({"provenance": prov, "results": meta}, fh)
'''


class RefResults(rs.TorchResults):
    def inputs(self, i):
        """the pictures of case i, checked to be the child's bytes"""
        import zlib
        xs = ref_pictures(self.cases[i])                                    # noqa: F821 -- defined by exec(_PICTURES)
        assert [zlib.crc32(x.numpy().tobytes()) for x in xs] == self._meta[i]["inputs"], ("the child drew other pictures", self.cases[i])
        return xs

    def pictures(self, i):
        """torch's pictures of case i, in their shapes"""
        flat, out, at = self[i], [], 0
        for shape in self._meta[i]["shapes"]:
            n = int(np.prod(shape))
            out.append(flat[at:at + n].reshape(shape))
            at += n
        return out


def torch_results(cases, directory):
    """resize_support.torch_results -- one child under ATEN_CPU_CAPABILITY=default, at least two threads, no GPU touched, all of it
    asserted there -- with this file's child program in place of the resize one."""
    saved = rs._TORCH_CHILD
    rs._TORCH_CHILD = _CHILD
    try:
        r = rs.torch_results(cases, directory)
    finally:
        rs._TORCH_CHILD = saved
    r.__class__ = RefResults
    return r


def run_case(ops, pictures, c, **kw):
    """a case through the package's public functions -> the list of its result pictures"""
    if c["kind"] == "scale":
        return ops.scale_reference_images(pictures, c["method"], c["megapixels"], c["steps"], **kw)
    return [ops.batch_reference_images(pictures, c["method"], **kw)]


def build_host_lib(directory):
    out = os.path.join(str(directory), "librefbatch_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "refbatch_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    P, I64 = C.c_void_p, C.c_int64
    lib.hm_refbatch_check.argtypes = [P, I64, I64, I64, I64]
    lib.hm_refbatch.argtypes = [P, I64, P, I64, P, I64, P, I64]
    lib.hm_refbatch_quantise.argtypes = [P, I64, P, I64, P, I64]
    for fn in (lib.hm_refbatch_check, lib.hm_refbatch, lib.hm_refbatch_quantise):
        fn.restype = C.c_int
    return lib


@contextlib.contextmanager
def on_host(monkeypatch, ops, lib):
    """the package's planning -- sizes, pads, rectangles, offsets, records -- with the host-compiled header in place of the launch: CPU
    pictures stay where they are and every record is computed by csrc/vrg_refbatch_math.hpp in plain loops"""
    launches = []

    def place(images, what):
        return torch.device("cpu"), [t.detach().contiguous() for t in images]

    def launch(dev, jobs, out):
        if not jobs:
            return
        desc, tiles, (f_base, f_floats), (b_base, b_bytes) = ops.refbatch_table(jobs, out.numel())
        launches.append((desc.copy(), tiles))
        if out.dtype == torch.uint8:
            rc = lib.hm_refbatch_quantise(f_base, f_floats, desc.ctypes.data, len(jobs), out.data_ptr(), out.numel())
        else:
            rc = lib.hm_refbatch(f_base, f_floats, b_base, b_bytes, desc.ctypes.data, len(jobs), out.data_ptr(), out.numel())
        assert rc == 0, rc

    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "device", contextlib.nullcontext)
        m.setattr(ops, "_refbatch_place", place)
        m.setattr(ops, "_refbatch_launch", launch)
        yield launches


def same_bits(got, want):
    """bit for bit, NaN by position (any NaN payload equals any other)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    return int((gn != wn).sum() + ((got.view(np.uint32) != want.view(np.uint32)) & ~gn & ~wn).sum())


def pil_lanczos(pictures, sizes):
    """comfy's ``lanczos`` with live Pillow and numpy: fp32 [B, H, W, 3] -> fp32 [B, h, w, 3] for every (picture, (h, w))"""
    from PIL import Image
    out = []
    for p, (h, w) in zip(pictures, sizes):
        frames = []
        for frame in p.numpy():
            image = Image.fromarray(np.clip(255. * frame, 0, 255).astype(np.uint8))
            frames.append(np.array(image.resize((w, h), resample=Image.Resampling.LANCZOS)).astype(np.float32) / 255.0)
        out.append(np.stack(frames))
    return out

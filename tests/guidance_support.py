"""Shared by the guidance tests (tests/test_guidance_host.py, tests/test_gpu_guidance.py): the cases, their seeded latents, the contract of
ops.ltx_guidance as plain torch, csrc/vrg_guidance_math.hpp compiled for the host, and the LIVE yardstick -- torch in one child process with
its plain CPU kernels, through the mechanism of resize_support.torch_results.

The child knows nothing of the package.  Per case and step it evaluates the contract twice: (a) on the fp32 latents, which is what the
reference's guider computes, and (b) on their ``.double()`` copies, the truth.  The bar every kernel result is held to:

    E(x) = max|x - truth| / max|truth|,     E(kernel) <= 2 * E(fp32 torch) + 2^-23

(the factor 2: element-wise roundings taken in another order where a phase is folded; 2^-23: cases in which fp32 torch happens to be exact).
Plain CFG with or without STG has no reduction and must equal (a) bit for bit.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import resize_support as rs
from conftest import PKG_DIR, ROOT

F32P = rs.F32P
F64P = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
SPAN = 4096                     # elements of a row one workgroup takes; the tests assert that the package says the same
OUTPUTS = ("guided", "negative", "average")


def case(name, shape, *, negative=True, mode="CFG", cfg=4.0, star=False, stg=None, rescale=0.0, eta=1.0, threshold=0.0, momentum=0.0, steps=1,
         sliced=None, special=None, seed=0):
    """sliced: "all" -- every latent is big[1:] of a tensor one batch entry longer -- or "positive"; special: a degenerate input (_LATENTS)"""
    return {"name": name, "shape": list(shape), "negative": bool(negative), "mode": mode, "cfg": float(cfg), "star": bool(star),
            "stg": None if stg is None else float(stg), "rescale": float(rescale), "eta": float(eta), "threshold": float(threshold),
            "momentum": float(momentum), "steps": int(steps), "sliced": sliced, "special": special, "seed": int(seed)}


SHAPES = {
    "rows70": ((2, 3, 2, 5, 7), None),              # row_len 70, no multiple of 4; three rows per batch
    "len1": ((3, 1, 1, 1), None),                   # 4-D, row_len 1, rows = batches
    "span+1": ((1, 2, 1, 1, SPAN + 1), None),       # a row that crosses a workgroup's span by one element
    "aligned48": ((2, 2, 3, 4, 4), None),           # everything on the 16-byte grid
    "slice": ((2, 3, 3, 5, 7), "all"),              # big[1:]: 315 floats in, 12 bytes off the grid
    "slice-mixed": ((2, 3, 3, 5, 7), "positive"),   # only positive is off the grid: the operands disagree
    "rows128": ((1, 128, 3, 4, 6), None),           # many short rows
    "chunks": ((1, 32768 + 5, 1, 1, 3), None),      # more rows than a grid's second dimension would take: the grid has one dimension
}
MODES = {
    "cfg": dict(),
    "cfg-stg": dict(stg=1.0),
    "none": dict(negative=False),
    "star": dict(star=True),
    "star-stg-rescale": dict(star=True, stg=0.75, rescale=0.7),
    "cfg-rescale": dict(rescale=0.5),
    "none-stg-rescale": dict(negative=False, stg=1.5, rescale=1.0),
    "apg": dict(mode="APG"),
    "apg-threshold": dict(mode="APG", threshold=5.0, eta=0.0),
    "apg-momentum": dict(mode="APG", momentum=-0.5, steps=2, eta=-0.5),
    "apg-all": dict(mode="APG", star=True, threshold=0.8, momentum=0.25, steps=2, eta=-0.5, stg=1.0, rescale=0.7),
}
EXACT_MODES = ("cfg", "cfg-stg", "none")            # no reduction: bit for bit



def _crossed(shape_name, kw):
    """Every mode on every shape, but one: with rows of ONE element the CFG-star negative n * (p * n / (n * n + 1e-8)) is p up to 1e-8, so
    the APG guidance p - n' is the residue of a cancellation -- about 1e-8 * p in exact arithmetic, below the 6e-8 * p of one fp32 rounding.
    No fp32 evaluation has a correct digit there (torch's own is 18 % off the truth), so an accuracy bar says nothing: on that shape
    "apg-all" runs without the star (the star on that shape is covered by "star" and "star-stg-rescale", where guided is not a residue)."""
    if shape_name == "len1" and kw.get("mode") == "APG" and kw.get("star"):
        return dict(kw, star=False)
    return kw


CASES = [case(f"{s}/{m}", shape, sliced=sliced, seed=100 * i + j, **_crossed(s, kw))
         for i, (s, (shape, sliced)) in enumerate(SHAPES.items()) for j, (m, kw) in enumerate(MODES.items())]
CASES += [
    case("zero-negative/star", (2, 3, 2, 5, 7), star=True, special="zero-negative", seed=901),
    case("zero-guidance-row/apg", (2, 3, 2, 5, 7), mode="APG", threshold=5.0, special="zero-guidance-row", seed=902),
    case("zero-positive-row/apg", (2, 3, 2, 5, 7), mode="APG", threshold=5.0, special="zero-positive-row", seed=903),
    case("constant-guided/rescale", (2, 3, 2, 5, 7), negative=False, stg=1.0, rescale=0.7, special="constant-guided", seed=904),
]
DEGENERATE = tuple(c["name"] for c in CASES if c["special"])


def is_exact(c):
    return c["name"].split("/")[1] in EXACT_MODES and not c["special"]


# The latents of a case and the contract of ops.ltx_guidance (section 1 of the operator's docstring, the reference's expressions in the
# reference's order): ONE text, executed here and in the child.
_CONTRACT = r'''
def guidance_latents(c):
    """per step (positive, negative, perturbed): the FULL tensors; where c["sliced"] says so the latent is full[1:]"""
    import torch
    g = torch.Generator().manual_seed(int(c["seed"]))
    shape = tuple(c["shape"])

    def draw(which):
        longer = c["sliced"] == "all" or (c["sliced"] == "positive" and which == "positive")
        full = (shape[0] + 1, *shape[1:]) if longer else shape
        rows = 1
        for v in full[:-3]:
            rows *= v
        # uniform in [-2, 2) (torch.rand draws the same bits under every CPU capability), rows of growing size: norms on both sides of a threshold
        ramp = torch.tensor([0.1 + 1.4 * r / max(1, rows - 1) for r in range(rows)], dtype=torch.float32).reshape(*full[:-3], 1, 1, 1)
        return ((torch.rand(full, generator=g) * 4.0 - 2.0) * ramp).contiguous()

    steps = []
    for _ in range(c["steps"]):
        p = draw("positive")
        n = draw("negative") if c["negative"] else None
        q = draw("perturbed") if c["stg"] is not None else None
        if c["special"] == "zero-negative":
            n.zero_()
        elif c["special"] == "zero-guidance-row":          # row 1 of batch 0: positive == negative
            n[0, 1] = p[0, 1]
        elif c["special"] == "zero-positive-row":
            p[1, 2] = 0.0
        elif c["special"] == "constant-guided":            # multiples of 1/8: p + 1.0 * (p - q) is 0.5 everywhere, exactly
            p = torch.round(p * 8.0) / 8.0
            q = 2.0 * p - 0.5
        steps.append((p, n, q))
    return steps


def guidance_view(c, which, t):
    if t is None:
        return None
    return t[1:] if c["sliced"] == "all" or (c["sliced"] == "positive" and which == "positive") else t


def guidance_contract(c, p, n, q, average):
    """{"guided", "negative" (with a star), "average" (APG with a momentum)} of one step, in the dtype of the latents"""
    import torch
    dims = [-1, -2, -3]
    out = {}
    if n is not None and c["star"]:
        b = p.shape[0]
        pf, nf = p.reshape(b, -1), n.reshape(b, -1)
        alpha = torch.sum(pf * nf, dim=1, keepdim=True) / (torch.sum(nf.square(), dim=1, keepdim=True) + 1e-8)
        n = n * alpha.reshape(b, *([1] * (n.ndim - 1)))
        out["negative"] = n
    if n is None:
        guided = p
    elif c["mode"] == "APG":
        g = p - n
        if c["momentum"] != 0.0:
            if average is not None:
                g = c["momentum"] * average + g
            out["average"] = g
        if c["threshold"] > 0:
            norm = g.norm(p=2, dim=dims, keepdim=True).clamp_min(1e-12)
            g = g * torch.minimum(torch.ones_like(norm), c["threshold"] / norm)
        g64 = g.double()
        u = torch.nn.functional.normalize(p.double(), dim=dims)
        par64 = (g64 * u).sum(dim=dims, keepdim=True) * u
        par, orth = par64.to(g.dtype), (g64 - par64).to(g.dtype)
        guided = p + (c["cfg"] - 1.0) * (orth + c["eta"] * par)
    else:
        guided = p + (c["cfg"] - 1.0) * (p - n)
    if q is not None:
        guided = guided + c["stg"] * (p - q)
    if c["rescale"] != 0.0:
        guided_std = guided.std().clamp_min(1e-12)
        guided = guided * (c["rescale"] * (p.std() / guided_std) + (1.0 - c["rescale"]))
    out["guided"] = guided
    return out


def guidance_steps(c, double):
    """the contract over the steps of a case, the running average fed back: a list of {name: tensor}"""
    results, average = [], None
    for p, n, q in guidance_latents(c):
        p, n, q = (guidance_view(c, w, t) for w, t in (("positive", p), ("negative", n), ("perturbed", q)))
        if double:
            p, n, q = (None if t is None else t.double() for t in (p, n, q))
        out = guidance_contract(c, p, n, q, average)
        average = out.get("average")
        results.append(out)
    return results
'''
exec(_CONTRACT)

_GUIDANCE_CHILD = r'''
import json, os, sys, zlib
import numpy as np, torch
if torch.get_num_threads() < 2:
    torch.set_num_threads(2)
''' + _CONTRACT + r'''
with open(sys.argv[1]) as fh:
    cases = json.load(fh)
meta, offset = [], 0
with open(sys.argv[2], "wb") as data, torch.no_grad():
    for c in cases:
        crcs = [zlib.crc32(t.numpy().tobytes()) for step in guidance_latents(c) for t in step if t is not None]
        parts, size = [], 0
        for kind, double in (("fp32", False), ("truth", True)):
            for step, out in enumerate(guidance_steps(c, double)):
                for name in sorted(out):
                    a = out[name].contiguous().numpy()
                    assert a.dtype == (np.float64 if double else np.float32)
                    flat = a.reshape(-1).view(np.float32)            # a double travels as two floats
                    data.write(flat.tobytes())
                    parts.append({"kind": kind, "step": step, "name": name, "shape": list(a.shape), "offset": size, "floats": int(flat.size)})
                    size += int(flat.size)
        meta.append({"shape": [size], "offset": offset, "inputs": crcs, "parts": parts})
        offset += size
prov = {"torch": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(), "threads": torch.get_num_threads(),
        "ATEN_CPU_CAPABILITY": os.environ.get("ATEN_CPU_CAPABILITY"), "cuda_initialized": bool(torch.cuda.is_initialized())}
with open(sys.argv[3], "w") as fh:
    json.dump({"provenance": prov, "results": meta}, fh)
'''


class GuidanceResults(rs.TorchResults):
    def latents(self, i):
        """the steps of case i as guidance_latents draws them, checked to be the child's bytes"""
        import zlib
        steps = guidance_latents(self.cases[i])                               # noqa: F821 -- defined by exec(_CONTRACT)
        crcs = [zlib.crc32(t.numpy().tobytes()) for step in steps for t in step if t is not None]
        assert crcs == self._meta[i]["inputs"], ("the child drew other latents", self.cases[i])
        return steps

    def part(self, i, kind, step, name):
        """one result of the child (kind "fp32" or "truth") as a numpy array, None where the step has no such output"""
        flat = self[i]
        for p in self._meta[i]["parts"]:
            if (p["kind"], p["step"], p["name"]) == (kind, step, name):
                a = flat[p["offset"]:p["offset"] + p["floats"]]
                return (a.view(np.float64) if kind == "truth" else a).reshape(p["shape"])
        return None


def torch_results(cases, directory):
    """resize_support.torch_results -- one child under ATEN_CPU_CAPABILITY=default, no GPU touched -- with this file's child program"""
    saved = rs._TORCH_CHILD
    rs._TORCH_CHILD = _GUIDANCE_CHILD
    try:
        r = rs.torch_results(cases, directory)
    finally:
        rs._TORCH_CHILD = saved
    r.__class__ = GuidanceResults
    return r


def error(got, truth):
    """E = max|got - truth| / max|truth| in fp64 (0 / 0 = 0)"""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    assert got.shape == truth.shape, (got.shape, truth.shape)
    top = float(np.max(np.abs(truth))) if truth.size else 0.0
    diff = float(np.max(np.abs(got - truth))) if truth.size else 0.0
    return diff / top if top > 0.0 else diff


def bar(e_ref):
    return 2.0 * e_ref + 2.0 ** -23


def operator_arguments(c):
    """the keyword arguments of ops.ltx_guidance for a case (the latents and the average apart)"""
    return {"cfg": c["cfg"], "stg_scale": 0.0 if c["stg"] is None else c["stg"], "rescale": c["rescale"], "cfg_star": c["star"], "mode": c["mode"],
            "eta": c["eta"], "norm_threshold": c["threshold"], "momentum": c["momentum"], "want_negative": c["star"]}


# ---- csrc/vrg_guidance_math.hpp on the host --------------------------------------------------------------------------------------------------

def build_host_lib(directory, desc_type):
    out = os.path.join(str(directory), "libguidance_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "guidance_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    D = C.POINTER(desc_type)
    lib.hm_gd_check.argtypes, lib.hm_gd_check.restype = [D], C.c_int
    lib.hm_gd_scratch_bytes.argtypes, lib.hm_gd_scratch_bytes.restype = [D], C.c_int64
    lib.hm_gd_alpha.argtypes, lib.hm_gd_alpha.restype = [C.c_double, C.c_double], C.c_float
    lib.hm_gd_rows.argtypes, lib.hm_gd_rows.restype = [D, F32P, F32P, C.c_void_p, F32P, F32P], None
    lib.hm_gd_row_scalars.argtypes, lib.hm_gd_row_scalars.restype = [D, F64P, F32P, F64P], None
    lib.hm_gd_combine.argtypes, lib.hm_gd_combine.restype = [D, F32P, C.c_void_p, C.c_void_p, C.c_void_p, F32P, F32P, F64P, F32P, F32P], None
    lib.hm_gd_factor.argtypes, lib.hm_gd_factor.restype = [D] + [C.c_double] * 5, C.c_float
    lib.hm_gd_merge.argtypes, lib.hm_gd_merge.restype = [F64P, C.c_int64, F64P], None
    return lib


def _opt(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_step(lib, ops, c, p, n, q, average):
    """One step through the host-compiled header: the element-wise expressions and the derived scalars are the header's, every SUM is
    numpy's, in fp64.  Returns {"guided", "negative", "average"} as fp32 arrays (None where the step has none)."""
    p, n, q, average = (None if t is None else np.ascontiguousarray(t, dtype=np.float32) for t in (p, n, q, average))
    desc = ops.guidance_desc(p.shape, has_negative=n is not None, has_perturbed=q is not None, has_average=average is not None,
                             **{k: v for k, v in operator_arguments(c).items()})
    rows, batch = int(desc.rows), int(desc.batch)
    d = C.byref(desc)
    alpha = np.ones(batch, dtype=np.float32)
    if desc.cfg_star:
        p64, n64 = p.reshape(batch, -1).astype(np.float64), n.reshape(batch, -1).astype(np.float64)
        alpha = np.array([lib.hm_gd_alpha(float((p64[b] * n64[b]).sum()), float((n64[b] * n64[b]).sum())) for b in range(batch)], dtype=np.float32)
    scale, coef = np.ones(rows, dtype=np.float32), np.zeros(rows, dtype=np.float64)
    g = None
    if desc.has_negative and desc.mode == 1:
        g = np.empty_like(p)
        lib.hm_gd_rows(d, p, n, _opt(average if desc.has_average else None), alpha, g)
        g64, p64 = g.reshape(rows, -1).astype(np.float64), p.reshape(rows, -1).astype(np.float64)
        sums = np.ascontiguousarray(np.stack([(g64 * g64).sum(1), (p64 * p64).sum(1), (g64 * p64).sum(1)], axis=1))
        lib.hm_gd_row_scalars(d, sums, scale, coef)
    guided, n_out = np.empty_like(p), np.empty_like(p)
    lib.hm_gd_combine(d, p, _opt(n), _opt(q), _opt(g if desc.has_momentum else None), alpha, scale, coef, guided, n_out)
    if desc.has_rescale:
        p64, g64 = p.reshape(-1).astype(np.float64), guided.reshape(-1).astype(np.float64)
        mp, mg = p64.mean(), g64.mean()
        factor = lib.hm_gd_factor(d, float(p64.size), float(mp), float(((p64 - mp) ** 2).sum()), float(mg), float(((g64 - mg) ** 2).sum()))
        guided = guided * np.float32(factor)
    return {"guided": guided, "negative": n_out if desc.want_negative else None, "average": g if desc.has_momentum else None}

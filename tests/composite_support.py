"""Shared by tests/test_composite_host.py, tests/test_gpu_composite.py and tools/make_golden_composite.py: the recorded reference results
(tests/golden/composite.npz + .json) and csrc/vrg_composite_math.hpp compiled for the host."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "comfyui-vrgamedevgirl_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")

F32P = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
U32P = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
STATS_WORDS = 16
ULP1 = 2.0 ** -23


def meta():
    with open(os.path.join(GOLDEN, "composite.json")) as fh:
        return json.load(fh)


def arrays():
    return np.load(os.path.join(GOLDEN, "composite.npz"))


def build_host_lib(directory):
    out = os.path.join(str(directory), "libcomposite_check.so")
    src = os.path.join(ROOT, "tests", "host_math", "composite_check.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse", "-fPIC", "-shared",
           "-I", os.path.join(PKG_DIR, "csrc"), src, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_composite_linspace.argtypes = [C.c_int32, C.c_float, F32P]
    lib.hm_composite_linspace.restype = None
    lib.hm_composite_box.argtypes = [F32P, C.c_void_p, C.c_void_p, I32P, F32P, F32P]
    lib.hm_composite_box.restype = None
    lib.hm_composite_stats.argtypes = [F32P, F32P, C.c_void_p, C.c_void_p, C.c_int64, I32P, U32P]
    lib.hm_composite_stats.restype = None
    lib.hm_composite_apply.argtypes = [F32P, F32P, C.c_void_p, C.c_void_p, U32P, C.c_int64, I32P, F32P, F32P]
    lib.hm_composite_apply.restype = None
    return lib


def _f32c(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class HostCall:
    """One composite call on numpy arrays through the host arithmetic: the table comes from ops.composite_table, as in ops.composite_frames."""

    def __init__(self, lib, ops, originals, crops, entries, rule, color_match, user_mask=None):
        self.lib, self.ops = lib, ops
        self.originals, self.crops = _f32c(originals), _f32c(crops)
        self.user_mask = None if user_mask is None else _f32c(user_mask)
        self.frames = len(entries)
        self.nc = ops.composite_channels(rule, self.originals.shape[3], self.crops.shape[3])
        self.table, self.match, self.max_pixels = ops.composite_table(entries, rule, color_match, self.originals.shape[1], self.originals.shape[2])
        m = self.user_mask
        self.g10 = np.array([*self.crops.shape[1:4], *self.originals.shape[1:4], *((m.shape[1], m.shape[2], m.shape[3] if m.ndim == 4 else 1) if m is not None else (0, 0, 0)),
                             self.nc], dtype=np.int32)

    def _mask_ptr(self):
        return None if self.user_mask is None else self.user_mask.ctypes.data_as(C.c_void_p)

    def box(self, f):
        """(alpha [paste_h, paste_w], resampled crop [paste_h, paste_w, 4]) of output frame f"""
        d = self.table[f]
        alpha = np.zeros((d.paste_h, d.paste_w), dtype=np.float32)
        crop = np.zeros((d.paste_h, d.paste_w, 4), dtype=np.float32)
        self.lib.hm_composite_box(self.crops, self._mask_ptr(), C.cast(C.byref(d), C.c_void_p), self.g10, alpha, crop)
        return alpha, crop

    def stats(self):
        rec = np.zeros((max(1, self.frames), STATS_WORDS), dtype=np.uint32)
        self.lib.hm_composite_stats(self.crops, self.originals, self._mask_ptr(), C.cast(self.table, C.c_void_p), self.frames, self.g10, rec)
        return rec

    def truth_stats(self, selection=None):
        """The records with the means taken in numpy fp64 over the host arithmetic's resampled crop; `selection(f)` = the boolean
        [paste_h, paste_w] selection of frame f (the fixture's own mask > threshold), default the host arithmetic's alpha."""
        rec = np.zeros((max(1, self.frames), STATS_WORDS), dtype=np.uint32)
        f32 = rec.view(np.float32)
        for f in self.match:
            d = self.table[f]
            alpha, crop = self.box(f)
            sel = (alpha > np.float32(d.threshold)) if selection is None else selection(f)
            count = int(sel.sum())
            rec[f, 0], rec[f, 1] = count, int(count >= 16)
            if count == 0:
                continue
            target = self.originals[d.original_index, d.top:d.top + d.paste_h, d.left:d.left + d.paste_w, :self.nc]
            sm = crop[..., :self.nc][sel].astype(np.float64).mean(axis=0).astype(np.float32)
            dm = target[sel].astype(np.float64).mean(axis=0).astype(np.float32)
            f32[f, 2:2 + self.nc], f32[f, 6:6 + self.nc] = sm, dm
            if count >= 16:
                f32[f, 10:10 + self.nc] = ((dm - sm).astype(np.float32) * np.float32(d.match_strength)).astype(np.float32)
        return rec

    def apply(self, rec):
        out = np.empty((self.frames, *self.originals.shape[1:]), dtype=np.float32)
        mask = np.empty((self.frames, *self.originals.shape[1:3]), dtype=np.float32)
        self.lib.hm_composite_apply(self.crops, self.originals, self._mask_ptr(), C.cast(self.table, C.c_void_p), np.ascontiguousarray(rec),
                                    self.frames, self.g10, out, mask)
        return out, mask


def case_call(lib, ops, case, arr):
    """The HostCall of a fixture case and the inputs it was made from."""
    originals, crops = arr[case["key"] + ".originals"], arr[case["key"] + ".crops"]
    user_mask = arr[case["key"] + ".user_mask"] if case.get("user_mask") else None
    entries, rule, color_match = case_entries(ops, case, originals.shape[0], crops.shape[0], 0 if user_mask is None else user_mask.shape[0])
    return HostCall(lib, ops, originals, crops, entries, rule, color_match, user_mask)


def case_entries(ops, case, n_originals, n_crops, n_masks):
    if case["node"] == "paste":
        rule = ops.CompositeRule(case["blend_shape"], feather=case["feather_strength"], inset=case["inset_padding"])
        return ops.paste_back_entries(n_originals, n_crops, n_masks, case["crop_data"][1]), rule, case["color_match"]
    kind = "radial" if case["node"] == "facefix" else "opaque"
    rule = ops.CompositeRule(kind, feather=case["feather_pixels"])
    return ops.face_fix_entries(case["entries"], n_crops, case["offset"], n_originals), rule, case.get("color_match", 0.0)


def mismatches(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((got.view(np.uint32) != want.view(np.uint32)).sum())


def ulp_distance(a, b):
    """largest |a - b| in units of ulp(1.0)"""
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() / ULP1) if np.asarray(a).size else 0.0


def tie_margin(x64):
    """relative distance of the fp64 values from the nearest fp32 rounding tie (the midpoint of two neighbouring fp32 values)"""
    x64 = np.atleast_1d(np.asarray(x64, dtype=np.float64))
    lo = x64.astype(np.float32)
    other = np.where(lo.astype(np.float64) <= x64, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf)))
    mid = (lo.astype(np.float64) + other.astype(np.float64)) / 2.0
    return np.abs(x64 - mid) / np.maximum(np.abs(x64), 2.0 ** -126)

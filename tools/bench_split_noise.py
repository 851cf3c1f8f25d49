"""Long batch_size = 0 grain batches (an RNG chunk of more than 2^29 elements, which torch draws as several kernels): the split-noise route
against the route it replaces, alternated in one process, 7 rounds after 2 warm-up rounds -> profiles/split_noise.json.

    python tools/build_variant.py parent --unit vrg_chain.hip --source <the parent commit's csrc/vrg_chain.hip>
    python tools/bench_split_noise.py --old-lib tools/ab/lib_parent.so [--frames 91] [--host-frames 97] [--out profiles/split_noise.json]

"old" is the parent commit's route restated here, running on the parent's library: the chunk's noise written to HBM leaf by leaf
(vrg_noise_f32), applied with vrg_grain_injected_f32, the rest of a chain as a pass of its own; host-fed, the node uploads the whole batch
before the first kernel (one piece of `step` = all frames).  "new" is the package as it stands.  Rows: device-resident grain alone and
grain -> unsharp (time from HIP events, peak HBM above the input and output tensors), and FastFilmGrain(batch_size 0) on pageable host
frames with the result on the host (wall clock around the call and a synchronise, peak HBM)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

load_package()
from comfyui_vrgamedevgirl_amd import _devices as D, _hip, nodes, ops, rng  # noqa: E402

I, SAT = 0.04, 0.5


def old_film_grain(x, out=None):
    """the parent's ops._film_grain_oversize for one chunk (chunk_frames 0), from the default generator"""
    out = torch.empty_like(x) if out is None else out
    F, fe = x.shape[0], x[0].numel()
    lib = _hip.lib()
    st = _hip.current_stream()
    split = rng.reserve_split(F * fe, x.device)
    noise = torch.empty((F * fe,), dtype=torch.float32, device=x.device)
    for start, size, G, off in split.leaves:
        d = _hip.NoiseDesc(seed0=split.seed, seed_stride=0, offset0=off, offset_stride=0, chunk0=0, chunk_frames=1, grid_threads=G)
        _hip.check(lib.vrg_noise_f32(C.c_void_p(noise.data_ptr() + 4 * start), 1, size, C.byref(d), st), "vrg_noise_f32")
    _hip.check(lib.vrg_grain_injected_f32(_hip.ptr(x), _hip.ptr(noise), _hip.ptr(out), F * fe // 3, ops._f32(I), ops._f32(SAT), ops._f32(1.0 - SAT), st),
               "vrg_grain_injected_f32")
    return out


def old_grain_unsharp(x, out):
    return ops.fused_chain(old_film_grain(x), ops.ChainSpec(sharpen=("unsharp", 0.6, False)), out=out)


def new_film_grain(x, out):
    return ops.film_grain(x, I, SAT, chunk_frames=0, out=out)


def new_grain_unsharp(x, out):
    return ops.fused_chain(x, ops.ChainSpec(grain=(I, SAT, 0), sharpen=("unsharp", 0.6, False)), out=out)


def old_node(x):
    """the parent's FastFilmGrain.apply_grain for an oversize batch: no whole-batch reservation, pieces of `step` = all frames"""
    return nodes._run_grouped(x, lambda gpu, _first, out=None: old_film_grain(gpu, out), multiple_of=int(x.shape[0]))


def new_node(x):
    return nodes.FastFilmGrain().apply_grain(x, I, SAT, 0)[0]


def load_old_library(path):
    """the parent's library: bound like _hip.load_library, minus the entry points it does not have yet"""
    cdll = C.CDLL(path)
    for name, (res, args) in _hip._SIGNATURES.items():
        fn = getattr(cdll, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return _hip.Library(cdll, path)


def summary(values):
    return {"best": min(values), "median": statistics.median(values), "spread": max(values) - min(values), "all": values}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old-lib", required=True)
    ap.add_argument("--frames", type=int, default=91)
    ap.add_argument("--host-frames", type=int, default=97)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_noise.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    libs = {"new": _hip.lib(), "old": load_old_library(a.old_lib)}
    ops.toolchain_selfcheck(dev)

    def use(side):
        _hip._lib = libs[side]

    result = {"device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "warmup": a.warmup, "old_lib": os.path.basename(a.old_lib), "rows": {}}
    x = torch.rand((a.frames, a.height, a.width, 3), device=dev)
    out = torch.empty_like(x)
    assert x.numel() > rng.MAX_CHUNK_NUMEL
    for name, fns in (("device_resident_grain", {"old": lambda: old_film_grain(x, out), "new": lambda: new_film_grain(x, out)}),
                      ("device_resident_grain_unsharp", {"old": lambda: old_grain_unsharp(x, out), "new": lambda: new_grain_unsharp(x, out)})):
        ms, peak = {"old": [], "new": []}, {}
        results = {}
        for r in range(a.warmup + a.rounds):
            for side in ("old", "new"):
                use(side)
                torch.manual_seed(7)
                torch.cuda.synchronize(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[side]()
                e1.record()
                torch.cuda.synchronize(dev)
                if r >= a.warmup:
                    ms[side].append(e0.elapsed_time(e1))
                peak[side] = torch.cuda.max_memory_allocated(dev) - base
                if r == 0:
                    results[side] = out.clone()
        same = bool(torch.equal(results["old"], results["new"]))
        del results
        result["rows"][name] = {"frames": a.frames, "height": a.height, "width": a.width, "same_bits": same,
                                "old_ms": summary(ms["old"]), "new_ms": summary(ms["new"]),
                                "old_peak_bytes_above_in_out": peak["old"], "new_peak_bytes_above_in_out": peak["new"]}
        print(name, json.dumps({k: v for k, v in result["rows"][name].items() if not k.endswith("_ms")}),
              "old", result["rows"][name]["old_ms"]["median"], "new", result["rows"][name]["new_ms"]["median"], flush=True)
    del x, out
    torch.cuda.empty_cache()
    host = torch.rand((a.host_frames, a.height, a.width, 3))
    D.LAZY_SECONDS, D.DEFER_GRAPH, D.LAZY_DOWNLOAD = 60.0, False, False
    sec, peak, first = {"old": [], "new": []}, {}, {}
    for r in range(a.warmup + a.rounds):
        for side, fn in (("old", old_node), ("new", new_node)):
            use(side)
            torch.manual_seed(7)
            D._DEVICE_COPIES.clear()
            torch.cuda.synchronize(dev)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            t0 = time.perf_counter()
            got = fn(host)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                sec[side].append(dt)
            peak[side] = torch.cuda.max_memory_allocated(dev)
            if r == 0:
                first[side] = got[::16].clone()
            del got
    result["rows"]["host_fed_node"] = {"frames": a.host_frames, "height": a.height, "width": a.width,
                                       "same_bits_every_16th_frame": bool(torch.equal(first["old"], first["new"])),
                                       "old_s": summary(sec["old"]), "new_s": summary(sec["new"]),
                                       "old_peak_bytes": peak["old"], "new_peak_bytes": peak["new"]}
    print("host_fed_node old", result["rows"]["host_fed_node"]["old_s"]["median"], "new", result["rows"]["host_fed_node"]["new_s"]["median"],
          "peak", peak, flush=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Tensor-level operators over device-resident fp32 ``[F, H, W, C]`` frames.

Each function enqueues hand-written HIP kernels (libvrgdg_hip.so, C ABI in include/vrgdg_hip.h) on the
current torch HIP stream and returns a new tensor; inputs are never modified.  Scalars that the reference
computes in Python doubles are computed here in double and rounded to fp32 exactly once, as torch does
when a Python float meets an fp32 tensor.

PyTorch is used for device memory, streams and the generator state only -- there is no torch arithmetic
on the data path and no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import operator
import os
import threading
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _hip, rng

_F3 = C.c_float * 3

#: Arithmetic policy of the Lab transforms / statistics transfer (include/vrgdg_hip.h, enum vrg_cm_math).
#: "device" (default): each element-wise op is the one torch-ROCm runs for it on this GPU (bit-equal to the reference's
#: colour match executed on the MI355X, given the same statistics); "fast": table-driven powers, a few ulp away, 1.2-1.4x faster.
CM_MATH = {"device": _hip.CM_MATH_DEVICE, "fast": _hip.CM_MATH_FAST}


def default_cm_math() -> int:
    name = os.environ.get("VRGDG_CM_MATH", "device").strip().lower()
    if name not in CM_MATH:
        raise ValueError(f"VRGDG_CM_MATH must be one of {sorted(CM_MATH)}, got {name!r}")
    return CM_MATH[name]


def _cm_math(value) -> int:
    if value is None:
        return default_cm_math()
    if isinstance(value, str):
        return CM_MATH[value]
    return int(value)


#: Where the colour statistics come from.  "device" (default with the device arithmetic): torch-ROCm's own fp32 reductions replayed
#: bit for bit (csrc/vrg_torch_stats.hip) -- with it the whole colour match equals the reference run on this GPU; the value depends on
#: the node's batch_size like the reference's does.  "fp64": fp64-accumulated (n, mean, M2), rounded once -- closer to the exact
#: statistics than either reference, independent of batch_size, mergeable across GPUs (sharding.py), and what the fast policy uses.
CM_STATS = ("device", "fp64")


_NO_DEVICE_STATS_WARNED = set()
_STATE_LOCK = threading.RLock()     # re-entrant: HipEvent.__del__ takes it and may run in a GC pass triggered while it is held          # guards the small per-process caches below (first-use races between host threads)


def device_stats_supported(device) -> bool:
    """Can csrc/vrg_torch_stats.hip replay torch's reductions on this GPU?  torch's setReduceConfig takes another branch
    (force_splitting_output) on devices with fewer than 100 CUs -- e.g. one CPX partition of an MI355X; vrg_lab_stats_torch_f32 returns
    VRG_ERR_UNSUPPORTED there."""
    return torch.cuda.get_device_properties(device).multi_processor_count >= 100


def _cm_stats(value, cm_math, device=None) -> str:
    """Resolve the statistics policy.  An explicit value is taken as it is; the DEFAULT ("device" with the device arithmetic) falls
    back to "fp64" with a one-time warning on a GPU whose reduction geometry is not replayed (`device` given and unsupported)."""
    if value is None:
        value = os.environ.get("VRGDG_CM_STATS", "").strip().lower() or ("device" if _cm_math(cm_math) == _hip.CM_MATH_DEVICE else "fp64")
        if value == "device" and device is not None and torch.device(device).type == "cuda" and not device_stats_supported(device):
            key = torch.device(device).index
            with _STATE_LOCK:
                first = key not in _NO_DEVICE_STATS_WARNED
                _NO_DEVICE_STATS_WARNED.add(key)
            if first:
                import warnings
                warnings.warn(f"comfyui-vrgamedevgirl_amd: {torch.cuda.get_device_name(device)} reports "
                              f"{torch.cuda.get_device_properties(device).multi_processor_count} CUs; torch's reduction geometry is replayed for "
                              "devices with >= 100 CUs only -- colour statistics fall back to the fp64 form (a few ulp from the reference "
                              "run on this GPU instead of bit-equal to it)", RuntimeWarning)
            value = "fp64"
    if value not in CM_STATS:
        raise ValueError(f"cm_stats must be one of {CM_STATS}, got {value!r}")
    return value


def _on_device(fn):
    """Run `fn` with the device of its first tensor argument current: the kernels are enqueued on torch's current
    stream of the current device and the C side asks hipGetDevice(), so a tensor on cuda:1 while cuda:0 is current
    would otherwise get device-1 pointers on a device-0 stream."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        first = next((a for a in args if isinstance(a, torch.Tensor)), None)
        if first is None:
            first = next((a for a in kwargs.values() if isinstance(a, torch.Tensor)), None)
        if first is not None and first.is_cuda and first.device.index != torch.cuda.current_device():
            with torch.cuda.device(first.device):
                return fn(*args, **kwargs)
        return fn(*args, **kwargs)
    return wrapped


def _f32(v: float) -> float:
    """Python double -> nearest fp32 (as a Python float), the rounding torch applies to a scalar operand."""
    return float(np.float32(v))


def _check_frames(t: torch.Tensor, name="images", channels: Optional[int] = None, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or t.ndim != 4:
        raise ValueError(f"{name} must be a [frames, height, width, channels] tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {str(dtype).replace('torch.', '')}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (ops.* are device-resident; nodes.* move data for you)")
    if channels is not None and t.shape[-1] != channels:
        raise ValueError(f"{name} must have {channels} channels, got {t.shape[-1]}")
    return t if t.is_contiguous() else t.contiguous()


def _check_side(t: torch.Tensor, name: str, like: torch.Tensor, shape_tail=None, dtype=torch.float32):
    """A small device-resident operand of a kernel (statistics rows, LUT record table): the kernels read it through a raw
    pointer, so it must be contiguous, of the stated type and on the frames' GPU."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} tensor")
    if t.device != like.device:
        raise RuntimeError(f"{name} lives on {t.device}, the frames on {like.device}")
    if shape_tail is not None and tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"{name} must be shaped [n, {', '.join(str(v) for v in shape_tail)}], got {tuple(t.shape)}")
    return t


def _checked_out(out, shape, dtype, device, what: str, name: str = "out") -> torch.Tensor:
    """The destination of an operator: a fresh tensor of `shape`, `dtype` on `device`, or the caller's `out` -- the kernels write it
    through a raw pointer, so it must be a contiguous tensor of exactly that shape and type on that device (`name`: its argument)."""
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device
            or not out.is_contiguous()):
        raise ValueError(f"{what}: {name} must be a contiguous {str(dtype).replace('torch.', '')} {list(shape)} tensor on {device}")
    return out


def _disjoint(what: str, writes, reads) -> None:
    """The one overlap rule of the operators (include/vrgdg_hip.h, "Operands must not overlap"): the kernels take every operand through a
    `__restrict__` pointer and read pixels other than the one they store, so no operand that a call writes may share a byte with one it
    reads, or with another one it writes.  `writes` and `reads` are lists of (name, tensor or None): the checked, contiguous tensors
    that reach the kernels, as half-open byte ranges [data_ptr(), data_ptr() + nbytes).  Only operands in one address space are
    compared (both on the same device: what the operator uploads from the CPU itself cannot meet a resident operand); an empty
    tensor and None overlap nothing.  ValueError, naming the operator `what` and both operands, before anything is launched."""
    def spans(entries):
        return [(name, t.device, t.data_ptr(), t.data_ptr() + t.nbytes) for name, t in entries
                if isinstance(t, torch.Tensor) and t.device.type != "meta" and t.nbytes > 0]
    w, r = spans(writes), spans(reads)
    for i, (name, dev, lo, hi) in enumerate(w):
        for other, other_dev, other_lo, other_hi in r + w[i + 1:]:
            if dev == other_dev and lo < other_hi and other_lo < hi:
                raise ValueError(f"{what}: {name} must not alias {other} (bytes {max(lo, other_lo) - lo} .. {min(hi, other_hi) - lo} of {name} "
                                 f"lie inside {other}; the kernels read neighbours of what they write, so operands may not overlap)")


def _out_like(x: torch.Tensor, out: Optional[torch.Tensor], what: str, name: str = "the input frames") -> torch.Tensor:
    """_checked_out for a result shaped and typed like the (checked, contiguous) frames `x` (`name` in the message), which `out` must
    not overlap -- the stencils read neighbours of what they write."""
    out = _checked_out(out, x.shape, x.dtype, x.device, what)
    _disjoint(what, [("out", out)], [(name, x)])
    return out


def _placement(devices, what: str, noun: str, *, ring: bool, prefer: Optional[torch.device] = None) -> torch.device:
    """The GPU a call whose inputs live on `devices` (one torch.device per input, CPU ones included) runs on.  Inputs on two GPUs
    are refused under both rules; `what` names the operator and `noun` its inputs in the message.

    ring=False, the follow rule: CPU inputs follow the resident ones -- the operator uploads them itself with `.to(device)`, which
    reaches any GPU.  With nothing resident the call runs on `prefer` (the device of a resident `out`) or the compute device.

    ring=True, the ring rule: CPU inputs always go to the compute device, because `_devices.upload_frames` stages them through the
    page-locked ring, which uploads there and nowhere else (the grid and the sheet; the MSR frames and the first/last guide upload with
    `.to()` and simply inherited the rule).  Resident inputs on another GPU next to CPU ones are therefore refused, not moved."""
    from . import _devices
    on = [d for d in devices if d.type == "cuda"]
    if on and not (ring and len(on) < len(devices)):
        dev = on[0]
    else:
        dev = prefer if prefer is not None and not on else _devices.compute_device()
        if on and on[0] != dev:
            raise RuntimeError(f"{what}: CPU {noun} go to {dev}, the CUDA {noun} live on {on[0]}; move them there")
    if any(d != dev for d in on):
        raise RuntimeError(f"{what}: the {noun} live on more than one GPU")
    return dev


def _as_tensor(p):
    """A caller's numpy picture as a tensor over the same memory -- over a copy where the array is not contiguous or read-only (torch
    takes no read-only array) -- and a tensor detached; anything else as it is, for the caller's own refusal."""
    if isinstance(p, np.ndarray):
        p = torch.from_numpy(np.ascontiguousarray(p) if p.flags.writeable else np.array(p))                 # Pillow's arrays are read-only
    return p.detach() if isinstance(p, torch.Tensor) else p


def _byte_picture(p, what: str, *, allow_empty: bool) -> torch.Tensor:
    """One decoded picture (numpy array or tensor, never written) as a detached [height, width, 3] uint8 tensor"""
    p = _as_tensor(p)
    if (not isinstance(p, torch.Tensor) or p.dtype != torch.uint8 or p.ndim != 3 or int(p.shape[2]) != 3
            or not (allow_empty or min(int(v) for v in p.shape[:2]) >= 1)):
        raise ValueError(f"{what} must be a {'' if allow_empty else 'non-empty '}[height, width, 3] uint8 tensor or array")
    return p


def _refuse(rc: int, what: str, bad_arg: str, unsupported: str) -> None:
    """The return code of a host check (no device, so without the error strings _hip.check asks the library for) as the exception of
    the operator `what`: a ValueError for records that are wrong, a RuntimeError for a call that is larger than the kernels take."""
    if rc == _hip.VRG_ERR_BAD_ARG:
        raise ValueError(f"{what}: {bad_arg}")
    if rc != _hip.VRG_OK:
        raise RuntimeError(f"{what}: {unsupported}")


_upload_lock = threading.Lock()


def _uploaded(cache: dict, key, build, device, limit: int = 64) -> torch.Tensor:
    """``cache[key]``: on a miss the table of ``build()`` (a numpy array of records), uploaded to ``device`` as bytes.  A cache that holds ``limit``
    tables is cleared first: a handful of geometries per job; never grows without bound.  The table is marked as used on the caller's current stream:
    a cache cleared under another stream drops it while this caller's launch may still be queued, and the allocator then keeps the block
    until that launch is done."""
    t = cache.get(key)
    if t is None:
        t = _hip.upload_records(build(), device)
        with _upload_lock:
            if len(cache) >= limit:
                cache.clear()
            cache[key] = t
    if t.is_cuda:
        t.record_stream(torch.cuda.current_stream(t.device))
    return t


# ------------------------------------------------------------------------------------------------
# noise descriptors
# ------------------------------------------------------------------------------------------------

@dataclass
class NoisePlan:
    """How the frames of a call map onto torch.randn calls: `chunk_frames` frames per call."""
    chunk_frames: int
    stream: rng.ChunkedStream
    chunk0: int = 0

    def desc(self, chunk0: Optional[int] = None) -> _hip.NoiseDesc:
        s = self.stream
        return _hip.NoiseDesc(seed0=s.seed, seed_stride=s.seed_stride, offset0=s.offset0, offset_stride=s.offset_stride,
                              chunk0=self.chunk0 if chunk0 is None else chunk0, chunk_frames=self.chunk_frames,
                              grid_threads=s.grid_threads)


@dataclass
class SplitNoisePlan:
    """Frames [first, first + frames) of a run of RNG chunks of `chunk_frames` frames that torch itself splits (more than
    rng.MAX_CHUNK_NUMEL elements each, rng.reserve_split): chunk j of the run is call j of `stream`.  Counter-based noise needs no whole
    chunks: any range of whole frames is a plan (slice_plans), and a frame finds the leaves it meets (split_launches)."""
    chunk_frames: int
    stream: rng.SplitStream
    first: int = 0
    frames: int = 0


def oversize_chunks(frames: int, frame_numel: int, chunk_frames: int) -> bool:
    """Does the reference's chunk loop draw a torch.randn that ATen has to split (more than 2^29 elements)?"""
    step = min(chunk_frames if chunk_frames > 0 else frames, frames)
    return step * frame_numel > rng.MAX_CHUNK_NUMEL


def plan_noise(frames: int, frame_numel: int, chunk_frames: int, device, generator=None, geom=None):
    """Reserve the generator range FastFilmGrain's chunk loop would consume (nodes.py:46-51).
    Returns (plan for the full chunks or None, plan for the ragged tail chunk or None, n_full_chunks).  A chunk of more than
    rng.MAX_CHUNK_NUMEL elements (read now) is a draw torch splits: its plan is a SplitNoisePlan, and the generator moves as ATen moves it
    -- per chunk the outer call's unused reservation, then the leaves."""
    step = chunk_frames if chunk_frames > 0 else frames
    step = min(step, frames)
    n_full, tail = divmod(frames, step)
    limit = rng.MAX_CHUNK_NUMEL

    def plan(chunk, n):
        if chunk * frame_numel > limit:
            return SplitNoisePlan(chunk, rng.reserve_split(chunk * frame_numel, device, generator, geom, n_chunks=n), 0, chunk * n)
        return NoisePlan(chunk, rng.reserve(chunk * frame_numel, n, device, generator, geom))

    main = plan(step, n_full) if n_full else None
    tail_plan = plan(tail, 1) if tail else None
    return main, tail_plan, n_full


def _plan_frames(plan, n_chunks: int) -> int:
    return plan.frames if isinstance(plan, SplitNoisePlan) else n_chunks * plan.chunk_frames


def _plan_segments(plans, frames: int, what: str) -> list:
    """[(first frame, frames, plan)] of a call over `frames` frames under `plans` (plan_noise / slice_plans)"""
    main, tail, n_full = plans
    segments, done = [], 0
    for plan, n in ((main, n_full), (tail, 1)):
        if plan is not None:
            segments.append((done, _plan_frames(plan, n), plan))
            done += segments[-1][1]
    if done != frames and any(isinstance(p, SplitNoisePlan) for p in (main, tail)):       # (a slice of a split batch is any frame range)
        raise ValueError(f"{what}: the noise plans describe {done} frames, the call has {frames}")
    return segments


def split_launches(plan: SplitNoisePlan, frame_numel: int) -> list:
    """The launches of a split plan: [(first frame of the plan, frames, seed, leaves)], each inside one chunk and meeting at most
    rng.NOISE_LEAVES_MAX leaves -- `leaves` as rng.SplitStream.leaves_of gives them, relative to the launch's first element.  Halving stops
    at pieces of at most `limit` elements, so a leaf holds at least (limit + 1) // 2 and a frame of fewer than `limit` meets at most 3; a
    single frame that meets more than the maximum (more than 1.8 G elements at the real limit) comes back with leaves = None: that frame's
    noise is written to memory (_film_grain_oversize)."""
    out = []
    step, s = plan.chunk_frames, plan.stream
    f, end = plan.first, plan.first + plan.frames
    while f < end:
        chunk, lo = divmod(f, step)
        hi_max = min(step, lo + end - f)
        hi = lo + 1
        leaves = s.leaves_of(chunk, lo * frame_numel, hi * frame_numel)
        if len(leaves) > rng.NOISE_LEAVES_MAX:
            out.append((f - plan.first, 1, s.seed, None))
        else:
            while hi < hi_max:
                more = s.leaves_of(chunk, lo * frame_numel, (hi + 1) * frame_numel)
                if len(more) > rng.NOISE_LEAVES_MAX:
                    break
                hi, leaves = hi + 1, more
            out.append((f - plan.first, hi - lo, s.seed, leaves))
        f += hi - lo
    return out


def _split_records(plan, frame_numel: int):
    """[(first frame of the plan, frames, _hip.NoiseSplit)] for the launches of a split plan, [] for any other plan; None where a frame
    meets more leaves than a launch takes"""
    if not isinstance(plan, SplitNoisePlan):
        return []
    launches = split_launches(plan, frame_numel)
    if any(leaves is None for _g0, _n, _seed, leaves in launches):
        return None
    return [(g0, n, _hip.NoiseSplit.of(seed, leaves)) for g0, n, seed, leaves in launches]


def _slice_split_plans(plans, first_frame: int, frames: int):
    main, tail, n_full = plans
    main_len = _plan_frames(main, n_full) if main is not None else 0
    tail_len = _plan_frames(tail, 1) if tail is not None else 0
    end = first_frame + frames
    if first_frame < 0 or frames < 0 or end > main_len + tail_len:
        raise ValueError("a piece of a grain batch must lie inside the batch")
    sub_main, sub_n = None, 0
    if first_frame < main_len and frames:           # (main is a split plan: a split tail is shorter than its main chunk, which is then split too)
        n = min(end, main_len) - first_frame
        sub_main = SplitNoisePlan(main.chunk_frames, main.stream, main.first + first_frame, n)
        sub_n = (sub_main.first + n - 1) // main.chunk_frames - sub_main.first // main.chunk_frames + 1
    sub_tail = None
    lo = max(first_frame, main_len) - main_len
    if end - main_len > lo:
        if isinstance(tail, SplitNoisePlan):
            sub_tail = SplitNoisePlan(tail.chunk_frames, tail.stream, tail.first + lo, end - main_len - lo)
        elif lo != 0 or end - main_len != tail_len:
            raise ValueError("a piece of a grain batch must be made of whole noise chunks")
        else:
            sub_tail = tail
    return sub_main, sub_tail, sub_n


def slice_plans(plans, first_frame: int, frames: int):
    """The part of a whole-batch reservation (`plan_noise`) that covers frames [first_frame, first_frame + frames): what `plan_noise` would
    have returned for that piece had the pieces been reserved one after the other -- a batch's chunks are consecutive generator ranges, so
    reserving it at once (when the node is called) and slicing (when a piece runs) consumes the generator exactly as the reference's
    chunk loop does.  `first_frame` must be a multiple of the chunk size -- except under split plans (chunks torch itself splits), where
    any range of whole frames is a piece, across chunks too.  Touches no generator."""
    main, tail, n_full = plans
    if isinstance(main, SplitNoisePlan) or isinstance(tail, SplitNoisePlan):
        return _slice_split_plans(plans, first_frame, frames)
    step = main.chunk_frames if main is not None else (tail.chunk_frames if tail is not None else 1)
    full_end = n_full * step if main is not None else 0
    if first_frame % step and first_frame < full_end:
        raise ValueError("a piece of a grain batch must start on a noise chunk")
    end = first_frame + frames
    sub_main, sub_n = None, 0
    if main is not None and first_frame < full_end:
        sub_n = (min(end, full_end) - first_frame) // step
        if sub_n:
            sub_main = NoisePlan(step, main.stream, main.chunk0 + first_frame // step)
    covered = first_frame + sub_n * step if first_frame < full_end else first_frame
    sub_tail = None
    if covered < end:
        if tail is None or covered != full_end or end - covered != tail.chunk_frames:
            raise ValueError("a piece of a grain batch must be made of whole noise chunks")
        sub_tail = tail
    return sub_main, sub_tail, sub_n


# ------------------------------------------------------------------------------------------------
# grain
# ------------------------------------------------------------------------------------------------

def torch_stream_noise(frames: int, frame_numel: int, plan: NoisePlan, device) -> torch.Tensor:
    """The raw N(0,1) stream of `frames` frames under `plan` (test / debug entry)."""
    out = torch.empty((frames, frame_numel), dtype=torch.float32, device=device)
    d = plan.desc()
    _hip.check(_hip.lib().vrg_noise_f32(_hip.ptr(out), frames, frame_numel, C.byref(d), _hip.current_stream()), "vrg_noise_f32")
    return out


def _grain_call(x, out, f0, nf, plan: NoisePlan, I32, S32, T32):
    F, H, W, _ = x.shape
    fe = H * W * 3
    d = plan.desc()
    base_in = x.data_ptr() + f0 * fe * 4
    base_out = out.data_ptr() + f0 * fe * 4
    _hip.check(_hip.lib().vrg_grain_f32(C.c_void_p(base_in), C.c_void_p(base_out), nf, H, W, I32, S32, T32, C.byref(d),
                                       _hip.current_stream()), "vrg_grain_f32")


def _film_grain_oversize(x, out, f0, plan: SplitNoisePlan, I32, S32, T32):
    """RNG chunks beyond 2^29 elements (batch_size 0 or >= 22 4K / >= 87 1080p frames): torch runs such a randn as several
    kernels over 32-bit indexable sub-ranges ("leaves"), each with its own grid and generator offset (rng.reserve_split).  The
    leaves are not frame -- not even pixel -- aligned, so every element looks its leaf up in a table of at most eight that rides in the
    kernel arguments (vrg_grain_split_f32): one pass over frames [f0, f0 + plan.frames) of `x`, no noise in memory, one launch per group
    of frames that meets at most eight leaves.  A single frame that meets more (1.8 G elements at the real limit) has its noise
    written leaf by leaf with the stream kernel (bit-identical to torch.randn) and applied with the injected-noise grain kernel."""
    fe = x[0].numel()
    H, W = int(x.shape[1]), int(x.shape[2])
    lib = _hip.lib()
    for g0, nf, seed, leaves in split_launches(plan, fe):
        src = C.c_void_p(x.data_ptr() + 4 * (f0 + g0) * fe)
        dst = C.c_void_p(out.data_ptr() + 4 * (f0 + g0) * fe)
        if leaves is not None:
            rec = _hip.NoiseSplit.of(seed, leaves)
            _hip.check(lib.vrg_grain_split_f32(src, dst, nf, H, W, I32, S32, T32, C.byref(rec), _hip.current_stream()), "vrg_grain_split_f32")
            continue
        noise = torch.empty((fe,), dtype=torch.float32, device=x.device)
        chunk, lo = divmod(plan.first + g0, plan.chunk_frames)
        for start, size, G, off in plan.stream.leaves_of(chunk, lo * fe, (lo + 1) * fe):
            # the leaf's elements inside the frame: whole Philox calls of the leaf are drawn into a buffer of their own where the leaf
            # begins before the frame or ends behind it
            a, b = max(start, 0), min(start + size, fe)
            d = _hip.NoiseDesc(seed0=seed, seed_stride=0, offset0=off, offset_stride=0, chunk0=0, chunk_frames=1, grid_threads=G)
            if a == start and b == start + size:
                _hip.check(lib.vrg_noise_f32(C.c_void_p(noise.data_ptr() + 4 * start), 1, size, C.byref(d), _hip.current_stream()), "vrg_noise_f32")
            else:
                whole = torch.empty((size,), dtype=torch.float32, device=x.device)
                _hip.check(lib.vrg_noise_f32(_hip.ptr(whole), 1, size, C.byref(d), _hip.current_stream()), "vrg_noise_f32")
                noise[a:b] = whole[a - start:b - start]
        _hip.check(lib.vrg_grain_injected_f32(src, _hip.ptr(noise), dst, fe // 3, I32, S32, T32, _hip.current_stream()), "vrg_grain_injected_f32")
    return out


@_on_device
def film_grain(images: torch.Tensor, grain_intensity: float, saturation_mix: float, chunk_frames: int = 0,
               generator: Optional[torch.Generator] = None, plans=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Film grain with in-register Philox noise, bit-identical to the reference run on this GPU with the same
    generator state: chunks of `chunk_frames` frames each draw one ``torch.randn`` (0 = one draw for all)."""
    x = _check_frames(images, channels=3)
    F, H, W, _ = x.shape
    out = _out_like(x, out, "film_grain", "images")
    if F == 0:
        return out
    fe = H * W * 3
    if plans is None:
        plans = plan_noise(F, fe, chunk_frames, x.device, generator)
    I32, S32, T32 = _f32(grain_intensity), _f32(saturation_mix), _f32(1.0 - saturation_mix)
    for f0, nf, plan in _plan_segments(plans, F, "film_grain"):
        if isinstance(plan, SplitNoisePlan):
            _film_grain_oversize(x, out, f0, plan, I32, S32, T32)
        else:
            _grain_call(x, out, f0, nf, plan, I32, S32, T32)
    return out


@_on_device
def film_grain_seeded_frames(images: torch.Tensor, grain_intensity: float, saturation_mix: float, seed: int,
                             frame_start: int = 0) -> torch.Tensor:
    """Per-frame seeded grain: frame i uses generator seed (seed + frame_start + i) & 0x7FFFFFFF, offset 0
    (VRGDG_StandaloneVideoEnhancerNodes.py:262-278) -- independent of how frames are batched or sharded."""
    x = _check_frames(images, channels=3)
    F, H, W, _ = x.shape
    out = torch.empty_like(x)
    if F == 0 or grain_intensity <= 0:
        return x.clone() if F else out
    fe = H * W * 3
    I32, S32, T32 = _f32(grain_intensity), _f32(saturation_mix), _f32(1.0 - saturation_mix)
    first = int(seed) + int(frame_start)
    f = 0
    while f < F:   # split where the 31-bit mask wraps (practically never)
        s0 = (first + f) & 0x7FFFFFFF
        run = min(F - f, 0x80000000 - s0)
        plan = NoisePlan(1, rng.per_frame_seeded(fe, s0, x.device))
        _grain_call(x, out, f, run, plan, I32, S32, T32)
        f += run
    return out


@_on_device
def sharpen_then_seeded_grain(images: torch.Tensor, sharpen_strength: float, zero_border: bool, grain_intensity: float,
                              saturation_mix: float, seed: int, frame_start: int = 0) -> torch.Tensor:
    """Unsharp, then per-frame-seeded grain: the effect order of the stand-alone enhancer's _apply_effects_batch
    (VRGDG_StandaloneVideoEnhancerNodes.py:278-294) as ONE pass over the frames (vrg_sharpen_grain_f32: 24 B/px).  Frame sizes the
    fused kernel does not take (width not a multiple of 4 or below 344) run the two kernels; the result is the same bits either way
    (tests/test_gpu_parity.py::test_fused_sharpen_then_seeded_grain_equals_the_two_kernels)."""
    if isinstance(images, torch.Tensor) and images.dtype == torch.uint8:
        return _sharpen_then_seeded_grain_u8(images, sharpen_strength, zero_border, grain_intensity, saturation_mix, seed, frame_start)
    x = _check_frames(images, channels=3)
    F, H, W, _ = x.shape
    if F == 0 or sharpen_strength <= 0 or grain_intensity <= 0:
        y = stencil3x3(x, "unsharp", sharpen_strength, zero_border) if (F and sharpen_strength > 0) else x
        return film_grain_seeded_frames(y, grain_intensity, saturation_mix, seed, frame_start) if (F and grain_intensity > 0) else y
    fe = H * W * 3
    I32, S32, T32 = _f32(grain_intensity), _f32(saturation_mix), _f32(1.0 - saturation_mix)
    out = torch.empty_like(x)
    lib = _hip.lib()
    first = int(seed) + int(frame_start)
    f = 0
    while f < F:   # split where the 31-bit mask wraps (practically never)
        s0 = (first + f) & 0x7FFFFFFF
        run = min(F - f, 0x80000000 - s0)
        d = NoisePlan(1, rng.per_frame_seeded(fe, s0, x.device)).desc()
        st = lib.vrg_sharpen_grain_f32(C.c_void_p(x.data_ptr() + 4 * f * fe), C.c_void_p(out.data_ptr() + 4 * f * fe), run, H, W,
                                       _f32(sharpen_strength), _hip.BORDER_ZERO if zero_border else _hip.BORDER_REPLICATE, I32, S32, T32,
                                       C.byref(d), _hip.current_stream())
        if st == _hip.VRG_ERR_UNSUPPORTED:
            if f != 0:
                raise RuntimeError("vrg_sharpen_grain_f32 refused a later run of a batch it had accepted")
            return film_grain_seeded_frames(stencil3x3(x, "unsharp", sharpen_strength, zero_border), grain_intensity, saturation_mix,
                                            seed, frame_start)
        _hip.check(st, "vrg_sharpen_grain_f32")
        f += run
    return out


def _sharpen_then_seeded_grain_u8(frames_bgr, sharpen_strength, zero_border, grain_intensity, saturation_mix, seed, frame_start):
    """Decoded uint8 B,G,R frames in and out: ``_tensor_to_frames(_apply_effects_batch(_frames_to_tensor(frames)))`` of the enhancer's
    render loop (VRGDG_StandaloneVideoEnhancerNodes.py:417-421) as one kernel (vrg_sharpen_grain_u8, 3 + 3 B/px; any width, height and
    alignment since round 5).  A batch of fewer than four bytes, or a call with one of the two effects off, takes the converter -> fp32 ->
    converter route: the same bytes."""
    x = _check_frames(frames_bgr, "frames", channels=3, dtype=torch.uint8)
    F, H, W, _ = x.shape
    if F == 0:
        return x.clone()

    def through_fp32():
        y = frames_u8_to_f32(x)
        if sharpen_strength > 0:
            y = stencil3x3(y, "unsharp", sharpen_strength, zero_border)
        if grain_intensity > 0:
            y = film_grain_seeded_frames(y, grain_intensity, saturation_mix, seed, frame_start)
        return f32_to_frames_u8(y)

    if sharpen_strength <= 0 or grain_intensity <= 0:
        return through_fp32()
    fe = H * W * 3
    I32, S32, T32 = _f32(grain_intensity), _f32(saturation_mix), _f32(1.0 - saturation_mix)
    out = torch.empty_like(x)
    lib = _hip.lib()
    first = int(seed) + int(frame_start)
    f = 0
    while f < F:   # split where the 31-bit mask wraps (practically never)
        s0 = (first + f) & 0x7FFFFFFF
        run = min(F - f, 0x80000000 - s0)
        d = NoisePlan(1, rng.per_frame_seeded(fe, s0, x.device)).desc()
        st = lib.vrg_sharpen_grain_u8(C.c_void_p(x.data_ptr() + f * fe), C.c_void_p(out.data_ptr() + f * fe), run, H, W,
                                      _f32(sharpen_strength), _hip.BORDER_ZERO if zero_border else _hip.BORDER_REPLICATE, I32, S32, T32,
                                      C.byref(d), _hip.current_stream())
        if st == _hip.VRG_ERR_UNSUPPORTED:
            if f != 0:
                raise RuntimeError("vrg_sharpen_grain_u8 refused a later run of a batch it had accepted")
            return through_fp32()
        _hip.check(st, "vrg_sharpen_grain_u8")
        f += run
    return out


# ---------------------------------------------------------------------------------------------
# The stand-alone enhancer's upscale (cv2.resize(..., INTER_LANCZOS4) on decoded bytes, reference
# VRGDG_StandaloneVideoEnhancerNodes.py:213-230) and the upscale fused into sharpen -> grain
# ---------------------------------------------------------------------------------------------
LANCZOS_TAP_BYTES = C.sizeof(_hip.LzTap)          # one record of the table: int32 s, eight int16 weights
_host_lib = _hip.host_library   # the library for its HOST table functions (no GPU needed)


@functools.lru_cache(maxsize=512)
def pil_axis_table(number: int, n_in: int, n_out: int, box=None):
    """(ksize, one axis table as the kernels read it: bounds [n_out, 2] then weights [n_out, ksize], int32, read-only) of
    ``Image.resize(.., filter, box)``: ``n_out`` outputs from the source interval ``box`` = (in0, in1), as C floats, of an axis of ``n_in``
    pixels; ``number`` is Pillow's (1 LANCZOS, 3 BICUBIC).  Without a box: the whole axis under LANCZOS.  Host only, cached."""
    lib = _host_lib()
    if box is None:
        ksize = int(lib.vrg_pil_lanczos_ksize(n_in, n_out))
    else:
        ksize = int(lib.vrg_pil_filter_ksize(number, box[0], box[1], n_out))
    if n_in < 1 or n_out < 1 or ksize < 1:
        raise ValueError("pil_axis_table: sizes must be at least 1 and 0 <= in0 <= in1 <= n_in")
    table = np.zeros(n_out * (2 + ksize), dtype=np.int32)
    bounds, weights = C.c_void_p(table.ctypes.data), C.c_void_p(table[2 * n_out:].ctypes.data)
    if box is None:
        status = lib.vrg_pil_lanczos_table(n_in, n_out, bounds, weights)
    else:
        status = lib.vrg_pil_filter_table(number, n_in, box[0], box[1], n_out, bounds, weights)
    if status != _hip.VRG_OK:
        raise (ValueError if status == 1 else RuntimeError)(f"pil_axis_table: {lib.vrg_error_string(status).decode()}")
    table.setflags(write=False)
    return ksize, table


_lanczos_tables: dict = {}      # (in_h, in_w, out_h, out_w, device) -> the uploaded table


def lanczos4_taps(in_h: int, in_w: int, out_h: int, out_w: int) -> np.ndarray:
    """The table of the two Lanczos kernels, made on the host (no GPU needed): ``out_w`` column records then ``out_h`` row records as a
    structured array with fields ``s`` (floor of the source coordinate; the taps are s - 3 .. s + 4, clamped) and ``w`` (eight int16)."""
    in_h, in_w, out_h, out_w = int(in_h), int(in_w), int(out_h), int(out_w)
    if min(in_h, in_w, out_h, out_w) < 1:
        raise ValueError("lanczos4_taps: sizes must be at least 1")
    table = np.zeros(out_w + out_h, dtype=_hip.record_dtype(_hip.LzTap))
    _hip.check(_host_lib().vrg_lanczos4_taps(in_h, in_w, out_h, out_w, C.c_void_p(table.ctypes.data)), "vrg_lanczos4_taps")
    return table


def _lanczos_table(in_h, in_w, out_h, out_w, device) -> torch.Tensor:
    return _uploaded(_lanczos_tables, (in_h, in_w, out_h, out_w, str(device)), lambda: lanczos4_taps(in_h, in_w, out_h, out_w), device)


def _lanczos_sizes(x, out_w, out_h):
    out_w, out_h = int(out_w), int(out_h)
    if out_w < 1 or out_h < 1:
        raise ValueError("resize: output width and height must be at least 1")
    if x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("resize: frames must be at least 1 x 1")
    return out_w, out_h


@_on_device
def resize_frames_u8(frames_u8: torch.Tensor, out_w: int, out_h: int) -> torch.Tensor:
    """``cv2.resize(frame, (out_w, out_h), interpolation=cv2.INTER_LANCZOS4)`` on every frame of a ``[F,H,W,3]`` uint8 batch on the GPU
    (vrg_lanczos4_u8; the arithmetic is the restatement of csrc/vrg_lanczos_math.hpp).  Equal sizes hand the input back untouched, as the
    reference's _resize_frames does."""
    x = _check_frames(frames_u8, "frames", channels=3, dtype=torch.uint8)
    out_w, out_h = _lanczos_sizes(x, out_w, out_h)
    F, H, W, _ = x.shape
    if (W, H) == (out_w, out_h):
        return frames_u8
    out = torch.empty((F, out_h, out_w, 3), dtype=torch.uint8, device=x.device)
    if F == 0:
        return out
    taps = _lanczos_table(H, W, out_h, out_w, x.device)
    _hip.check(_hip.lib().vrg_lanczos4_u8(_hip.ptr(x), _hip.ptr(out), F, H, W, out_h, out_w, _hip.ptr(taps), _hip.current_stream()),
               "vrg_lanczos4_u8")
    return out


@_on_device
def upscale_sharpen_then_seeded_grain(frames_u8: torch.Tensor, out_w: int, out_h: int, strength: float, use_gpu: bool, intensity: float,
                                      saturation_mix: float, seed: int, frame_start: int = 0) -> torch.Tensor:
    """``sharpen_then_seeded_grain(resize_frames_u8(frames, out_w, out_h), ...)`` byte for byte, in ONE launch
    (vrg_upscale_sharpen_grain_u8): the upscaled frames never go to memory.  ``use_gpu`` selects the border of the unsharp as in the
    reference (True: avg_pool2d's zero padding, False: the numpy path's replicated edge).  Wherever the fused kernel refuses (vertical
    ratios below about 0.9), and for equal sizes, the two launches run."""
    x = _check_frames(frames_u8, "frames", channels=3, dtype=torch.uint8)
    out_w, out_h = _lanczos_sizes(x, out_w, out_h)
    F, H, W, _ = x.shape

    def two_launches():
        return sharpen_then_seeded_grain(resize_frames_u8(x, out_w, out_h), strength, bool(use_gpu), intensity, saturation_mix, seed, frame_start)

    if (W, H) == (out_w, out_h) or F == 0:
        return two_launches()
    fe_in, fe_out = H * W * 3, out_h * out_w * 3
    grain = intensity > 0
    I32, S32, T32 = _f32(intensity), _f32(saturation_mix), _f32(1.0 - saturation_mix)
    out = torch.empty((F, out_h, out_w, 3), dtype=torch.uint8, device=x.device)
    taps = _lanczos_table(H, W, out_h, out_w, x.device)
    lib = _hip.lib()
    first = int(seed) + int(frame_start)
    f = 0
    while f < F:   # split where the 31-bit mask wraps (practically never)
        s0 = (first + f) & 0x7FFFFFFF
        run = min(F - f, 0x80000000 - s0)
        d = NoisePlan(1, rng.per_frame_seeded(fe_out, s0, x.device)).desc() if grain else None
        st = lib.vrg_upscale_sharpen_grain_u8(C.c_void_p(x.data_ptr() + f * fe_in), C.c_void_p(out.data_ptr() + f * fe_out), run, H, W, out_h, out_w,
                                              _hip.ptr(taps), _f32(max(strength, 0.0)), _hip.BORDER_ZERO if use_gpu else _hip.BORDER_REPLICATE,
                                              I32 if grain else 0.0, S32, T32, C.byref(d) if grain else None, _hip.current_stream())
        if st == _hip.VRG_ERR_UNSUPPORTED:
            if f != 0:
                raise RuntimeError("vrg_upscale_sharpen_grain_u8 refused a later run of a batch it had accepted")
            return two_launches()
        _hip.check(st, "vrg_upscale_sharpen_grain_u8")
        f += run
    return out


@_on_device
def film_grain_injected(images: torch.Tensor, noise: torch.Tensor, grain_intensity: float, saturation_mix: float) -> torch.Tensor:
    """Grain arithmetic with caller-supplied N(0,1) noise (same shape): the noise-injection parity form."""
    x = _check_frames(images, channels=3)
    n = _check_frames(noise, "noise", channels=3)
    if n.shape != x.shape:
        raise ValueError("noise must have the shape of images")
    out = torch.empty_like(x)
    px = x.numel() // 3
    _hip.check(_hip.lib().vrg_grain_injected_f32(_hip.ptr(x), _hip.ptr(n), _hip.ptr(out), px, _f32(grain_intensity),
                                                _f32(saturation_mix), _f32(1.0 - saturation_mix), _hip.current_stream()),
               "vrg_grain_injected_f32")
    return out


# ------------------------------------------------------------------------------------------------
# 3D LUT
# ------------------------------------------------------------------------------------------------

@dataclass
class DeviceLut:
    table: torch.Tensor        # record table on the device: (N-1)^2 * N records of 12 fp32 (vrg_lut_prepare_f32)
    size: int                  # N
    domain_min: tuple
    domain_max: tuple
    nodes: Optional[torch.Tensor] = None   # the parsed [N,N,N,3] table itself on the device (ffmpeg-style lookup only)


def upload_lut(lut_data: dict, device) -> DeviceLut:
    """Upload a parsed .cube table ([N,N,N,3], index [b][g][r]) and rewrite it on the device into the
    cell-major form the kernels read (values copied verbatim)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is not None and device.index != torch.cuda.current_device():
        with torch.cuda.device(device):
            return upload_lut(lut_data, device)
    raw = lut_data["lut"].to(device=device, dtype=torch.float32).contiguous()
    if raw.ndim != 4 or raw.shape[-1] != 3 or not (raw.shape[0] == raw.shape[1] == raw.shape[2]):
        raise ValueError("LUT table must be [N, N, N, 3]")
    n = int(raw.shape[0])
    count = int(_hip.lib().vrg_lut_cells_floats(n))
    if count <= 0:
        raise ValueError(f"unsupported LUT size {n} (2..256)")
    cells = torch.empty((count,), dtype=torch.float32, device=device)
    _hip.check(_hip.lib().vrg_lut_prepare_f32(_hip.ptr(raw), n, _hip.ptr(cells), _hip.current_stream()), "vrg_lut_prepare_f32")
    dmin = tuple(float(v) for v in lut_data["domain_min"].to(torch.float32).cpu().tolist())
    dmax = tuple(float(v) for v in lut_data["domain_max"].to(torch.float32).cpu().tolist())
    return DeviceLut(cells, n, dmin, dmax, raw)


def blend_terms(strength: float):
    """(blend_mode, B, 1-B) from the node's 0..10 strength (VRGDG_IV_Adjustments.py:355-359).
    mode 0 = return the input, 1 = LUT only, 2 = x*(1-B) + y*B."""
    blend = max(0.0, min(10.0, float(strength))) / 10.0
    if blend <= 0.0:
        return 0, 0.0, 1.0
    if blend < 1.0:
        return 2, _f32(blend), _f32(1.0 - blend)
    return 1, 1.0, 0.0


@_on_device
def lut3d(image: torch.Tensor, lut: DeviceLut, strength: float = 10.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if image.ndim != 4 or image.shape[-1] < 3:
        raise ValueError("VRGDG_LUTS expects IMAGE input shaped like [batch, height, width, channels].")
    x = _check_frames(image, "image")
    mode, B, omB = blend_terms(strength)
    if mode == 0:
        if out is not None:
            _out_like(x, out, "lut3d", "image").copy_(x)
            return out
        return x
    _check_side(lut.table, "LUT record table", x)
    out = _out_like(x, out, "lut3d", "image")
    px = x.numel() // x.shape[-1]
    if px == 0:
        return out
    _hip.check(_hip.lib().vrg_lut3d_f32(_hip.ptr(x), _hip.ptr(out), px, x.shape[-1], _hip.ptr(lut.table), lut.size,
                                       _F3(*lut.domain_min), _F3(*lut.domain_max), mode, B, omB, _hip.current_stream()),
               "vrg_lut3d_f32")
    return out


@_on_device
def lut3d_ffmpeg_u8(frames_bgr: torch.Tensor, lut: DeviceLut, weights=None) -> torch.Tensor:
    """ffmpeg's ``lut3d`` (tetrahedral) and, with `weights` (one blend weight per frame), its ``blend`` expression
    ``A*(1-w)+B*w`` on decoded uint8 B,G,R frames: the per-pixel step of the reference's opening colour match as ffmpeg
    performs it.  Restated from ffmpeg's published sources, parity unpinned (csrc/vrg_lut_tetra.hip)."""
    x = _check_frames(frames_bgr, "frames", channels=3, dtype=torch.uint8)
    if lut.nodes is None:
        raise ValueError("this DeviceLut carries no node table (use ops.upload_lut)")
    _check_side(lut.nodes, "LUT node table", x)
    F, H, W, _ = x.shape
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    wt = None
    if weights is not None:
        wt = torch.tensor([float(w) for w in weights], dtype=torch.float64, device=x.device)
        if wt.numel() != F:
            raise ValueError(f"{wt.numel()} blend weights for {F} frames")
    _hip.check(_hip.lib().vrg_lut3d_tetra_u8(_hip.ptr(x), _hip.ptr(out), F, H * W, _hip.ptr(lut.nodes), lut.size,
                                            _F3(*lut.domain_min), _F3(*lut.domain_max), _hip.ptr(wt) if wt is not None else None,
                                            _hip.current_stream()), "vrg_lut3d_tetra_u8")
    return out


# ------------------------------------------------------------------------------------------------
# 3x3 stencils
# ------------------------------------------------------------------------------------------------

_STENCIL = {"unsharp": _hip.STENCIL_UNSHARP, "laplacian": _hip.STENCIL_LAPLACIAN, "sobel": _hip.STENCIL_SOBEL}


@_on_device
def stencil3x3(images: torch.Tensor, op: str, strength: float, zero_border: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """unsharp / laplacian / sobel.  zero_border=False is the reference's default numpy path (edge replicate);
    True is its ``use_gpu`` path (zero padding, and for laplacian/sobel the conv2d sign/epsilon conventions)."""
    x = _check_frames(images)
    out = _out_like(x, out, "stencil3x3", "images")
    F, H, W, Cn = x.shape
    if x.numel() == 0:
        return out
    _hip.check(_hip.lib().vrg_stencil3x3_f32(_hip.ptr(x), _hip.ptr(out), F, H, W, Cn, _STENCIL[op],
                                            _hip.BORDER_ZERO if zero_border else _hip.BORDER_REPLICATE, _f32(strength),
                                            _hip.current_stream()), "vrg_stencil3x3_f32")
    return out


# ------------------------------------------------------------------------------------------------
# frame resize / restore (Video Enhance: VRGDG_VideoEnhanceNodes.py:54-106, 394-419)
# ------------------------------------------------------------------------------------------------

FIT_STRETCH, FIT_CROP, FIT_LETTERBOX = "Stretch to dimensions", "Crop to fill", "Fit with letterbox (preserve all)"
#: the widget strings of `resize_method` -> F.interpolate mode; anything else is bicubic, as in the reference (:45-51)
INTERPOLATION = {"Nearest": "nearest", "Bilinear": "bilinear", "Bicubic (recommended)": "bicubic", "Area": "area"}
RESIZE_METHODS = {"bicubic": 0, "bilinear": 1, "area": 2, "nearest": 3}       # include/vrgdg_hip.h, enum vrg_resize_method


def interpolation_mode(resize_method) -> str:
    return INTERPOLATION.get(str(resize_method), "bicubic")


@dataclass(frozen=True)
class ResizeGeometry:
    """What one launch does: the `src` rectangle (x0, y0, w, h) of every input frame is resampled to the size of the `dst` rectangle and
    lands at its position in the [out_h, out_w] output frame; output pixels outside `dst` are zero (letterbox bars), and the part of `dst`
    outside the output frame is not produced (crop to fill: its resample positions are those of the whole scaled image)."""
    out_h: int
    out_w: int
    src: tuple
    dst: tuple


def resize_geometry(in_h: int, in_w: int, target_width, target_height, fit_mode) -> ResizeGeometry:
    """The integers of _resize_batch (:57-85), computed as the reference computes them (Python's round and //)."""
    source_height, source_width = int(in_h), int(in_w)
    target_width, target_height = int(target_width), int(target_height)
    src = (0, 0, source_width, source_height)
    if fit_mode == FIT_STRETCH:
        return ResizeGeometry(target_height, target_width, src, (0, 0, target_width, target_height))
    ratios = (target_width / source_width, target_height / source_height)
    scale = max(ratios) if fit_mode == FIT_CROP else min(ratios)
    scaled_width = max(1, int(round(source_width * scale)))
    scaled_height = max(1, int(round(source_height * scale)))
    if fit_mode == FIT_CROP:
        left = max(0, (scaled_width - target_width) // 2)
        top = max(0, (scaled_height - target_height) // 2)
        return ResizeGeometry(min(target_height, scaled_height - top), min(target_width, scaled_width - left), src,
                              (-left, -top, scaled_width, scaled_height))
    pad_left = max(0, (target_width - scaled_width) // 2)
    pad_right = max(0, target_width - scaled_width - pad_left)
    pad_top = max(0, (target_height - scaled_height) // 2)
    pad_bottom = max(0, target_height - scaled_height - pad_top)
    return ResizeGeometry(scaled_height + pad_top + pad_bottom, scaled_width + pad_left + pad_right, src,
                          (pad_left, pad_top, scaled_width, scaled_height))


def restore_geometry(work_h: int, work_w: int, source_width, source_height, fit_mode) -> ResizeGeometry:
    """The integers of _restore_batch (:89-106): the letterbox content rectangle is cut out again, then everything is a stretch."""
    working_height, working_width = int(work_h), int(work_w)
    source_width, source_height = int(source_width), int(source_height)
    dst = (0, 0, source_width, source_height)
    if fit_mode != FIT_LETTERBOX:
        return ResizeGeometry(source_height, source_width, (0, 0, working_width, working_height), dst)
    scale = min(working_width / source_width, working_height / source_height)
    content_width = min(working_width, max(1, int(round(source_width * scale))))
    content_height = min(working_height, max(1, int(round(source_height * scale))))
    left = max(0, (working_width - content_width) // 2)
    top = max(0, (working_height - content_height) // 2)
    return ResizeGeometry(source_height, source_width, (left, top, content_width, content_height), dst)


def _check_resize_source(t: torch.Tensor, name: str) -> torch.Tensor:
    t = _check_frames(t, name)
    if t.shape[0] < 1:
        raise ValueError("Video Enhance requires a non-empty IMAGE batch.")
    if t.shape[-1] < 3 or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError(f"{name} must have at least one pixel and 3 channels, got {tuple(t.shape)}")
    return t


def _geometry_args(x: torch.Tensor, g: ResizeGeometry):
    if g.out_h < 1 or g.out_w < 1:
        raise ValueError(f"resize to {g.out_w} x {g.out_h}: the target must have at least one pixel")
    return (int(x.shape[1]), int(x.shape[2]), int(x.shape[3]), *g.src, g.out_h, g.out_w, *g.dst)


@_on_device
def resize_geometry_frames(images: torch.Tensor, geometry: ResizeGeometry, resize_method, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RGB of `images` ([F, H, W, C >= 3]) resampled as `geometry` says, clamped to [0, 1]: [F, out_h, out_w, 3].  One launch."""
    x = _check_resize_source(images, "images")
    shape = (int(x.shape[0]), geometry.out_h, geometry.out_w, 3)
    args = _geometry_args(x, geometry)
    out = _checked_out(out, shape, torch.float32, x.device, "resize_geometry_frames")
    _disjoint("resize_geometry_frames", [("out", out)], [("images", x)])
    _hip.check(_hip.lib().vrg_resize_f32(_hip.ptr(x), _hip.ptr(out), shape[0], *args, RESIZE_METHODS[interpolation_mode(resize_method)],
                                        _hip.current_stream()), "vrg_resize_f32")
    return out


def resize_frames(images: torch.Tensor, target_width, target_height, fit_mode, resize_method, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """_resize_batch (:54-86) on device frames: stretch, crop to fill or letterbox to the target size."""
    x = _check_resize_source(images, "images")
    return resize_geometry_frames(x, resize_geometry(x.shape[1], x.shape[2], target_width, target_height, fit_mode), resize_method, out)


def _check_frame_indices(indices, frames: int) -> list:
    try:
        listed = [int(i) for i in indices]
    except TypeError:
        raise ValueError(f"indices must be a sequence of frame numbers or None, got {type(indices).__name__}") from None
    for i in listed:
        if not 0 <= i < frames:
            raise ValueError(f"frame index {i} is outside the batch of {frames} frame(s)")
    return listed


@_on_device
def prepare_frames(images: torch.Tensor, geometry: ResizeGeometry, resize_method, indices=None, want_f32: bool = True, want_u8: bool = True):
    """The pixels of VRGDGVideoEnhancePrepare.prepare (:224-228) in one launch: frame i of the result is `images[indices[i]]` (every frame in
    order for None; repeats and any order are fine) resampled as resize_geometry_frames does, bit for bit -- as float32
    [N, out_h, out_w, 3] and/or as the uint8 R,G,B bytes ``(x * 255).round().astype("uint8")`` of _save_image_batch (:117).  Returns
    (f32 | None, u8 | None).  The index list is checked here, before anything is launched."""
    x = _check_resize_source(images, "images")
    if not (want_f32 or want_u8):
        raise ValueError("prepare_frames: at least one of want_f32 and want_u8 must be set")
    frames = int(x.shape[0])
    args = _geometry_args(x, geometry)
    listed = None if indices is None else _check_frame_indices(indices, frames)
    n_out = frames if listed is None else len(listed)
    shape = (n_out, geometry.out_h, geometry.out_w, 3)
    f32 = torch.empty(shape, dtype=torch.float32, device=x.device) if want_f32 else None
    u8 = torch.empty(shape, dtype=torch.uint8, device=x.device) if want_u8 else None
    if n_out == 0:
        return f32, u8
    index = None if listed is None else torch.tensor(listed, dtype=torch.int32).to(x.device)
    null = C.c_void_p(0)
    _hip.check(_hip.lib().vrg_prepare_frames_f32(_hip.ptr(x), frames, *args[:3], null if index is None else _hip.ptr(index), n_out, *args[3:],
                                                RESIZE_METHODS[interpolation_mode(resize_method)], null if f32 is None else _hip.ptr(f32),
                                                null if u8 is None else _hip.ptr(u8), _hip.current_stream()), "vrg_prepare_frames_f32")
    return f32, u8


@_on_device
def restore_frames(work: torch.Tensor, originals: torch.Tensor, source_width, source_height, fit_mode, resize_method, strength: float,
                   frame_count: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """VRGDGVideoEnhanceRestoreOriginal.restore (:404-419) in one pass over the originals: the working-resolution frames `work` go back to
    the source size (_restore_batch), are blended over the RGB of the first min(frame_count, len(work)) `originals` as
    o * (1 - strength) + restored * strength, and everything -- further channels and the unmatched tail frames of the originals
    included -- is clamped to [0, 1].  Shaped like `originals`."""
    w = _check_resize_source(work, "work")
    o = _check_frames(originals, "originals")
    if o.device != w.device:
        raise RuntimeError(f"originals live on {o.device}, the working frames on {w.device}")
    if o.shape[-1] < 3:
        raise ValueError(f"originals must have at least 3 channels, got {o.shape[-1]}")
    g = restore_geometry(w.shape[1], w.shape[2], source_width, source_height, fit_mode)
    if (g.out_h, g.out_w) != (int(o.shape[1]), int(o.shape[2])):
        raise ValueError(f"originals are {int(o.shape[2])} x {int(o.shape[1])}, the restore target is {g.out_w} x {g.out_h}")
    frames = int(o.shape[0])
    usable = min(frames if frame_count is None else int(frame_count), int(w.shape[0]))
    if usable > frames:
        raise ValueError(f"{usable} restored frames for {frames} original frames")
    out = _out_like(o, out, "restore_frames", "originals")
    _disjoint("restore_frames", [("out", out)], [("work", w)])
    if o.numel() == 0:
        return out
    strength = float(strength)
    _hip.check(_hip.lib().vrg_restore_f32(_hip.ptr(w), _hip.ptr(o), _hip.ptr(out), max(0, usable), frames, *_geometry_args(w, g),
                                         int(o.shape[3]), RESIZE_METHODS[interpolation_mode(resize_method)], _f32(strength),
                                         _f32(1.0 - strength), _hip.current_stream()), "vrg_restore_f32")
    return out


# ------------------------------------------------------------------------------------------------
# feathered crop composite (Image Paste Back: VRGDG_ImagePasteBack.py:11-41, 209-262; Face Fix composite and its opaque twin:
# VRGDG_StandaloneFaceFixNodes.py:811-854, 874-919)
# ------------------------------------------------------------------------------------------------

COMPOSITE_RULES = {"ellipse": _hip.COMPOSITE_ELLIPSE, "rectangle": _hip.COMPOSITE_RECTANGLE, "radial": _hip.COMPOSITE_RADIAL,
                   "opaque": _hip.COMPOSITE_OPAQUE}
PASTE_BACK_THRESHOLD, FACE_FIX_THRESHOLD = 0.25, 0.35


@dataclass(frozen=True)
class CompositeRule:
    """Which alpha the composite uses and its widgets: kind "ellipse" / "rectangle" (Paste Back: `inset`, `feather`), "radial" (Face Fix:
    `feather`, alpha times the entry's strength) or "opaque" (Face Fix Opaque: `feather` = the edge width)."""
    kind: str
    feather: float = 0
    inset: float = 0


def _linspace_step(n: int) -> float:
    """torch.linspace(-1, 1, n) in fp32: (1 - -1) / (n - 1), one fp32 division (csrc/vrg_composite_math.hpp cp_linspace)"""
    return float(np.float32(2.0) / np.float32(n - 1)) if n > 1 else 0.0


def composite_table(entries, rule: CompositeRule, color_match, height: int, width: int):
    """The descriptor table of one composite call, from Python numbers exactly as the reference computes its rectangles and constants.
    `entries`: one dict per OUTPUT frame -- "original", "crop" (frame indices), optional "mask" (frame of the user mask), "box" =
    (left, top, right, bottom) or None (frame returned clamped, mask zero), "strength" (radial: the alpha factor).  Returns
    (ctypes array of _hip.CompositeDesc, list of the frames to measure, largest pasted region in pixels)."""
    if rule.kind not in COMPOSITE_RULES:
        raise ValueError(f"composite rule must be one of {sorted(COMPOSITE_RULES)}, got {rule.kind!r}")
    height, width = int(height), int(width)
    paste = rule.kind in ("ellipse", "rectangle")
    color_match = float(color_match)
    table = (_hip.CompositeDesc * max(1, len(entries)))()
    match, max_pixels = [], 0
    for f, entry in enumerate(entries):
        d = table[f]
        d.rule, d.original_index, d.crop_index, d.mask_index = _hip.COMPOSITE_NONE, int(entry["original"]), int(entry.get("crop", 0)), -1
        box = entry.get("box")
        if not box:
            continue
        left, top, right, bottom = (int(v) for v in box)
        box_w, box_h = right - left, bottom - top
        if paste:
            # paste_back (:215-230): the rectangle is cut at the right / bottom edge; a negative corner would be Python's negative slicing
            if box_w <= 0 or box_h <= 0:
                raise ValueError(f"Invalid crop rectangle in CROP_DATA: {tuple(box)!r}")
            if left < 0 or top < 0:
                raise ValueError(f"CROP_DATA {tuple(box)!r} has a negative corner: the reference slices from the far edge there, which is not "
                                 "a defined paste; refused")
            left, top = min(left, width), min(top, height)
            paste_w, paste_h = min(left + box_w, width) - left, min(top + box_h, height) - top
            if paste_w <= 0 or paste_h <= 0:
                d.flags = _hip.COMPOSITE_RAW_COPY                       # :233-236: the original is returned as it is, not clamped
                continue
            inset = max(0.0, min(float(rule.inset), (min(box_w, box_h) - 1) / 2.0))
            if rule.kind == "ellipse":
                cx, cy = (box_w - 1) / 2.0, (box_h - 1) / 2.0
                rx, ry = max(0.5, cx - inset), max(0.5, cy - inset)
                consts = (cx, cy, rx, ry, min(rx, ry))
            else:
                consts = (inset, box_w - 1 - inset, box_h - 1 - inset, 0.0, 0.0)
            step = rule.feather <= 0
            consts += (1.0 if step else float(rule.feather),)
            flags = _hip.COMPOSITE_STEP if step else 0
            if entry.get("mask") is not None:
                flags |= _hip.COMPOSITE_USER_MASK
                d.mask_index = int(entry["mask"])
            threshold = PASTE_BACK_THRESHOLD
        else:
            if rule.kind == "radial" and float(entry.get("strength", 0.0)) <= 0:
                continue                                                # the no-face decision comes first (:830): whatever the box says
            if box_w <= 0 or box_h <= 0:
                if rule.kind == "opaque":
                    continue                                            # the opaque node skips an empty box (:897)
                raise ValueError(f"Face Fix box {tuple(box)!r} is empty: the reference fails on it; refused")
            if left < 0 or top < 0 or right > width or bottom > height:
                raise ValueError(f"Face Fix box {tuple(box)!r} does not lie inside the {width} x {height} frame: the reference fails on a "
                                 "shape mismatch there; refused")
            paste_w, paste_h = box_w, box_h
            flags = _hip.COMPOSITE_CLAMP_CROP
            if rule.kind == "radial":
                strength = float(entry.get("strength", 0.0))
                feather_scale = max(1.0, float(rule.feather) / max(1.0, min(box_w, box_h) / 2.0))
                consts = (_linspace_step(box_w), _linspace_step(box_h), feather_scale, strength)
            else:
                feather = max(0, int(rule.feather))
                edge = min(1.0, (2.0 * feather) / max(1.0, float(min(box_w, box_h))))
                if edge <= 0:
                    flags |= _hip.COMPOSITE_STEP
                consts = (_linspace_step(box_w), _linspace_step(box_h), edge if edge > 0 else 1.0)
            threshold = FACE_FIX_THRESHOLD
        if color_match > 0 and rule.kind != "opaque":
            flags |= _hip.COMPOSITE_MATCH
            match.append(f)
        d.rule, d.flags = COMPOSITE_RULES[rule.kind], flags
        d.left, d.top, d.box_w, d.box_h, d.paste_w, d.paste_h = left, top, box_w, box_h, paste_w, paste_h
        d.match_strength, d.threshold = _f32(color_match), _f32(threshold)
        for i, v in enumerate(consts):
            d.p[i] = _f32(v)
        max_pixels = max(max_pixels, paste_w * paste_h)
    return table, match, max_pixels


def paste_back_entries(n_originals: int, n_crops: int, n_masks: int, box) -> list:
    """The output frames of paste_back (:221-225, _batch_item): as many as the longest input, each reading frame min(index, n - 1) of the
    shorter ones.  `box` = (x, y, right_edge, bottom_edge) of CROP_DATA; n_masks = 0 without a user mask."""
    frames = max(int(n_originals), int(n_crops), int(n_masks) if n_masks else 1)
    return [{"original": min(i, n_originals - 1), "crop": min(i, n_crops - 1), "mask": min(i, n_masks - 1) if n_masks else None,
             "box": tuple(int(v) for v in box)} for i in range(frames)]


def face_fix_entries(entries, n_work: int, offset: int, n_originals: int, first_frame: int = 0, last_frame: Optional[int] = None) -> list:
    """The output frames [first_frame, last_frame) of the Face Fix composites (:826-834, :887-899): source frame i takes work frame
    i + offset while i < usable = min(len(entries), max(0, n_work - offset)); everything else is returned clamped.  "original" counts
    from first_frame (the frames may be a piece of the batch), "strength" as the reference reads it (missing = 0)."""
    usable = min(len(entries), max(0, int(n_work) - int(offset)))
    last_frame = int(n_originals) if last_frame is None else int(last_frame)
    rows = []
    for i in range(int(first_frame), last_frame):
        box = entries[i].get("box") if i < usable else None
        rows.append({"original": i - int(first_frame), "crop": i + int(offset) if box else 0, "box": tuple(box) if box else None,
                     "strength": float(entries[i].get("strength", 0.0)) if box else 0.0})
    return rows


def composite_channels(rule: CompositeRule, original_channels: int, crop_channels: int) -> int:
    """How many channels are composited: Paste Back blends the channels both images have (:241, :255), the Face Fix nodes RGB."""
    if int(original_channels) not in (3, 4):
        raise ValueError(f"the composite is defined for 3 or 4 channels, the originals have {int(original_channels)}; refused")
    if int(crop_channels) not in (3, 4):
        raise ValueError(f"the composite is defined for 3 or 4 channels, the crop has {int(crop_channels)}; refused")
    return min(int(original_channels), int(crop_channels)) if rule.kind in ("ellipse", "rectangle") else 3


def _composite_prepare(originals, crops, entries, rule, color_match, user_mask):
    o = _check_frames(originals, "originals")
    c = _check_frames(crops, "crops")
    if c.device != o.device:
        raise RuntimeError(f"crops live on {c.device}, the originals on {o.device}")
    if o.shape[0] < 1 or c.shape[0] < 1 or min(o.shape[1], o.shape[2], c.shape[1], c.shape[2]) < 1:
        raise ValueError("the composite needs at least one original and one crop frame of at least one pixel")
    nc = composite_channels(rule, o.shape[3], c.shape[3])
    mask_h = mask_w = mask_stride = n_mask = 0
    m = None
    if user_mask is not None:
        m = user_mask
        if not isinstance(m, torch.Tensor) or m.ndim not in (3, 4) or m.dtype != torch.float32 or m.device != o.device:
            raise ValueError("user_mask must be a float32 [frames, height, width] (or [..., channels]) tensor on the originals' device")
        m = m if m.is_contiguous() else m.contiguous()
        n_mask, mask_h, mask_w = int(m.shape[0]), int(m.shape[1]), int(m.shape[2])
        mask_stride = int(m.shape[3]) if m.ndim == 4 else 1
        if min(n_mask, mask_h, mask_w, mask_stride) < 1:
            raise ValueError("user_mask must not be empty")
    table, match, max_pixels = composite_table(entries, rule, color_match, o.shape[1], o.shape[2])
    frames = len(entries)
    for f in range(frames):
        d = table[f]
        if not 0 <= d.original_index < o.shape[0] or not 0 <= d.crop_index < c.shape[0]:
            raise ValueError(f"entry {f} names original {d.original_index} / crop {d.crop_index} of {int(o.shape[0])} / {int(c.shape[0])}")
        if d.flags & _hip.COMPOSITE_USER_MASK and not 0 <= d.mask_index < n_mask:
            raise ValueError(f"entry {f} names frame {d.mask_index} of a user mask of {n_mask}")
    # one upload: the records, then the list of frames to measure
    dev_table = _hip.upload_records(table, o.device, frames, [np.asarray(match if frames else [0], dtype=np.int32)])  # never empty
    geom = (frames, int(o.shape[0]), int(c.shape[0]), n_mask, int(c.shape[1]), int(c.shape[2]), int(c.shape[3]), int(o.shape[1]),
            int(o.shape[2]), int(o.shape[3]), mask_h, mask_w, mask_stride, nc)
    stats = torch.zeros((max(frames, 1), _hip.COMPOSITE_STATS_WORDS), dtype=torch.int32, device=o.device)
    return o, c, m, dev_table, match, max_pixels, geom, stats


def _composite_measure(o, c, m, dev_table, match, max_pixels, geom, stats):
    if not match:
        return
    lib = _hip.lib()
    scratch = torch.empty(int(lib.vrg_composite_scratch_bytes(len(match), max_pixels)), dtype=torch.uint8, device=o.device)
    match_ptr = C.c_void_p(dev_table.data_ptr() + geom[0] * C.sizeof(_hip.CompositeDesc))
    _hip.check(lib.vrg_composite_stats_f32(_hip.ptr(c), _hip.ptr(o), _hip.ptr(m) if m is not None else None, _hip.ptr(dev_table), match_ptr,
                                           len(match), max_pixels, *geom, _hip.ptr(scratch), _hip.ptr(stats), _hip.current_stream()),
               "vrg_composite_stats_f32")


def _stats_record(stats: torch.Tensor, frames: int) -> dict:
    words = stats[:frames]
    f32 = words.view(torch.float32)
    return {"count": words[:, 0], "matched": words[:, 1], "crop_mean": f32[:, 2:6], "original_mean": f32[:, 6:10], "shift": f32[:, 10:14]}


@_on_device
def composite_stats(originals: torch.Tensor, crops: torch.Tensor, entries, rule: CompositeRule, color_match, user_mask=None) -> dict:
    """What the colour match of composite_frames measures, per output frame, as device tensors: "count" (selected pixels, int32),
    "matched" (count >= 16), "crop_mean" / "original_mean" ([frames, 4] fp32, fp64-accumulated) and "shift".  Zero for frames that are not
    measured (no box, strength 0, the opaque rule)."""
    prepared = _composite_prepare(originals, crops, entries, rule, color_match, user_mask)
    _composite_measure(*prepared)
    return _stats_record(prepared[-1], len(entries))


@_on_device
def composite_frames(originals: torch.Tensor, crops: torch.Tensor, entries, rule: CompositeRule, color_match=0.0, user_mask=None,
                     out: Optional[torch.Tensor] = None, mask_out: Optional[torch.Tensor] = None):
    """The feathered crop composite on device frames: for every entry (see composite_table) the crop is bicubic-resized to its box, blended
    over the original under the rule's alpha (times the bilinear-resized, clamped `user_mask`), after the mean-shift colour match when
    color_match > 0 and at least 16 pixels have alpha above the threshold -- decided on the device, no host synchronisation.  Returns
    (frames [len(entries), H, W, C] clamped to [0, 1], masks [len(entries), H, W]).  Two measuring launches (only for frames that ask for
    a match) and one pass over the output."""
    o, c, m, dev_table, match, max_pixels, geom, stats = _composite_prepare(originals, crops, entries, rule, color_match, user_mask)
    frames = len(entries)
    shape = (frames, int(o.shape[1]), int(o.shape[2]), int(o.shape[3]))
    out = _checked_out(out, shape, torch.float32, o.device, "composite_frames")
    mask_out = _checked_out(mask_out, shape[:3], torch.float32, o.device, "composite_frames", "mask_out")
    _disjoint("composite_frames", [("out", out), ("mask_out", mask_out)], [("originals", o), ("crops", c), ("user_mask", m)])
    if frames == 0:
        return out, mask_out
    _composite_measure(o, c, m, dev_table, match, max_pixels, geom, stats)
    _hip.check(_hip.lib().vrg_composite_apply_f32(_hip.ptr(c), _hip.ptr(o), _hip.ptr(m) if m is not None else None, _hip.ptr(dev_table),
                                                 _hip.ptr(stats), _hip.ptr(out), _hip.ptr(mask_out), *geom, _hip.current_stream()),
               "vrg_composite_apply_f32")
    return out, mask_out


# ------------------------------------------------------------------------------------------------
# landmark-aligned Face Fix composite (VRGDG_StandaloneFaceFixNodes.py:1015-1054): the face as bytes, cv2's byte Lanczos-4 affine warp
# (csrc/vrg_warp_math.hpp), the warp fused into the composite pass
# ------------------------------------------------------------------------------------------------
_warp_host_table = None
_warp_tables: dict = {}          # device -> the uploaded phase table


def warp_phase_table() -> np.ndarray:
    """The 1024 x 8 x 8 int16 weights of the warp (phase = fy * 32 + fx, tap row, tap column), made on the host once (no GPU needed);
    every phase sums to exactly 32768.  Read-only."""
    global _warp_host_table
    if _warp_host_table is None:
        table = np.zeros((1024, 8, 8), dtype=np.int16)
        _hip.check(_host_lib().vrg_warp_phase_table(C.c_void_p(table.ctypes.data)), "vrg_warp_phase_table")
        table.setflags(write=False)
        _warp_host_table = table
    return _warp_host_table


def _warp_table(device) -> torch.Tensor:
    return _uploaded(_warp_tables, str(device), warp_phase_table, device)


def _box_size(box):
    """(w, h) of a box with area, else None"""
    if not box:
        return None
    left, top, right, bottom = (int(v) for v in box)
    return (right - left, bottom - top) if right > left and bottom > top else None


def _pack_offsets(boxes):
    """Where each box's [h][w][3] byte image starts in the packed buffer (16-byte steps; -1 = no image), and the buffer's size."""
    offsets, total = [], 0
    for box in boxes:
        size = _box_size(box)
        if size is None:
            offsets.append(-1)
            continue
        offsets.append(total)
        total += (size[0] * size[1] * 3 + 15) // 16 * 16
    return offsets, total


def _warp_record_table(transforms, sizes, sources, offsets):
    """ctypes array of _hip.WarpDesc: result size sizes[f], source image sources[f] = (w, h) at offsets[f]; transforms[f] None = not set"""
    n = len(transforms)
    table = (_hip.WarpDesc * max(1, n))()
    lib = _host_lib()
    for f, t in enumerate(transforms):
        if t is None or sizes[f] is None or offsets[f] < 0:
            continue
        m = np.ascontiguousarray(np.asarray(t, dtype=np.float32).reshape(-1))
        if m.size != 6:
            raise ValueError(f"transform {f} must be a 2 x 3 matrix, got shape {np.asarray(t).shape}")
        if not np.isfinite(m).all():
            raise ValueError(f"transform {f} has a non-finite entry: cv2.warpAffine leaves that undefined; refused")
        status = lib.vrg_warp_record(C.c_void_p(m.ctypes.data), sizes[f][0], sizes[f][1], sources[f][0], sources[f][1], offsets[f],
                                     C.cast(C.byref(table[f]), C.c_void_p))
        if status != _hip.VRG_OK:
            raise ValueError(f"transform {f} scales a coordinate of its {sizes[f][0]} x {sizes[f][1]} box past the 32-bit fixed point of "
                             "cv2.warpAffine, which leaves that undefined; refused")
    return table


def warp_records(transforms, boxes):
    """The warp records of one composite call, made on the host (no GPU needed): transforms[f] = the forward 2 x 3 matrix warpAffine takes
    (or None: the frame keeps its bicubic face), boxes[f] = (left, top, right, bottom) or None.  The byte image of every box with area
    gets a place in the packed buffer whether or not it has a transform (the estimator reads it).  Returns (ctypes array of
    _hip.WarpDesc, byte offsets (-1 = no image), bytes of the packed buffer).  ValueError for a transform with a non-finite entry or one
    whose fixed-point terms leave int32 for some pixel of its box."""
    if len(transforms) != len(boxes):
        raise ValueError(f"{len(transforms)} transforms for {len(boxes)} boxes")
    offsets, total = _pack_offsets(boxes)
    sizes = [_box_size(b) for b in boxes]
    return _warp_record_table(transforms, sizes, sizes, offsets), offsets, total


@dataclass
class FaceBytes:
    """What face_bytes made: the packed uint8 images on the device (`generated`; `source` when device originals were given), where each
    entry's image starts (`offsets`, -1 = none) and its (w, h) (`sizes`)."""
    generated: torch.Tensor
    source: Optional[torch.Tensor]
    offsets: list
    sizes: list

    def piece(self, first: int, last: int) -> "FaceBytes":
        return FaceBytes(self.generated, self.source, self.offsets[first:last], self.sizes[first:last])

    def image(self, packed: np.ndarray, f: int) -> np.ndarray:
        """entry f's [h, w, 3] image inside a downloaded copy of `generated` or `source`"""
        w, h = self.sizes[f]
        return packed[self.offsets[f]:self.offsets[f] + w * h * 3].reshape(h, w, 3)


@_on_device
def face_bytes(crops: torch.Tensor, entries, height: int, width: int, originals: Optional[torch.Tensor] = None) -> FaceBytes:
    """Steps 1-2 of the landmark-aligned composite for every entry with a box (entries as for composite_frames, frames height x width):
    uint8(clip(rint(clamp(bicubic(crop -> box), 0, 1) * 255), 0, 255)) packed into one device buffer, one launch (vrg_face_bytes_u8).  With
    device `originals` the same quantisation of the unclamped original under each box is made next to it.  A NaN gives byte 0."""
    c = _check_frames(crops, "crops")
    composite_channels(CompositeRule("opaque"), 3 if originals is None else originals.shape[3], c.shape[3])
    table, _, max_pixels = composite_table(entries, CompositeRule("opaque"), 0.0, height, width)
    frames = len(entries)
    sizes = [(table[f].box_w, table[f].box_h) if table[f].rule != _hip.COMPOSITE_NONE else None for f in range(frames)]
    offsets, total = _pack_offsets([(0, 0, s[0], s[1]) if s else None for s in sizes])
    o = None
    if originals is not None:
        o = _check_frames(originals, "originals")
        if o.device != c.device or tuple(o.shape[1:3]) != (int(height), int(width)):
            raise ValueError("originals must be height x width frames on the crops' device")
    n_orig = int(o.shape[0]) if o is not None else max([1] + [table[f].original_index + 1 for f in range(frames)])
    for f in range(frames):
        if not 0 <= table[f].original_index < n_orig or not 0 <= table[f].crop_index < c.shape[0]:
            raise ValueError(f"entry {f} names original {table[f].original_index} / crop {table[f].crop_index} of {n_orig} / {int(c.shape[0])}")
    generated = torch.zeros(max(total, 16), dtype=torch.uint8, device=c.device)
    source = torch.zeros_like(generated) if o is not None else None
    if frames == 0 or total == 0:
        return FaceBytes(generated, source, offsets, sizes)
    dev_table = _hip.upload_records(table, c.device, frames, [np.asarray(offsets, dtype=np.int64)])
    offsets_ptr = C.c_void_p(dev_table.data_ptr() + frames * C.sizeof(_hip.CompositeDesc))
    _hip.check(_hip.lib().vrg_face_bytes_u8(_hip.ptr(c), _hip.ptr(o) if o is not None else None, _hip.ptr(dev_table), offsets_ptr,
                                           _hip.ptr(generated), _hip.ptr(source) if source is not None else None, total, max_pixels,
                                           frames, n_orig, int(c.shape[0]), int(c.shape[1]), int(c.shape[2]), int(c.shape[3]),
                                           int(height), int(width), int(o.shape[3]) if o is not None else 3, _hip.current_stream()),
               "vrg_face_bytes_u8")
    return FaceBytes(generated, source, offsets, sizes)


THUMB_SIDE = _hip.THUMB_SIDE    # the landmark network's input is 320 x 320
THUMB_DESC = _hip.record_dtype(_hip.ThumbDesc)
_THUMB_WHICH = {"generated": 0, "source": 1}


def thumb_plan(box_h: int, box_w: int):
    """(mode, cps, inv) of the resize of a box_w x box_h byte image to 320 x 320: vrg_grid_plan on the host (no GPU needed)"""
    mode, cps, inv = C.c_int32(), C.c_int32(), C.c_float()
    _hip.check(_host_lib().vrg_grid_plan(int(box_h), int(box_w), 3, THUMB_SIDE, THUMB_SIDE, C.byref(mode), C.byref(cps), C.byref(inv)),
               "vrg_grid_plan")
    return mode.value, cps.value, inv.value


def thumb_descriptors(jobs):
    """The vrg_thumb_desc records of jobs [(which 0 | 1, byte offset, box_w, box_h)] with the table pointers still relative, and the
    tables they name: (records, table bytes, [(record index, field, byte position in the tables)]).  One table per distinct
    (n_in, mode), made by grid_taps on the host (no GPU needed)."""
    desc = np.zeros(len(jobs), dtype=THUMB_DESC)
    tables, where, fix, plans = [], {}, [], {}
    for i, (which, offset, w, h) in enumerate(jobs):
        if (w, h) not in plans:
            plans[(w, h)] = thumb_plan(h, w)
        mode, cps, inv = plans[(w, h)]
        desc[i] = (0, 0, offset, which, w, h, mode, cps, inv)
        for field, n_in in (("xtab", w), ("ytab", h)):
            if (n_in, mode) not in where:
                where[(n_in, mode)] = len(tables) * THUMB_SIDE * AREA_CELL.itemsize
                tables.append(grid_taps(n_in, THUMB_SIDE, mode))
            fix.append((i, field, where[(n_in, mode)]))
    return desc, (np.concatenate(tables).view(np.uint8) if tables else np.zeros(0, dtype=np.uint8)), fix


def face_thumbs(faces: FaceBytes, which=("source", "generated"), source: Optional[torch.Tensor] = None):
    """The landmark estimator's input for every entry of `faces` that has an image of at least 2 x 2 pixels (the reference's `_landmarks`
    returns no landmarks below that and resizes nothing): ``cv2.cvtColor(cv2.resize(image, (320, 320), interpolation=cv2.INTER_AREA),
    cv2.COLOR_RGB2BGR)`` of the packed byte images, one launch (vrg_face_thumbs_u8).  Returns (uint8 ``[n, k, 320, 320, 3]`` B,G,R on the
    device, k = len(which) in that order; index[f] = the entry's row, -1 = none).  `source`: the packed source bytes at `faces.offsets`
    when face_bytes made none (host-fed originals: the node quantises the boxes on the CPU and uploads this one buffer)."""
    names = tuple(which)
    if not names or any(n not in _THUMB_WHICH for n in names):
        raise ValueError(f"which must name 'source' and / or 'generated', got {which!r}")
    with torch.cuda.device(faces.generated.device):             # the stream and the pointers belong to the bytes' GPU (_on_device)
        return _face_thumbs(faces, names, source)


def _face_thumbs(faces, names, source):
    g = faces.generated
    src = faces.source if faces.source is not None else source
    if "source" in names and src is None:
        raise ValueError("face_thumbs: there are no source bytes (face_bytes ran without device originals and no `source` was given)")
    if src is not None and (src.dtype != torch.uint8 or src.device != g.device or not src.is_contiguous() or src.numel() < g.numel()):
        raise ValueError("face_thumbs: source must be a contiguous uint8 buffer of the size of faces.generated on its device")
    k = len(names)
    index, jobs = [], []
    for offset, size in zip(faces.offsets, faces.sizes):
        if offset < 0 or size is None or size[0] < 2 or size[1] < 2:
            index.append(-1)
            continue
        index.append(len(jobs) // k)
        jobs += [(_THUMB_WHICH[n], offset, size[0], size[1]) for n in names]
    out = torch.empty((len(jobs) // k, k, THUMB_SIDE, THUMB_SIDE, 3), dtype=torch.uint8, device=g.device)
    if not jobs:
        return out, index
    desc, tables, fix = thumb_descriptors(jobs)
    records = torch.empty(desc.nbytes + tables.nbytes, dtype=torch.uint8, device=g.device)
    base = records.data_ptr() + desc.nbytes
    for i, field, at in fix:
        desc[field][i] = base + at
    n_bytes = int(g.numel())
    lib = _hip.lib()
    _hip.check(lib.vrg_face_thumbs_check(C.c_void_p(desc.ctypes.data), len(desc), n_bytes, int(src is not None)), "vrg_face_thumbs_check")
    _hip.upload_records(desc, g.device, trailing=[tables], out=records)
    _hip.check(lib.vrg_face_thumbs_u8(_hip.ptr(g), _hip.ptr(src) if src is not None else None, n_bytes, _hip.ptr(records), len(desc),
                                      _hip.ptr(out), _hip.current_stream()), "vrg_face_thumbs_u8")
    return out, index


@_on_device
def warp_affine_u8(frames_u8: torch.Tensor, transforms, out_w: int, out_h: int) -> torch.Tensor:
    """``cv2.warpAffine(frame, transform, (out_w, out_h), flags=cv2.INTER_LANCZOS4, borderMode=cv2.BORDER_REFLECT101)`` on every frame of
    a ``[F,H,W,3]`` uint8 batch on the GPU (vrg_warp_affine_u8; the arithmetic is the restatement of csrc/vrg_warp_math.hpp).
    transforms[f] = the frame's 2 x 3 matrix; None gives a frame of zeros.  Refuses as warp_records does."""
    x = _check_frames(frames_u8, "frames", channels=3, dtype=torch.uint8)
    out_w, out_h = int(out_w), int(out_h)
    F, H, W, _ = (int(v) for v in x.shape)
    if out_w < 1 or out_h < 1 or H < 1 or W < 1:
        raise ValueError("warp: frames and the output must be at least 1 x 1")
    if len(transforms) != F:
        raise ValueError(f"{len(transforms)} transforms for {F} frames")
    table = _warp_record_table(transforms, [(out_w, out_h)] * F, [(W, H)] * F, [f * H * W * 3 for f in range(F)])
    out = torch.empty((F, out_h, out_w, 3), dtype=torch.uint8, device=x.device)
    if F == 0:
        return out
    rec = _hip.upload_records(table, x.device, F)
    _hip.check(_hip.lib().vrg_warp_affine_u8(_hip.ptr(x), x.numel(), _hip.ptr(out), _hip.ptr(rec), _hip.ptr(_warp_table(x.device)), F,
                                            out_h, out_w, _hip.current_stream()), "vrg_warp_affine_u8")
    return out


@_on_device
def aligned_composite_frames(originals: torch.Tensor, crops: torch.Tensor, entries, feather, transforms, generated: Optional[FaceBytes] = None,
                             out: Optional[torch.Tensor] = None, mask_out: Optional[torch.Tensor] = None):
    """The landmark-aligned composite on device frames: composite_frames with the opaque rule, where every entry f with transforms[f]
    (2 x 3, as warpAffine takes it) blends fl(warpAffine(byte face) / 255) in place of the bicubic face -- one pass over the output
    (vrg_composite_warp_apply_f32).  `generated`: the FaceBytes of these entries if face_bytes has run already (the node downloads them for
    its estimator), else made here.  Entries without a transform, and a call without any, give composite_frames' bits."""
    if len(transforms) != len(entries):
        raise ValueError(f"{len(transforms)} transforms for {len(entries)} entries")
    rule = CompositeRule("opaque", feather=feather)
    o, c, m, dev_table, match, max_pixels, geom, stats = _composite_prepare(originals, crops, entries, rule, 0.0, None)
    if generated is None:
        sizes = [_box_size(e.get("box")) for e in entries]
        offsets = None
    else:
        if len(generated.offsets) != len(entries) or generated.generated.device != o.device:
            raise ValueError("generated does not belong to these entries")
        sizes, offsets = generated.sizes, generated.offsets
    live = [t if sizes[f] is not None else None for f, t in enumerate(transforms)]
    if offsets is None:
        offsets, _ = _pack_offsets([(0, 0, s[0], s[1]) if s else None for s in sizes])
    records = _warp_record_table(live, sizes, sizes, offsets)                 # refuses before any launch
    if not any(records[f].set for f in range(len(entries))):
        return composite_frames(o, c, entries, rule, 0.0, out=out, mask_out=mask_out)
    if generated is None:
        generated = face_bytes(c, entries, o.shape[1], o.shape[2])
    frames = len(entries)
    shape = (frames, int(o.shape[1]), int(o.shape[2]), int(o.shape[3]))
    out = _checked_out(out, shape, torch.float32, o.device, "aligned_composite_frames")
    mask_out = _checked_out(mask_out, shape[:3], torch.float32, o.device, "aligned_composite_frames", "mask_out")
    _disjoint("aligned_composite_frames", [("out", out), ("mask_out", mask_out)], [("originals", o), ("crops", c), ("generated", generated.generated)])
    rec = _hip.upload_records(records, o.device, frames)
    g = generated.generated
    _hip.check(_hip.lib().vrg_composite_warp_apply_f32(_hip.ptr(c), _hip.ptr(o), None, _hip.ptr(dev_table), _hip.ptr(stats), _hip.ptr(rec),
                                                      _hip.ptr(g), g.numel(), _hip.ptr(_warp_table(o.device)), _hip.ptr(out),
                                                      _hip.ptr(mask_out), *geom, _hip.current_stream()), "vrg_composite_warp_apply_f32")
    return out, mask_out


# ------------------------------------------------------------------------------------------------
# Face Fix crop sequence (both Prepare nodes: VRGDG_StandaloneFaceFixNodes.py:320-351, 387-389, 486-516, 537-539)
# ------------------------------------------------------------------------------------------------

CROP_SIZE = (512, 512)           # the reference's F.interpolate(size=(512, 512))
_CROP_DESC = _hip.record_dtype(_hip.CropDesc)


@dataclass(frozen=True)
class CropPlan:
    """Which rectangle every OUTPUT frame of the crop sequence is resampled from: `sources[k]` = (source frame, (left, top, right,
    bottom)) for output frame k, the `ltx_offset` prefix frames first; `frames`, `height`, `width`: the video the plan was made for."""
    frames: int
    height: int
    width: int
    ltx_offset: int
    sources: tuple

    @property
    def count(self) -> int:
        return len(self.sources)


def _crop_box(box, index: int, height: int, width: int):
    try:
        values = tuple(box)
        if len(values) != 4:
            raise TypeError
        left, top, right, bottom = (operator.index(v) for v in values)
    except TypeError:
        raise ValueError(f"Face Fix box {box!r} of frame {index} is not four integers (left, top, right, bottom); refused") from None
    if right <= left or bottom <= top:
        raise ValueError(f"Face Fix box {(left, top, right, bottom)!r} of frame {index} is empty: the reference fails on it; refused")
    if left < 0 or top < 0 or right > width or bottom > height:
        raise ValueError(f"Face Fix box {(left, top, right, bottom)!r} of frame {index} does not lie inside the {width} x {height} frame: "
                         "the reference crops less than the box there; refused")
    return left, top, right, bottom


def crop_sequence_plan(entries, frames: int, height: int, width: int, *, per_shot: bool = False) -> CropPlan:
    """Which output frame of the Face Fix crop sequence reads which (source frame, box) -- the list work of both Prepare nodes without
    the pixels.  An entry has a crop when entry["box"] is truthy.  A frame without one takes the last crop before it, leading ones the
    first crop of the video (:333-342); with per_shot the first crop of its entry["shot_id"], a shot without any the first crop of the
    video (:501-511).  (-(frames - 1)) % 8 copies of output frame 0 go in front (:348-351): `ltx_offset`.  Pure Python."""
    frames, height, width = int(frames), int(height), int(width)
    entries = list(entries)
    if len(entries) != frames:
        raise ValueError(f"{len(entries)} Face Fix entries for {frames} video frames; refused")
    own = [(i, _crop_box(entry["box"], i, height, width)) if entry.get("box") else None for i, entry in enumerate(entries)]
    valid = [s for s in own if s is not None]
    if not valid:
        raise ValueError("No face was detected in the video. Lower confidence or minimum face pixels.")
    filled = list(own)
    if per_shot:
        first_of_shot = {}
        for entry, s in zip(entries, own):
            if s is not None:
                first_of_shot.setdefault(entry["shot_id"], s)
        for i, entry in enumerate(entries):
            if filled[i] is None:
                filled[i] = first_of_shot.get(entry["shot_id"], valid[0])
    else:
        last = valid[0]
        for i in range(frames):
            if filled[i] is None:
                filled[i] = last
            else:
                last = filled[i]
    ltx_offset = (-(frames - 1)) % 8
    return CropPlan(frames, height, width, ltx_offset, tuple([filled[0]] * ltx_offset + filled))


def _crop_size(size):
    size_h, size_w = (int(v) for v in size)
    if size_h < 1 or size_w < 1:
        raise ValueError(f"crop size {size!r}: the work frames must have at least one pixel")
    return size_h, size_w


@_on_device
def crop_resize(source: torch.Tensor, records, size=CROP_SIZE, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One launch of vrg_crop_resize_f32: `source` = any contiguous float32 device tensor, `records` = one (src_offset, row_pitch,
    pixel_stride, box_w, box_h) per output frame, in floats from the start of `source` (include/vrgdg_hip.h, vrg_crop_desc).  Every record
    is checked against the size of `source` here: one that reaches outside is a ValueError, nothing is launched.  Returns
    [len(records), size_h, size_w, 3], clamped to [0, 1]."""
    if not isinstance(source, torch.Tensor) or source.dtype != torch.float32 or not source.is_contiguous():
        raise ValueError("source must be a contiguous float32 tensor")
    if not source.is_cuda:
        raise RuntimeError("source must live on the GPU (ops.* are device-resident; crop_frames_host packs CPU frames)")
    size_h, size_w = _crop_size(size)
    table = np.zeros(len(records), dtype=_CROP_DESC)
    if len(records):
        rec = np.asarray(records, dtype=np.int64).reshape(len(records), 5)
        offset, pitch, stride, box_w, box_h = (rec[:, k] for k in range(5))
        if (box_w < 1).any() or (box_h < 1).any() or (stride < 3).any() or (pitch < 0).any() or (offset < 0).any() or (rec[:, 1:] > 0x7fffffff).any():
            raise ValueError("crop record with an empty box, a pixel stride below 3 or a negative offset / pitch; refused")
        last = offset + (box_h - 1) * pitch + (box_w - 1) * stride + 3
        bad = np.nonzero((last > source.numel()) | (box_w * stride > 0x7fffffff))[0]
        if bad.size:
            k = int(bad[0])
            raise ValueError(f"crop record {k} {tuple(int(v) for v in rec[k])} reaches float {int(last[k])} of a source of {source.numel()}; refused")
        for k, name in enumerate(("src_offset", "row_pitch", "pixel_stride", "box_w", "box_h")):
            table[name] = rec[:, k]
    out = _checked_out(out, (len(records), size_h, size_w, 3), torch.float32, source.device, "crop_resize")
    _disjoint("crop_resize", [("out", out)], [("source", source)])
    if len(records) == 0:
        return out
    dev_table = _hip.upload_records(table, source.device)
    _hip.check(_hip.lib().vrg_crop_resize_f32(_hip.ptr(source), source.numel(), _hip.ptr(out), _hip.ptr(dev_table), len(records), size_h, size_w,
                                             _hip.current_stream()), "vrg_crop_resize_f32")
    return out


def _check_crop_plan(plan: CropPlan, shape):
    if not isinstance(plan, CropPlan):
        raise ValueError("plan must come from crop_sequence_plan")
    if (int(shape[0]), int(shape[1]), int(shape[2])) != (plan.frames, plan.height, plan.width):
        raise ValueError(f"the plan was made for {plan.frames} frames of {plan.width} x {plan.height}, the video has {int(shape[0])} of "
                         f"{int(shape[2])} x {int(shape[1])}")
    if int(shape[3]) < 3:
        raise ValueError(f"frames must have at least 3 channels, got {int(shape[3])}")


def crop_frames(frames: torch.Tensor, plan: CropPlan, size=CROP_SIZE, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The Face Fix crop sequence of device-resident `frames` ([F, H, W, C >= 3] float32, never written): output frame k is the box
    plan.sources[k] bicubic-resampled to `size` and clamped -- crops, filled holes and the LTX prefix in one launch, no intermediate.
    Returns [plan.ltx_offset + F, size_h, size_w, 3] on the frames' device."""
    x = _check_frames(frames, "frames")
    _check_crop_plan(plan, x.shape)
    h, w, c = int(x.shape[1]), int(x.shape[2]), int(x.shape[3])
    records = [(((f * h + top) * w + left) * c, w * c, c, right - left, bottom - top) for f, (left, top, right, bottom) in plan.sources]
    return crop_resize(x, records, size, out)


def crop_frames_host(frames_cpu: torch.Tensor, plan: CropPlan, size=CROP_SIZE) -> torch.Tensor:
    """crop_frames for CPU frames: only the boxes cross to the GPU.  Every DISTINCT (frame, box) of the plan is packed once as
    [box_h][box_w][3] float32 into a page-locked buffer (a strided torch copy per box), uploaded, and the records point into the pack;
    whole frames are never uploaded.  A pack above VRGDG_PIN_LIMIT_GB goes through in pieces along the output-frame axis.  The batch is
    returned on intermediate_device()."""
    from . import _devices
    if not isinstance(frames_cpu, torch.Tensor) or frames_cpu.ndim != 4 or frames_cpu.is_cuda:
        raise ValueError("frames_cpu must be a CPU [frames, height, width, channels] tensor")
    _check_crop_plan(plan, frames_cpu.shape)
    size_h, size_w = _crop_size(size)
    dev = _devices.compute_device()
    pin = _devices.PIN_LIMIT_BYTES > 0
    limit = (_devices.PIN_LIMIT_BYTES if pin else _devices.STAGE_BYTES) // 4                   # floats per piece
    with torch.cuda.device(dev):
        out = torch.empty((plan.count, size_h, size_w, 3), dtype=torch.float32, device=dev)
        first = 0
        while first < plan.count:
            # the output frames [first, stop) whose distinct boxes fit one pack (one box alone always goes)
            where, floats, stop = {}, 0, first
            while stop < plan.count:
                src = plan.sources[stop]
                if src not in where:
                    left, top, right, bottom = src[1]
                    n = (right - left) * (bottom - top) * 3
                    if where and floats + n > limit:
                        break
                    where[src] = floats
                    floats += n
                stop += 1
            pack = None
            if pin:
                try:
                    pack = torch.empty(floats, dtype=torch.float32, pin_memory=True)
                except RuntimeError:                  # the host refused to page-lock that much: pageable pack
                    pack = None
            if pack is None:
                pack = torch.empty(floats, dtype=torch.float32)
            for (f, (left, top, right, bottom)), at in where.items():
                bw, bh = right - left, bottom - top
                pack[at:at + bh * bw * 3].view(bh, bw, 3).copy_(frames_cpu[f, top:bottom, left:right, :3])
            records = [(where[s], (s[1][2] - s[1][0]) * 3, 3, s[1][2] - s[1][0], s[1][3] - s[1][1]) for s in plan.sources[first:stop]]
            crop_resize(pack.to(dev, non_blocking=True), records, (size_h, size_w), out[first:stop])
            torch.cuda.current_stream().synchronize()  # the pack is reused by the allocator once it is dropped
            first = stop
    return out.to(_devices.intermediate_device())


def crop_host_bytes(plan: CropPlan) -> int:
    """Bytes crop_frames_host uploads for `plan`: its distinct boxes as float32 RGB."""
    return sum((r - l) * (b - t) * 12 for _, (l, t, r, b) in set(plan.sources))


# ------------------------------------------------------------------------------------------------
# The hard-cut score of the shot-aware Face Fix Prepare nodes (reference VRGDG_StandaloneFaceFixNodes.py:421-435, :456): 64 x 64
# INTER_AREA thumbnails of the quantised frames, their hue / saturation histograms, four integers per consecutive pair
# ------------------------------------------------------------------------------------------------
CUT_THUMB = 64                  # the thumbnail is 64 x 64 x 3 bytes
AREA_CELL = _hip.record_dtype(_hip.AreaCell)
_area_tables: dict = {}         # (height, width, device) -> the uploaded table


def _check_cut_shape(shape):
    """The refusals of the cut score, before anything is uploaded."""
    if len(shape) != 4:
        raise ValueError("cut score: frames must be a [frames, height, width, channels] batch")
    if int(shape[3]) < 3:
        raise ValueError(f"cut score: frames must have at least 3 channels, got {int(shape[3])}")
    if int(shape[1]) < CUT_THUMB or int(shape[2]) < CUT_THUMB:
        raise ValueError(f"cut score: {int(shape[2])} x {int(shape[1])} frames have a side below {CUT_THUMB} px; cv2's INTER_AREA takes "
                         "another, bilinear-like route there, which is out of scope; refused")


def area_taps(in_h: int, in_w: int) -> np.ndarray:
    """The table of the thumbnail kernel, made on the host (no GPU needed): 64 column cells then 64 row cells (AREA_CELL records: the
    taps of output index d are the source samples first .. first + count - 1, the first weighs w_first, the last w_last, the others w_mid)."""
    in_h, in_w = int(in_h), int(in_w)
    if min(in_h, in_w) < CUT_THUMB:
        raise ValueError(f"area_taps: sides must be at least {CUT_THUMB}")
    table = np.zeros(2 * CUT_THUMB, dtype=AREA_CELL)
    _hip.check(_host_lib().vrg_area_taps(in_h, in_w, C.c_void_p(table.ctypes.data)), "vrg_area_taps")
    return table


def _area_table(in_h, in_w, device) -> torch.Tensor:
    return _uploaded(_area_tables, (in_h, in_w, str(device)), lambda: area_taps(in_h, in_w), device)


@_on_device
def cut_thumbnails(frames: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``cv2.resize(rgb, (64, 64), interpolation=cv2.INTER_AREA)`` of ``rgb = (frame[..., :3].clamp(0, 1) * 255).round().astype(uint8)`` for
    every frame of a device-resident ``[F, H, W, C >= 3]`` fp32 batch (never written), in one launch of vrg_cut_thumbs_f32.  Returns
    ``[F, 64, 64, 3]`` uint8 on the frames' device."""
    if isinstance(frames, torch.Tensor):
        _check_cut_shape(frames.shape)
    x = _check_frames(frames, "frames")
    F, H, W, Cn = (int(v) for v in x.shape)
    if Cn > 4:
        x = x[..., :3].contiguous()
        Cn = 3
    out = _checked_out(out, (F, CUT_THUMB, CUT_THUMB, 3), torch.uint8, x.device, "cut_thumbnails")
    _disjoint("cut_thumbnails", [("out", out)], [("frames", x)])
    if F == 0:
        return out
    taps = _area_table(H, W, x.device)
    _hip.check(_hip.lib().vrg_cut_thumbs_f32(_hip.ptr(x), _hip.ptr(out), F, H, W, Cn, _hip.ptr(taps), _hip.current_stream()), "vrg_cut_thumbs_f32")
    return out


def cut_thumbnails_host(frames_cpu: torch.Tensor) -> torch.Tensor:
    """cut_thumbnails for CPU frames: they go up through the staging pipeline of _devices in pieces along the frame axis (page-locked
    ring, upload of piece i + 1 under the kernel of piece i); nothing comes back -- the ``[F, 64, 64, 3]`` thumbnails stay on the compute
    device for the pair pass."""
    from . import _devices
    if not isinstance(frames_cpu, torch.Tensor) or frames_cpu.is_cuda:
        raise ValueError("frames_cpu must be a CPU [frames, height, width, channels] tensor")
    _check_cut_shape(frames_cpu.shape)
    if frames_cpu.dtype != torch.float32:
        frames_cpu = frames_cpu.float()
    dev = _devices.compute_device()
    with torch.cuda.device(dev):
        out = torch.empty((int(frames_cpu.shape[0]), CUT_THUMB, CUT_THUMB, 3), dtype=torch.uint8, device=dev)
        _devices.upload_frames(frames_cpu, lambda gpu, first: cut_thumbnails(gpu, out=out[first:first + int(gpu.shape[0])]))
    return out


@_on_device
def cut_histograms(thumbs: torch.Tensor) -> torch.Tensor:
    """``calcHist([cvtColor(thumb, COLOR_RGB2HSV)], [0, 1], None, [32, 32], [0, 180, 0, 256])`` as int32 ``[F, 1024]`` (vrg_cut_hist_u8)."""
    t = _check_frames(thumbs, "thumbs", channels=3, dtype=torch.uint8)
    if tuple(t.shape[1:3]) != (CUT_THUMB, CUT_THUMB):
        raise ValueError(f"thumbs must be [frames, {CUT_THUMB}, {CUT_THUMB}, 3] uint8")
    hist = torch.empty((int(t.shape[0]), 1024), dtype=torch.int32, device=t.device)
    if t.shape[0]:
        _hip.check(_hip.lib().vrg_cut_hist_u8(_hip.ptr(t), _hip.ptr(hist), int(t.shape[0]), _hip.current_stream()), "vrg_cut_hist_u8")
    return hist


@_on_device
def cut_pair_sums(thumbs: torch.Tensor, hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 ``[F - 1, 4]`` = (D, S11, S22, S12) of every consecutive pair of thumbnails: D = sum |a - b| over the 12288 bytes, the S the
    sums of squares and products of the two histograms (cut_histograms, computed here when not given).  Exact integers: the score made
    of them does not depend on how the frames were cut into launches."""
    t = _check_frames(thumbs, "thumbs", channels=3, dtype=torch.uint8)
    if hist is None:
        hist = cut_histograms(t)
    F = int(t.shape[0])
    hist = _check_side(hist, "hist", t, shape_tail=(1024,), dtype=torch.int32)
    if int(hist.shape[0]) != F:
        raise ValueError(f"{int(hist.shape[0])} histograms for {F} thumbnails")
    sums = torch.empty((max(F - 1, 0), 4), dtype=torch.int64, device=t.device)
    if F > 1:
        _hip.check(_hip.lib().vrg_cut_pair_sums(_hip.ptr(t), _hip.ptr(hist), _hip.ptr(sums), F, _hip.current_stream()), "vrg_cut_pair_sums")
    return sums


# ------------------------------------------------------------------------------------------------
# The Video Folder Grid Plot (reference LTXLoraTrain.py:7926-8314): every tile of every output frame quantised, resized as
# cv2.resize(..., INTER_AREA) does on bytes and written as fp32 / 255 straight into the grid frame (csrc/vrg_grid.hip, arithmetic
# csrc/vrg_grid_math.hpp)
# ------------------------------------------------------------------------------------------------
GRID_MODES = ("copy", "fast", "fast 2x2", "general", "linear")          # include/vrgdg_hip.h, enum vrg_grid_mode
GRID_ROW_VALUES = 4096          # source values one wave stages at a time (csrc/vrg_grid_math.hpp): the most one column's taps may cover
GRID_DESC = _hip.record_dtype(_hip.GridDesc)
_grid_tables: dict = {}         # (n_in, n_out, mode, device) -> the uploaded table of one axis; at most 256


@dataclass(frozen=True)
class GridTile:
    """One tile: the source size and what `_fit_frame_to_tile` makes of it."""
    height: int
    width: int
    channels: int
    new_w: int
    new_h: int
    x_off: int
    y_off: int
    mode: int
    cps: int
    inv: float
    xtab: np.ndarray
    ytab: np.ndarray


@dataclass(frozen=True)
class GridPlan:
    cell_w: int
    cell_h: int
    columns: int
    rows: int
    band: int
    tiles: tuple

    @property
    def grid_w(self) -> int:
        return self.columns * self.cell_w

    @property
    def grid_h(self) -> int:
        return self.rows * self.cell_h


def grid_taps(n_in: int, n_out: int, mode: int) -> np.ndarray:
    """The table of one axis of one resize in one mode, made on the host (AREA_CELL records, n_out of them)."""
    table = np.zeros(int(n_out), dtype=AREA_CELL)
    _hip.check(_host_lib().vrg_grid_taps(int(n_in), int(n_out), int(mode), C.c_void_p(table.ctypes.data)), "vrg_grid_taps")
    return table


def grid_tile(height: int, width: int, channels: int, cell_w: int, cell_h: int, band: int) -> GridTile:
    """The geometry of `_fit_frame_to_tile` (LTXLoraTrain.py:8063-8074) in Python doubles, the rule cv2 takes for it and its tables."""
    height, width, channels, cell_w, cell_h, band = (int(v) for v in (height, width, channels, cell_w, cell_h, band))
    if channels not in (3, 4):
        raise ValueError(f"video grid: frames must have 3 or 4 channels, got {channels}")
    if height < 1 or width < 1:
        raise ValueError("video grid: empty frames")
    content_h = max(16, cell_h - band)
    scale = min(float(cell_w) / max(1, width), float(content_h) / max(1, height))
    new_w, new_h = max(1, int(round(width * scale))), max(1, int(round(height * scale)))
    x_off, y_off = max(0, (cell_w - new_w) // 2), band + max(0, (content_h - new_h) // 2)
    if y_off + new_h > cell_h or x_off + new_w > cell_w:
        raise ValueError(f"video grid: the {new_w} x {new_h} picture at ({x_off}, {y_off}) does not fit the {cell_w} x {cell_h} tile "
                         "(the reference's slice assignment fails here too)")
    mode, cps, inv = C.c_int32(), C.c_int32(), C.c_float()
    status = _host_lib().vrg_grid_plan(height, width, channels, new_h, new_w, C.byref(mode), C.byref(cps), C.byref(inv))
    if status == _hip.VRG_ERR_UNSUPPORTED:
        raise ValueError(f"video grid: one column of the {new_w} x {new_h} picture covers more than {GRID_ROW_VALUES} source values of a "
                         f"{width}-wide row with {channels} channels (more than {GRID_ROW_VALUES // channels} pixels); the kernel does not take that")
    _hip.check(status, "vrg_grid_plan")
    return GridTile(height, width, channels, new_w, new_h, x_off, y_off, mode.value, cps.value, inv.value,
                    grid_taps(width, new_w, mode.value), grid_taps(height, new_h, mode.value))


def grid_plan(sizes, cell_w: int, cell_h: int, columns: int, band: int = 0) -> GridPlan:
    """Sizes ``[(height, width, channels), ...]`` of the tiles' sources -> geometry, modes and tables; no GPU is needed."""
    cell_w, cell_h, columns, band = int(cell_w), int(cell_h), int(columns), int(band)
    sizes = [tuple(int(v) for v in s) for s in sizes]
    if not sizes:
        raise ValueError("video grid: no tiles")
    if cell_w < 1 or cell_h < 1 or columns < 1 or band < 0:
        raise ValueError("video grid: cell_w, cell_h, columns must be positive and band non-negative")
    tiles = tuple(grid_tile(h, w, c, cell_w, cell_h, band) for h, w, c in sizes)
    return GridPlan(cell_w, cell_h, columns, -(-len(sizes) // columns), band, tiles)


def _grid_table(n_in, n_out, mode, table, device) -> torch.Tensor:
    return _uploaded(_grid_tables, (n_in, n_out, mode, str(device)), lambda: table, device, limit=256)


def _grid_overlays(plan: GridPlan, overlays, device):
    """[tiles, band, cell_w, 3] uint8 on the device (or None) and which tiles have one"""
    n = len(plan.tiles)
    if overlays is None or plan.band == 0 or all(o is None for o in overlays):
        return None, [False] * n
    if len(overlays) != n:
        raise ValueError(f"{len(overlays)} overlays for {n} tiles")
    host = np.zeros((n, plan.band, plan.cell_w, 3), dtype=np.uint8)
    has = []
    for i, o in enumerate(overlays):
        has.append(o is not None)
        if o is not None:
            o = np.asarray(o)
            if o.dtype != np.uint8 or o.shape != (plan.band, plan.cell_w, 3):
                raise ValueError(f"overlay {i} must be uint8 [{plan.band}, {plan.cell_w}, 3]")
            host[i] = o
    return torch.from_numpy(host).to(device), has


def _grid_descriptors(plan: GridPlan, device, jobs, dev_overlays, has_overlay):
    """The vrg_grid_desc records of jobs [(tile index or None for an empty cell, cell index, device frames [n, H, W, C] or None, first
    output frame, source index per output frame (int array; -1: no picture))] and the tensors they point into."""
    parts, keep = [], []
    for tile_index, cell, source, first, index in jobs:
        index = np.asarray(index, dtype=np.int64)
        d = np.zeros(len(index), dtype=GRID_DESC)
        d["frame"] = first + np.arange(len(index))
        d["dst_x"], d["dst_y"] = (cell % plan.columns) * plan.cell_w, (cell // plan.columns) * plan.cell_h
        d["band"] = plan.band
        if tile_index is not None:
            t = plan.tiles[tile_index]
            if dev_overlays is not None and has_overlay[tile_index]:
                d["overlay"] = dev_overlays[tile_index].data_ptr()
            if source is not None:
                if tuple(source.shape[1:]) != (t.height, t.width, t.channels) or not source.is_contiguous() or source.device != device:
                    raise ValueError("video grid: a source does not match its plan")
                if index.size and (int(index.max()) >= int(source.shape[0]) or int(index.min()) < -1):
                    raise ValueError("video grid: a source frame index lies outside its batch")
                xtab = _grid_table(t.width, t.new_w, t.mode, t.xtab, device)
                ytab = _grid_table(t.height, t.new_h, t.mode, t.ytab, device)
                keep += [source, xtab, ytab]
                frame_bytes = t.height * t.width * t.channels * source.element_size()
                d["src"] = np.where(index >= 0, source.data_ptr() + index * frame_bytes, 0).astype(np.uint64)
                d["xtab"], d["ytab"] = xtab.data_ptr(), ytab.data_ptr()
                for name in ("height", "width", "channels", "mode", "new_w", "new_h", "x_off", "y_off", "cps", "inv"):
                    d[name] = getattr(t, name)
        parts.append(d)
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=GRID_DESC)), keep


def _grid_launch(plan: GridPlan, out: torch.Tensor, jobs, dev_overlays, has_overlay, byte_sources: bool):
    """One launch (vrg_grid_tiles_f32 / _u8) of the jobs of _grid_descriptors into `out`, checked on the host first."""
    frames = int(out.shape[0])
    desc, _keep = _grid_descriptors(plan, out.device, jobs, dev_overlays, has_overlay)
    if not len(desc):
        return
    lib = _hip.lib()
    geometry = (frames, plan.cell_w, plan.cell_h, plan.grid_w, plan.grid_h)
    _hip.check(lib.vrg_grid_check(C.c_void_p(desc.ctypes.data), len(desc), int(byte_sources), *geometry), "vrg_grid_check")
    dev_desc = _hip.upload_records(desc, out.device)
    entry = lib.vrg_grid_tiles_u8 if byte_sources else lib.vrg_grid_tiles_f32
    _hip.check(entry(_hip.ptr(dev_desc), len(desc), _hip.ptr(out), *geometry, _hip.current_stream()),
               "vrg_grid_tiles_u8" if byte_sources else "vrg_grid_tiles_f32")


def _grid_batches(batches, dtype):
    out = []
    for i, b in enumerate(batches):
        if not isinstance(b, torch.Tensor) or b.ndim not in (3, 4):
            raise ValueError(f"video grid: batch {i} must be a [frames, height, width, channels] or [height, width, channels] tensor")
        if b.ndim == 3:
            b = b.unsqueeze(0)
        if int(b.shape[0]) < 1:
            raise ValueError(f"video grid: batch {i} is empty")
        if int(b.shape[3]) not in (3, 4):
            raise ValueError(f"video grid: frames must have 3 or 4 channels, got {int(b.shape[3])}")
        if b.dtype != dtype:
            b = b.to(dtype)
        out.append(b.detach())
    if not out:
        raise ValueError("video grid: no batches")
    return out


def _grid_run(batches, index, plan, overlays, out, byte_sources):
    """Device-resident batches and the empty cells in one launch; every CPU batch through the page-locked ring in pieces along its frames,
    one launch per piece for its tile alone.  index[i][f]: the frame of batch i that output frame f shows (-1: none)."""
    from . import _devices
    frames = len(index[0])
    dev = _placement([b.device for b in batches if b is not None], "video grid", "batches", ring=True)     # every CUDA batch lives on it
    with torch.cuda.device(dev):
        out = _checked_out(out, (frames, plan.grid_h, plan.grid_w, 3), torch.float32, dev, "video grid")
        dev_overlays, has = _grid_overlays(plan, overlays, dev)
        jobs = [(None, cell, None, 0, np.full(frames, -1)) for cell in range(len(batches), plan.rows * plan.columns)]
        for i, b in enumerate(batches):
            if b is None:
                jobs.append((i, i, None, 0, index[i]))
            elif b.is_cuda:
                jobs.append((i, i, b.contiguous(), 0, index[i]))
        _disjoint("video grid", [("out", out)], [(f"batch {job[0]}", job[2]) for job in jobs])
        _grid_launch(plan, out, jobs, dev_overlays, has, byte_sources)
        for i, b in enumerate(batches):
            if b is None or b.is_cuda:
                continue
            idx = np.asarray(index[i], dtype=np.int64)

            def piece(gpu, first, i=i, idx=idx):
                n = int(gpu.shape[0])
                shown = np.nonzero((idx >= first) & (idx < first + n))[0]         # the output frames that show a frame of this piece
                if first == 0:
                    shown = np.union1d(shown, np.nonzero(idx < 0)[0])
                for run in np.split(shown, np.nonzero(np.diff(shown) != 1)[0] + 1):
                    if len(run):
                        local = np.where(idx[run] >= 0, idx[run] - first, -1)
                        _grid_launch(plan, out, [(i, i, gpu, int(run[0]), local)], dev_overlays, has, byte_sources)

            _devices.upload_frames(b, piece)
    return out


def video_grid(batches, cell_w: int, cell_h: int, columns: int, band: int = 0, overlays=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The grid frames of VRGDG_VideoFolderGridPlot for IMAGE batches (``[F, H, W, C]`` or ``[H, W, C]`` fp32, C 3 or 4, on the GPU or on
    the CPU, never written): fp32 ``[max F, rows * cell_h, columns * cell_w, 3]`` on the GPU.  A batch that has ended holds its last
    frame.  ``overlays[i]``: uint8 ``[band, cell_w, 3]`` R,G,B or None, shown / 255 in the first ``band`` rows of tile i."""
    batches = _grid_batches(batches, torch.float32)
    plan = grid_plan([tuple(b.shape[1:]) for b in batches], cell_w, cell_h, columns, band)
    frames = max(int(b.shape[0]) for b in batches)
    index = [np.minimum(np.arange(frames), int(b.shape[0]) - 1) for b in batches]
    return _grid_run(batches, index, plan, overlays, out, False)


def video_grid_bytes(batches, index, cell_w: int, cell_h: int, columns: int, band: int = 0, overlays=None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """video_grid for decoded B,G,R byte frames: uint8 ``[n, H, W, 3]`` per tile, or None for a tile that never had a picture (the
    reference fits a black frame there).  ``index[i][f]`` names the frame of batch i that output frame f shows, -1 for none."""
    prepared = [None if b is None else _grid_batches([b], torch.uint8)[0] for b in batches]
    if any(b is not None and int(b.shape[3]) != 3 for b in prepared):
        raise ValueError("video grid: decoded frames must have 3 channels")
    shapes = [tuple(b.shape[1:]) if b is not None else (max(16, int(cell_h) - int(band)), int(cell_w), 3) for b in prepared]
    plan = grid_plan(shapes, cell_w, cell_h, columns, band)
    index = [np.asarray(ix, dtype=np.int64) for ix in index]
    if len(index) != len(prepared) or len({len(ix) for ix in index}) != 1 or not len(index[0]):
        raise ValueError("video grid: one index row per tile, all of one positive length")
    index = [np.full(len(ix), -1) if b is None else ix for b, ix in zip(prepared, index)]
    return _grid_run(prepared, index, plan, overlays, out, True)


# ------------------------------------------------------------------------------------------------
# The input of the Face Fix face detector (reference VRGDG_StandaloneFaceFixNodes.py:95-185, VRGDG_FaceFix.py:67-157): rotated scans and
# 300 x 300 blobs in one launch (csrc/vrg_detect.hip, arithmetic csrc/vrg_detect_math.hpp)
# ------------------------------------------------------------------------------------------------
DETECT_BLOB = 300               # the network's input is 300 x 300
DETECT_MIN_SIDE = 8             # a region with a smaller side is refused (the Builder skips those)
DETECT_MAX_SIDE = 32767         # positions of the warp are int16
DETECT_DESC, DETECT_FRAME_DESC = _hip.record_dtype(_hip.DetectDesc), _hip.record_dtype(_hip.DetectFrameDesc)


def linear_taps(n_in: int, n_out: int = DETECT_BLOB) -> dict:
    """The tables of one axis of ``cv2.resize(..., INTER_LINEAR)`` on bytes from ``n_in`` to ``n_out`` samples, made on the host by
    vrg_linear_taps (no GPU needed): ``h_ofs`` int32 [n_out] and ``h_coef`` int16 [n_out, 2] for the horizontal pass (sample s and s + 1;
    at the borders s is 0 or n_in - 1 and the second weight 0), ``v_ofs`` / ``v_coef`` for the vertical pass (s = floor(f), which may be -1
    or n_in - 1: the two rows are clamped to the axis, the weights stay)."""
    n_in, n_out = int(n_in), int(n_out)
    if not (1 <= n_in <= DETECT_MAX_SIDE and 1 <= n_out <= DETECT_MAX_SIDE):
        raise ValueError(f"linear_taps: sizes must lie in 1 .. {DETECT_MAX_SIDE}")
    ofs = np.zeros(2 * n_out, dtype=np.int32)
    coef = np.zeros(4 * n_out, dtype=np.int16)
    _hip.check(_host_lib().vrg_linear_taps(n_in, n_out, C.c_void_p(ofs.ctypes.data), C.c_void_p(coef.ctypes.data)), "vrg_linear_taps")
    coef = coef.reshape(2, n_out, 2)
    return {"h_ofs": ofs[:n_out].copy(), "h_coef": coef[0].copy(), "v_ofs": ofs[n_out:].copy(), "v_coef": coef[1].copy()}


def _detect_inputs(frames, descriptors, transforms, dtype, name):
    """The refusals of the detector input, before anything is uploaded -> (frames [F, H, W, C], descriptor records, [T, 6] doubles)."""
    if not isinstance(frames, torch.Tensor) or frames.ndim != 4:
        raise ValueError(f"{name}: frames must be a [frames, height, width, channels] tensor")
    F, H, W, Cn = (int(v) for v in frames.shape)
    if frames.dtype == torch.uint8:
        if Cn != 3:
            raise ValueError(f"{name}: uint8 frames are decoded B,G,R frames with 3 channels, got {Cn}")
    elif Cn < 3:
        raise ValueError(f"{name}: frames must have at least 3 channels, got {Cn}")
    if H < 1 or W < 1 or H > DETECT_MAX_SIDE or W > DETECT_MAX_SIDE:
        raise ValueError(f"{name}: {W} x {H} frames: sides must lie in 1 .. {DETECT_MAX_SIDE}")
    t = np.ascontiguousarray(np.asarray(transforms if transforms is not None else [], dtype=np.float64).reshape(-1, 6))
    if not np.isfinite(t).all():
        raise ValueError(f"{name}: transforms must be finite")
    d = np.asarray(descriptors)
    if d.dtype != dtype:
        d = np.array([tuple(int(v) for v in row) for row in np.asarray(descriptors).reshape(-1, len(dtype.names)).tolist()], dtype=dtype)
    d = np.ascontiguousarray(d.reshape(-1))
    return d, t, (F, H, W, Cn)


def detect_check(descriptors, frames: int, height: int, width: int, transforms: int) -> None:
    """ValueError when a blob descriptor names a frame or a transform that does not exist, or a region that does not lie inside the frame
    or has a side below 8 (vrg_detect_check, on the host)."""
    d = np.ascontiguousarray(descriptors)
    st = _host_lib().vrg_detect_check(C.c_void_p(d.ctypes.data if d.size else 0), int(d.size), int(frames), int(height), int(width), int(transforms))
    if st != _hip.VRG_OK:
        raise ValueError(f"detector input: a descriptor names a frame outside 0 .. {int(frames) - 1}, a transform outside -1 .. {int(transforms) - 1}, "
                         f"or a region that does not lie inside the {int(width)} x {int(height)} frame with both sides >= {DETECT_MIN_SIDE}")


def _detect_run(frames, records, launch, out):
    """Run `launch(gpu_frames, records of those frames with the frame index rebased, out rows)` over device frames at once or over CPU
    frames piece by piece through the staging pipeline of _devices; `out` rows are in the order of the records."""
    if frames.is_cuda:
        x = frames if frames.is_contiguous() else frames.contiguous()
        with torch.cuda.device(x.device):
            launch(x, records, out)
        return out
    from . import _devices
    # only the frames the records name cross PCIe: a run of frames as a view, scattered ones gathered on the host first
    used = np.unique(records["frame"])
    if used.size < int(frames.shape[0]):
        records = records.copy()
        if int(used[-1]) - int(used[0]) + 1 == used.size:
            frames = frames[int(used[0]):int(used[-1]) + 1]
            records["frame"] -= int(used[0])
        else:
            frames = frames.index_select(0, torch.from_numpy(used.astype(np.int64)))
            records["frame"] = np.searchsorted(used, records["frame"]).astype(np.int32)
    order = np.arange(records.size)

    def piece(gpu, first):
        last = first + int(gpu.shape[0])
        pick = order[(records["frame"] >= first) & (records["frame"] < last)]
        if pick.size == 0:
            return
        sub = records[pick].copy()
        sub["frame"] -= first
        if int(pick[-1]) - int(pick[0]) + 1 == pick.size and (np.diff(pick) == 1).all():
            launch(gpu, sub, out[int(pick[0]):int(pick[-1]) + 1])
        else:                                                                    # records not grouped by frame: gather the rows afterwards
            tmp = torch.empty((pick.size,) + tuple(out.shape[1:]), dtype=out.dtype, device=out.device)
            launch(gpu, sub, tmp)
            out.index_copy_(0, torch.from_numpy(pick).to(out.device), tmp)

    _devices.upload_frames(frames, piece)
    return out


def detect_blobs(frames: torch.Tensor, descriptors, transforms) -> torch.Tensor:
    """``blobFromImage(cv2.resize(rotated[top:bottom, left:right], (300, 300)), 1.0, (300, 300), (104, 177, 123))`` for every descriptor
    ``(frame, transform, left, top, right, bottom)`` (DETECT_DESC records or rows of six integers), where ``rotated`` is
    ``cv2.warpAffine(bgr, M, (W, H), INTER_LINEAR, BORDER_REPLICATE)`` of the quantised B,G,R frame for ``transform >= 0`` (``transforms``:
    ``[T, 6]`` doubles, the INVERTED matrices) and the frame itself for -1 -- one launch of vrg_detect_blobs_f32 / _u8; the rotated frame
    is never written.  ``frames``: ``[F, H, W, C >= 3]`` fp32 R,G,B (other float types are converted) or ``[F, H, W, 3]`` uint8 B,G,R, on
    the GPU or on the CPU (of CPU frames those the descriptors name go up through the staging pipeline of _devices in pieces, once); never written.  Returns fp32
    ``[N, 3, 300, 300]`` on the compute device."""
    d, t, (F, H, W, Cn) = _detect_inputs(frames, descriptors, transforms, DETECT_DESC, "detect_blobs")
    detect_check(d, F, H, W, len(t))
    if frames.dtype not in (torch.uint8, torch.float32):
        frames = frames.float()
    from . import _devices
    dev = frames.device if frames.is_cuda else _devices.compute_device()
    with torch.cuda.device(dev):
        out = torch.empty((d.size, 3, DETECT_BLOB, DETECT_BLOB), dtype=torch.float32, device=dev)
        if d.size == 0:
            return out
        tr = torch.from_numpy(t.copy()).to(dev) if len(t) else None

        def launch(x, records, rows):
            rec = _hip.upload_records(records, x.device)
            n, h, w, c = (int(v) for v in x.shape)
            if x.dtype == torch.uint8:
                st = _hip.lib().vrg_detect_blobs_u8(_hip.ptr(x), n, h, w, _hip.ptr(tr) if tr is not None else None, len(t), _hip.ptr(rec), records.size,
                                                    _hip.ptr(rows), _hip.current_stream())
            else:
                st = _hip.lib().vrg_detect_blobs_f32(_hip.ptr(x), n, h, w, c, _hip.ptr(tr) if tr is not None else None, len(t), _hip.ptr(rec),
                                                     records.size, _hip.ptr(rows), _hip.current_stream())
            _hip.check(st, "vrg_detect_blobs")
            rec.record_stream(torch.cuda.current_stream())

        return _detect_run(frames, d, launch, out)


def warp_linear_bytes(frames: torch.Tensor, descriptors, transforms) -> torch.Tensor:
    """``cv2.warpAffine(bgr, M, (W, H), flags=INTER_LINEAR, borderMode=BORDER_REPLICATE)`` of the quantised B,G,R frame for every descriptor
    ``(frame, transform)`` (-1: the B,G,R bytes of the frame itself) -> uint8 ``[N, H, W, 3]`` on the compute device (vrg_warp_linear_u8).
    Frames and transforms as detect_blobs takes them; never written."""
    d, t, (F, H, W, Cn) = _detect_inputs(frames, descriptors, transforms, DETECT_FRAME_DESC, "warp_linear_bytes")
    if d.size and (int(d["frame"].min()) < 0 or int(d["frame"].max()) >= F or int(d["transform"].min()) < -1 or int(d["transform"].max()) >= len(t)):
        raise ValueError(f"warp_linear_bytes: a descriptor names a frame outside 0 .. {F - 1} or a transform outside -1 .. {len(t) - 1}")
    if frames.dtype not in (torch.uint8, torch.float32):
        frames = frames.float()
    from . import _devices
    dev = frames.device if frames.is_cuda else _devices.compute_device()
    with torch.cuda.device(dev):
        out = torch.empty((d.size, H, W, 3), dtype=torch.uint8, device=dev)
        if d.size == 0:
            return out
        tr = torch.from_numpy(t.copy()).to(dev) if len(t) else None

        def launch(x, records, rows):
            rec = _hip.upload_records(records, x.device)
            n, h, w, c = (int(v) for v in x.shape)
            st = _hip.lib().vrg_warp_linear_u8(_hip.ptr(x), 0 if x.dtype == torch.uint8 else c, n, h, w, _hip.ptr(tr) if tr is not None else None,
                                               len(t), _hip.ptr(rec), records.size, _hip.ptr(rows), _hip.current_stream())
            _hip.check(st, "vrg_warp_linear_u8")
            rec.record_stream(torch.cuda.current_stream())

        return _detect_run(frames, d, launch, out)


# ------------------------------------------------------------------------------------------------
# 13-slider Adjust (video routes)
# ------------------------------------------------------------------------------------------------

def adjust_terms(adjust: dict, device_math: bool = False) -> "_hip.AdjustDesc":
    """Slider arithmetic of _apply_adjust_tensor (VRGDG_LUTVideoTools.py:309-315 ff.) in Python doubles, rounded
    once to fp32 -- what torch does with a Python scalar operand.  `adjust` is a normalized settings dict.
    `device_math`: reproduce the reference run with device="cuda" (its `/ 0.45`, `/ 1.05` become multiplications by the
    fp32-rounded reciprocal, as torch evaluates tensor / scalar on a GPU) instead of with device="cpu" (IEEE quotients)."""
    d = _hip.AdjustDesc()
    d.div_mode = _hip.ADJUST_DIV_DEVICE if device_math else _hip.ADJUST_DIV_IEEE
    d.enabled = 1 if adjust["enabled"] else 0
    t, ti = adjust["temperature"], adjust["tint"]
    d.shift[0] = _f32(t / 400.0 - ti / 900.0)
    d.shift[1] = _f32(ti / 450.0)
    d.shift[2] = _f32(-t / 400.0 - ti / 900.0)
    d.exposure = _f32(2.0 ** (adjust["exposure"] / 100.0))
    d.contrast = _f32(1.0 + (adjust["contrast"] / 100.0))
    d.saturation = _f32(1.0 + (adjust["saturation"] / 100.0))
    d.highlights = _f32(adjust["highlights"] / 220.0)
    d.shadows = _f32(adjust["shadows"] / 220.0)
    d.whites = _f32(adjust["whites"] / 240.0)
    d.blacks = _f32(adjust["blacks"] / 240.0)
    clarity = adjust["clarity"] / 100.0
    sharpen = adjust["sharpen"] / 100.0
    d.has_clarity = 1 if abs(clarity) > 0.001 else 0
    d.clarity = _f32(clarity)
    d.has_sharpen = 1 if sharpen > 0.001 else 0
    d.sharpen = _f32(sharpen)
    fade = adjust["fade"] / 100.0
    d.has_fade = 1 if fade > 0.0 else 0
    d.fade_mul = _f32(1.0 - fade * 0.35)
    d.fade_add = _f32(fade * 0.18)
    vignette = adjust["vignette"] / 100.0
    d.has_vignette = 1 if vignette > 0.0 else 0
    d.vignette = _f32(vignette)
    return d


@_on_device
def adjust(images: torch.Tensor, terms: "_hip.AdjustDesc", out: torch.Tensor | None = None,
           workspace: torch.Tensor | None = None) -> torch.Tensor:
    """Run the Adjust kernels on ``[F,H,W,3]`` frames: fp32 R,G,B tensors, or uint8 B,G,R decoded frames (then the
    result is uint8 B,G,R as well, equal to convert -> adjust -> convert).  `workspace` (fp32, same shape) is used
    only when clarity and sharpen are both active; it is allocated when not supplied."""
    u8 = isinstance(images, torch.Tensor) and images.dtype == torch.uint8       # decoded BGR frames (video routes)
    x = _check_frames(images, dtype=torch.uint8 if u8 else torch.float32)
    if x.shape[-1] != 3:
        raise ValueError("adjust expects 3-channel frames")
    out = _checked_out(out, x.shape, x.dtype, x.device, "adjust")
    F, H, W, _ = x.shape
    tmp = None
    if terms.enabled and terms.has_clarity and terms.has_sharpen:
        tmp = workspace if workspace is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
        if (not isinstance(tmp, torch.Tensor) or tmp.shape != x.shape or tmp.dtype != torch.float32 or not tmp.is_contiguous()
                or tmp.device != x.device):
            raise ValueError("adjust workspace must be a contiguous float32 tensor shaped like the frames")
    _disjoint("adjust", [("out", out), ("workspace", tmp)], [("images", x)])
    if x.numel() == 0:
        return out
    fn, name = (_hip.lib().vrg_adjust_u8, "vrg_adjust_u8") if u8 else (_hip.lib().vrg_adjust_f32, "vrg_adjust_f32")
    _hip.check(fn(_hip.ptr(x), _hip.ptr(out), _hip.ptr(tmp) if tmp is not None else None, F, H, W, C.byref(terms),
                  _hip.current_stream()), name)
    return out


# ------------------------------------------------------------------------------------------------
# uint8 BGR frames <-> fp32 RGB tensors (video I/O edge)
# ------------------------------------------------------------------------------------------------

@_on_device
def frames_u8_to_f32(frames_bgr: torch.Tensor) -> torch.Tensor:
    """``[F,H,W,3]`` uint8 B,G,R on the GPU -> fp32 R,G,B in [0,1] (``/ 255.0``)."""
    x = _check_frames(frames_bgr, "frames", channels=3, dtype=torch.uint8)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if x.numel():
        _hip.check(_hip.lib().vrg_u8bgr_to_f32rgb(_hip.ptr(x), _hip.ptr(out), x.numel() // 3, _hip.current_stream()),
                   "vrg_u8bgr_to_f32rgb")
    return out


@_on_device
def f32_to_frames_u8(images: torch.Tensor) -> torch.Tensor:
    """fp32 R,G,B -> ``clip(x * 255, 0, 255)`` truncated to uint8, B,G,R order."""
    x = _check_frames(images, channels=3)
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if x.numel():
        _hip.check(_hip.lib().vrg_f32rgb_to_u8bgr(_hip.ptr(x), _hip.ptr(out), x.numel() // 3, _hip.current_stream()),
                   "vrg_f32rgb_to_u8bgr")
    return out


# ------------------------------------------------------------------------------------------------
# colour match
# ------------------------------------------------------------------------------------------------

def _stats_scratch(frames: int, device) -> torch.Tensor:
    nbytes = int(_hip.lib().vrg_lab_stats_scratch_bytes(frames))
    return torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=device)


@_on_device
def lab_stats(images: torch.Tensor, cm_math=None) -> torch.Tensor:
    """Per-frame Lab statistics as fp64 ``[F, 3, 3]`` = (n, mean, M2) per channel L,a,b."""
    x = _check_frames(images, channels=3)
    F, H, W, _ = x.shape
    stats = torch.empty((F, 3, 3), dtype=torch.float64, device=x.device)
    if F == 0:
        return stats
    scratch = _stats_scratch(F, x.device)
    _hip.check(_hip.lib().vrg_lab_stats_f32(_hip.ptr(x), F, H, W, _hip.ptr(stats), _hip.ptr(scratch), _cm_math(cm_math),
                                           _hip.current_stream()), "vrg_lab_stats_f32")
    return stats


@_on_device
def finalize_stats(stats: torch.Tensor) -> torch.Tensor:
    """(n, mean, M2) fp64 -> fp32 ``[F, 3, 2]`` = (mean, unbiased std + 1e-5) (nodes.py:99-100, 109-110)."""
    F = stats.shape[0]
    ms = torch.empty((F, 3, 2), dtype=torch.float32, device=stats.device)
    if F:
        _hip.check(_hip.lib().vrg_lab_stats_finalize(_hip.ptr(stats), _hip.ptr(ms), F, _hip.current_stream()),
                   "vrg_lab_stats_finalize")
    return ms


def _chunk_runs(frames: int, chunks) -> list:
    """`chunks`: frames per reference call (an int: the node's batch_size, last call = remainder) or the explicit list of call
    sizes.  Returns [(first_frame, frames, call_size)] runs of equally sized calls."""
    if isinstance(chunks, int):
        if chunks < 1:
            raise ValueError("colour-match chunk must be >= 1")
        return [(0, frames, chunks)] if frames else []
    sizes = [int(c) for c in chunks]
    if any(c < 1 for c in sizes) or sum(sizes) != frames:
        raise ValueError("colour-match chunk sizes must be positive and add up to the number of frames")
    runs, f = [], 0
    for c in sizes:
        if runs and runs[-1][2] == c and runs[-1][1] % c == 0:
            runs[-1] = (runs[-1][0], runs[-1][1] + c, c)
        else:
            runs.append((f, c, c))
        f += c
    return runs


_TS_CHECKED = {}             # device index -> True (replay == this torch build) / False


def _selfcheck_planes(device):
    """Probe tensors of the self-check: small planes for the generic (one workgroup per plane) form -- an aligned one and one whose
    H*W is odd, so that planes start off a vector boundary -- and, for the whole-frame forms the video-sized calls take, one plane
    per batch_size class (block (256,2) for 1, (128,4) for 2, (64,8) for >= 3) shaped like a 4K row band: long enough (>= 2 rounds of
    2048 pixels plus a ragged tail) to run the same thread loop, lane tree and warp tree as a full frame."""
    g = torch.Generator().manual_seed(20260926)
    small = (torch.rand((3, 24, 40, 3), generator=g) * 100.0 - 30.0).to(device)
    odd = (torch.rand((4, 23, 41, 3), generator=g) * 100.0 - 30.0).to(device)
    band = (torch.rand((6, 4, 3840, 3), generator=g) * 120.0 - 40.0).to(device)          # H*W = 15,360: 7.5 rounds
    many = (torch.rand((66, 4, 3840, 3), generator=g) * 120.0 - 40.0).to(device)        # > 64 frames: the one-workgroup-per-frame form
    return [(small, (1, 3)), (odd, (1, 2, 4)), (band, (1, 2, 3, 6)), (many, (1,))]


def device_stats_selfcheck(device, force: bool = False) -> bool:
    """Once per device and process (a few ms): the replayed reductions against THIS torch build's `mean` / `std` over the call
    geometries that matter -- every batch_size class of the whole-frame kernels, an unaligned plane, ragged last calls.  The replay
    follows torch 2.10.0+rocm7.0's reduce_kernel; another build may pick another geometry or contraction -- then the node is no longer
    bit-equal to the reference run under that build (it stays within the statistics band, ~20 ulp(1.0)).  Returns whether the replay
    matched; a mismatch warns once and is reported by `device_stats_status()` so that a host can surface it next to its results."""
    key = torch.device(device).index
    if key is None:
        key = torch.cuda.current_device()
    with _STATE_LOCK:
        if key in _TS_CHECKED and not force:
            return _TS_CHECKED[key]
    ok = True
    with torch.cuda.device(key):
        for probe, call_sizes in _selfcheck_planes(torch.device("cuda", key)):
            F, H, W, _ = probe.shape
            for calls in call_sizes:
                want = []
                for i in range(0, F, calls):
                    t = probe[i:i + calls].permute(0, 3, 1, 2).contiguous()
                    want.append(torch.stack([t.mean(dim=[2, 3]), t.std(dim=[2, 3])], dim=-1))
                want = torch.cat(want, dim=0)
                got = torch.empty((F, 3, 2), dtype=torch.float32, device=probe.device)
                _hip.check(_hip.lib().vrg_lab_stats_torch_f32(_hip.ptr(probe), F, H, W, calls, _hip.ptr(got), _f32(0.0), _hip.current_stream()),
                           "vrg_lab_stats_torch_f32")
                ok = ok and torch.equal(got, want)
                # the forms production takes (lab_stats_device): with a scratch buffer, the throughput entry and the latency entry
                # (one accumulator per lane, <= 2 frames per call)
                nbytes = int(_hip.lib().vrg_lab_stats_torch_scratch_bytes(F))
                if nbytes:
                    scratch = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.float32, device=probe.device)
                    for name in ("vrg_lab_stats_torch_ws_f32", "vrg_lab_stats_torch_lat_f32"):
                        got2 = torch.empty((F, 3, 2), dtype=torch.float32, device=probe.device)
                        _hip.check(getattr(_hip.lib(), name)(_hip.ptr(probe), F, H, W, calls, _hip.ptr(got2), _f32(0.0), _hip.ptr(scratch), nbytes,
                                                             _hip.current_stream()), name)
                        ok = ok and torch.equal(got2, want)
    with _STATE_LOCK:
        first = key not in _TS_CHECKED
        _TS_CHECKED[key] = ok
    if not ok and first:
        import warnings
        warnings.warn(f"comfyui-vrgamedevgirl_amd: torch {torch.__version__} reduces mean()/std() in another order than the one this "
                      "library replays (torch 2.10.0+rocm7.0): ColorMatchToReference stays within a few ulp of the reference instead of "
                      "bit-equal to it (ops.device_stats_status())", RuntimeWarning)
    return ok


def device_stats_status(device=None) -> dict:
    """What a host can log next to a colour-match result: which statistics the default policy uses on `device` and whether the
    replay of torch's reductions was verified against this torch build in this process."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if not device_stats_supported(device):
        return {"cm_stats": "fp64", "bit_equal_to_torch": False, "reason": "fewer than 100 CUs: torch's reduction geometry is not replayed"}
    ok = device_stats_selfcheck(device)
    return {"cm_stats": "device", "bit_equal_to_torch": bool(ok), "torch": torch.__version__,
            "reason": None if ok else "this torch build reduces in another order than the replayed one (torch 2.10.0+rocm7.0)"}


def _device_stats_selfcheck(device) -> None:
    device_stats_selfcheck(device)
    if os.environ.get("VRGDG_SELFCHECK", "1") != "0":
        toolchain_selfcheck(device)


# ------------------------------------------------------------------------------------------------
# Toolchain coupling, checked at first use: two fast forms rest on measurements of ONE ROCm build --
#   * dev_pow_ziv's rounding test carries half-widths calibrated against this build's ocml logarithm (tools/ziv_calibration.json);
#     another ocml could make it accept a wrongly rounded power;
#   * the steady rows of the wave march issue their LUT gathers as inline-assembly LDS-DMA with hand-counted `vmcnt` waits
#     (csrc/vrg_march.hip); a compiler that schedules other memory operations between them breaks the count.
# The first colour match / fused chain on a device compares (a) dev_pow_ziv at its three call sites with torch.pow -- ocml's powf --
# on that device over 3 x 2^20 arguments of the call sites' domains, the neighbourhood of 1.0 included, and (b) the march with the
# LDS-tile kernels (vrg_chain_desc.variant 2 against 1) on a geometry whose rows are steady.  (b) failing switches the automatic
# choice to the tile kernels for the process (same results, slower) and warns; (a) failing warns and is reported by
# `toolchain_status()` -- the powers then differ from the reference's by an ulp in rare lanes.
# ------------------------------------------------------------------------------------------------
_TOOLCHAIN = {}              # device index -> {"pow": bool, "march": bool}
_POW_SITES = ((12, 2.4, 0.0625, 2.0), (13, 1.0 / 2.4, 0.0031308, 4.0), (14, 1.0 / 3.0, 0.008856, 4.0))     # (vrg_debug_cm_math op, y, domain) per call site


def _pow_probe_arguments(lo: float, hi: float, device) -> torch.Tensor:
    a, b = np.float32(lo).view(np.uint32), np.float32(hi).view(np.uint32)
    n = 1 << 20
    bits = (int(a) + (np.arange(n, dtype=np.uint64) * (int(b) - int(a)) // (n - 1))).astype(np.uint32)
    near1 = (np.float32(1.0).view(np.uint32) + np.arange(-4096, 4096, dtype=np.int64)).astype(np.uint32)      # saturated pixels: x ~ 1
    return torch.from_numpy(np.concatenate([bits, near1]).view(np.float32)).to(device)


_TOOLCHAIN_RUNNING = set()   # device indices whose probes are running right now (on whatever thread)


def toolchain_selfcheck(device, force: bool = False) -> dict:
    key = torch.device(device).index
    if key is None:
        key = torch.cuda.current_device()
    with _STATE_LOCK:
        if key in _TOOLCHAIN and not force:
            return _TOOLCHAIN[key]
        if key in _TOOLCHAIN_RUNNING:
            # the probes below run fused_chain themselves (re-entrancy), and another host thread may arrive while they run: both get the
            # SAFE answer for this one call -- the tile kernels, same bits -- and nothing is recorded before the probes have finished
            return {"pow": True, "march": False}
        if torch.cuda.is_current_stream_capturing():
            return {"pow": True, "march": False}          # the probes synchronise: not inside a graph capture; checked at the next plain call
        _TOOLCHAIN_RUNNING.add(key)
    dev = torch.device("cuda", key)
    res = {"pow": True, "march": True}
    try:
        with torch.cuda.device(key):
            lib = _hip.lib()
            for site, (op, y, lo, hi) in enumerate(_POW_SITES):
                x = _pow_probe_arguments(lo, hi, dev)
                got = torch.empty_like(x)
                _hip.check(lib.vrg_selfcheck_pow_f32(_hip.ptr(x), _hip.ptr(got), x.numel(), site, _hip.current_stream()), "vrg_selfcheck_pow_f32")
                res["pow"] = res["pow"] and bool(torch.equal(got, torch.pow(x, y)))
            g = torch.Generator(device=dev).manual_seed(20260926)
            frames = torch.rand((2, 512, 512, 3), generator=g, device=dev)       # one RNG chunk of 2 frames: full-grid Philox geometry, steady rows
            axis = np.linspace(0.0, 1.0, 33, dtype=np.float32)
            bb, gg, rr = np.meshgrid(axis, axis, axis, indexing="ij")             # [b][g][r] -> (r, g, b): a smooth non-identity grade
            table = np.stack([rr ** 1.25, 0.9 * gg + 0.1 * bb, bb * bb], axis=-1).astype(np.float32)
            lut = upload_lut({"lut": torch.from_numpy(table), "domain_min": torch.zeros(3), "domain_max": torch.ones(3)}, dev)
            outs = []
            for variant in (2, 1):
                gen = torch.Generator(device=dev).manual_seed(7)
                spec = ChainSpec(grain=(0.04, 0.5, 2), lut=(lut, 10.0), sharpen=("unsharp", 0.5, False), variant=variant)
                outs.append(fused_chain(frames, spec, generator=gen))
            res["march"] = bool(torch.equal(outs[0], outs[1]))
    except Exception as exc:             # a probe that cannot run (out of memory, a launch error) proves nothing: take the safe kernels, say so
        res = {"pow": False, "march": False, "error": f"{type(exc).__name__}: {exc}"}
    finally:
        with _STATE_LOCK:
            _TOOLCHAIN_RUNNING.discard(key)
            _TOOLCHAIN[key] = res
    if not (res["pow"] and res["march"]):
        import warnings
        what = []
        if "error" in res:
            what.append(f"the first-use self-check could not run ({res['error']}): fused chains take the tile kernels in this process")
        else:
            if not res["march"]:
                what.append("the wave-march kernel disagrees with the tile kernels (hand-counted waits of its LDS-DMA gathers): fused chains take the "
                            "tile kernels in this process")
            if not res["pow"]:
                what.append("dev_pow_ziv disagrees with this ROCm's powf (its rounding test is calibrated against ROCm 7.0's ocml): colour match may "
                            "differ from the reference by an ulp in rare pixels")
        warnings.warn("comfyui-vrgamedevgirl_amd: built or run with another toolchain than the one its fast forms were measured on -- "
                      + "; ".join(what) + " (ops.toolchain_status())", RuntimeWarning)
    return res


def toolchain_status(device=None) -> dict:
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    res = toolchain_selfcheck(device)
    return {"pow_equals_ocml": res["pow"], "march_equals_tile_kernels": res["march"], "error": res.get("error"), "hip": torch.version.hip,
            "torch": torch.__version__}


def _auto_variant(device) -> int:
    """vrg_chain_desc.variant for the automatic choice: 0, or 1 (tile kernels) where the march failed its self-check on this device."""
    if os.environ.get("VRGDG_SELFCHECK", "1") == "0":
        return 0
    return 0 if toolchain_selfcheck(device)["march"] else 1


@_on_device
def lab_stats_device(lab: torch.Tensor, chunks=1, eps: float = 1e-5, out: Optional[torch.Tensor] = None, latency_form: bool = False) -> torch.Tensor:
    """fp32 ``[F, 3, 2]`` = (mean, unbiased std + eps) of an interleaved Lab image ``[F,H,W,3]`` with the BITS
    ``lab.mean(dim=[2,3])`` / ``lab.std(dim=[2,3]) + 1e-5`` have when torch evaluates them on this GPU for ``chunks`` frames per
    call (nodes.py:99-100, 109-110).  include/vrgdg_hip.h: vrg_lab_stats_torch_f32.  `latency_form`: allow the one-accumulator-per-lane
    kernels for calls of at most two frames (vrg_lab_stats_torch_lat_f32) -- faster on an otherwise idle GPU, slower beside a full-size
    pass; same bits."""
    x = _check_frames(lab, "lab", channels=3)
    F, H, W, _ = x.shape
    ms = out if out is not None else torch.empty((F, 3, 2), dtype=torch.float32, device=x.device)
    if out is not None:
        _check_side(out, "statistics output", x, (3, 2))
        if int(out.shape[0]) != F:
            raise ValueError("statistics output must hold one [3, 2] record per frame")
        _disjoint("lab_stats_device", [("out", out)], [("lab", x)])
    fe = H * W * 3
    if F:
        _device_stats_selfcheck(x.device)
    lib = _hip.lib()
    for f0, nf, c in _chunk_runs(F, chunks):
        nbytes = int(lib.vrg_lab_stats_torch_scratch_bytes(nf))      # small batches: the half-block form wants a scratch buffer (0: another form)
        scratch = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.float32, device=x.device) if nbytes else None
        entry = lib.vrg_lab_stats_torch_lat_f32 if latency_form else lib.vrg_lab_stats_torch_ws_f32
        _hip.check(entry(C.c_void_p(x.data_ptr() + f0 * fe * 4), nf, H, W, c, C.c_void_p(ms.data_ptr() + f0 * 24), _f32(eps),
                         _hip.ptr(scratch) if scratch is not None else None, nbytes, _hip.current_stream()),
                   "vrg_lab_stats_torch_lat_f32" if latency_form else "vrg_lab_stats_torch_ws_f32")
    return ms


#: steps of at most this many frames take the latency form of the reference frame's statistics (measured: 4 / 8 / 16 frames per step
#: 2.0 / 2.8 / 4.5 ms against 2.4 / 3.4 / 5.0; 32 / 64 frames 8.4 / 16.8 against 8.0 / 14.4 -- profiles/r04_frames_table_*.json)
SMALL_STEP_FRAMES = 16


def reference_stats(reference_image: torch.Tensor, cm_math=None, cm_stats=None, step_frames: Optional[int] = None) -> torch.Tensor:
    """fp32 ``[R, 3, 2]`` (mean, std + 1e-5) of the reference frame(s) (nodes.py:98-100): one reduction call over the whole
    reference batch with the device statistics.  `step_frames`: how many frames the step these statistics belong to processes, if the
    caller knows -- small steps leave the GPU idle and take the latency form of the reduction (SMALL_STEP_FRAMES)."""
    ref = _check_frames(reference_image, "reference_image", channels=3)
    if _cm_stats(cm_stats, cm_math, ref.device) == "fp64":
        return finalize_stats(lab_stats(ref, cm_math))
    lab = torch.empty_like(ref)
    Rn, H, W, _ = ref.shape
    if Rn:
        d = _chain_desc(ChainSpec(cm_math=cm_math), None, [], ref)
        _hip.check(_hip.lib().vrg_chain_stats_lab_f32(_hip.ptr(ref), _hip.ptr(lab), Rn, H, W, C.byref(d), None, None, _hip.current_stream()),
                   "vrg_chain_stats_lab_f32")        # the Lab image only
    return lab_stats_device(lab, max(int(Rn), 1), latency_form=step_frames is not None and int(step_frames) <= SMALL_STEP_FRAMES)


_SIDE_STREAMS = {}


def _side_stream(device) -> "torch.cuda.Stream":
    """One extra stream per device for work that is off the critical path of the frame passes: the statistics of the reference frame.
    HIGH priority: its kernels are a handful of latency-bound workgroups; on a normal-priority stream they queue behind the thousands of
    workgroups of pass 1 (measured: 32 x 4K frames per step 11.7 ms = the passes' 9.4 ms + the reference statistics' 2.2 ms, nothing
    hidden), a high-priority queue lets the dispatcher slot them in as soon as they are submitted."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    with _STATE_LOCK:
        st = _SIDE_STREAMS.get(key)
        if st is None:
            st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=key, priority=-1)
    return st


@_on_device
def reference_stats_async(reference_image: torch.Tensor, cm_math=None, cm_stats=None, step_frames: Optional[int] = None):
    """reference_stats on the side stream: returns (ref_ms, event).  The reference frame's statistics are one latency-bound chain
    (16,200 dependent Welford updates per accumulator for a 4K frame: 1.5-2 ms on a handful of workgroups) that only the APPLY pass
    needs -- give `event` to ChainSpec.cm_ref_event and pass 1 of the batch runs meanwhile."""
    main = torch.cuda.current_stream()
    side = _side_stream(reference_image.device)
    side.wait_stream(main)                         # the reference frame may have been produced on the caller's stream
    with torch.cuda.stream(side):
        ref_ms = reference_stats(reference_image, cm_math, cm_stats, step_frames=step_frames)
        ev = torch.cuda.Event()
        ev.record(side)
    ref_ms.record_stream(main)
    reference_image.record_stream(side)
    return ref_ms, ev


def merge_stats(parts: torch.Tensor) -> torch.Tensor:
    """Chan/Golub/LeVeque merge of (n, mean, M2) triples along dim 0, in index order (deterministic):
    used to combine the slices of one reference frame reduced on different GPUs.  ``parts``: [R, ..., 3]."""
    acc = parts[0].clone()
    for r in range(1, parts.shape[0]):
        nb, mb, m2b = parts[r][..., 0], parts[r][..., 1], parts[r][..., 2]
        na, ma, m2a = acc[..., 0], acc[..., 1], acc[..., 2]
        n = na + nb
        delta = mb - ma
        mean = ma + delta * (nb / n)
        m2 = m2a + m2b + delta * delta * (na * nb / n)
        acc = torch.stack([n, mean, m2], dim=-1)
    return acc


@_on_device
def colormatch_apply(images: torch.Tensor, img_ms: torch.Tensor, ref_ms: torch.Tensor, match_strength: float,
                     cm_math=None) -> torch.Tensor:
    x = _check_frames(images, channels=3)
    F, H, W, _ = x.shape
    out = torch.empty_like(x)
    if F == 0:
        return out
    _check_side(ref_ms, "ref_ms", x, (3, 2))
    _check_side(img_ms, "img_ms", x, (3, 2))
    if int(img_ms.shape[0]) != F:
        raise ValueError(f"img_ms holds {int(img_ms.shape[0])} frames of statistics for {F} frames")
    R = int(ref_ms.shape[0])
    if R != 1 and F % R != 0:
        raise RuntimeError(f"The size of tensor a ({F}) must match the size of tensor b ({R}) at non-singleton dimension 0")
    _hip.check(_hip.lib().vrg_colormatch_apply_f32(_hip.ptr(x), _hip.ptr(out), F, H, W, _hip.ptr(img_ms), _hip.ptr(ref_ms), R,
                                                  _f32(match_strength), _f32(1.0 - match_strength), _cm_math(cm_math),
                                                  _hip.current_stream()),
               "vrg_colormatch_apply_f32")
    return out


@_on_device
def color_match(images: torch.Tensor, reference_image: torch.Tensor, match_strength: float,
                ref_ms: Optional[torch.Tensor] = None, cache_lab: bool = True, cm_math=None, cm_chunk=1, cm_stats=None,
                ref_event=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-frame Lab mean/std transfer to the reference frame(s) (nodes.py:91-124).  Two passes over HBM:
    statistics (which also stores the Lab image when cache_lab) and apply; see fused_chain.  `cm_chunk`: frames per statistics
    call of the reference (the node's batch_size, or the list of call sizes) -- it shapes the device statistics like it shapes
    the reference's (CM_STATS).  `ref_event`: the event of reference_stats_async when `ref_ms` comes from it."""
    x = _check_frames(images, channels=3)
    stats = _cm_stats(cm_stats, cm_math, x.device)
    if out is not None:
        out = _out_like(x, out, "color_match", "images")                 # refused before anything is launched
    if ref_ms is None:
        ref_ms = reference_stats(reference_image.to(x.device), cm_math, stats)
    if cache_lab or stats == "device":
        return fused_chain(x, ChainSpec(colormatch=(ref_ms, match_strength), cm_math=cm_math, cm_chunk=cm_chunk, cm_stats=stats,
                                        cm_ref_event=ref_event), out=out)
    if ref_event is not None:
        torch.cuda.current_stream().wait_event(ref_event)
    img_ms = finalize_stats(lab_stats(x, cm_math))
    res = colormatch_apply(x, img_ms, ref_ms, match_strength, cm_math)
    if out is not None:
        out.copy_(res)
        return out
    return res


# ------------------------------------------------------------------------------------------------
# fused chain
# ------------------------------------------------------------------------------------------------

@dataclass
class ChainSpec:
    """grain -> LUT -> colour match -> sharpen; None disables a stage."""
    grain: Optional[tuple] = None          # (intensity, saturation_mix, chunk_frames)
    lut: Optional[tuple] = None            # (DeviceLut, strength 0..10)
    colormatch: Optional[tuple] = None     # (ref_ms [R,3,2] fp32 device tensor, match_strength)
    sharpen: Optional[tuple] = None        # (op name, strength, zero_border)
    variant: int = 0
    cm_math: object = None                 # None = default_cm_math(); "device" / "fast" (colour-match arithmetic policy)
    cm_chunk: object = 1                   # frames per statistics call of the reference (batch_size), or the list of call sizes
    cm_stats: object = None                # None = by cm_math; "device" (torch's reductions, bit for bit) / "fp64" (CM_STATS)
    cm_ref_event: object = None            # torch.cuda.Event after which ref_ms is valid (reference_stats_async); waited for before pass 2


def _chain_desc(spec: ChainSpec, plan: Optional[NoisePlan], keep, like: Optional[torch.Tensor] = None):
    d = _hip.ChainDesc()
    stages = 0
    if spec.grain is not None:
        I, s, _ = spec.grain
        stages |= _hip.STAGE_GRAIN
        d.intensity, d.sat, d.one_minus_sat = _f32(I), _f32(s), _f32(1.0 - s)
        if isinstance(plan, NoisePlan):         # (a SplitNoisePlan travels beside the descriptor: _split_records)
            d.noise = plan.desc()
    if spec.lut is not None:
        lut, strength = spec.lut
        mode, B, omB = blend_terms(strength)
        if mode != 0:
            if like is not None:
                _check_side(lut.table, "LUT record table", like)
            stages |= _hip.STAGE_LUT
            d.lut = lut.table.data_ptr(); d.lut_size = lut.size
            d.domain_min = _F3(*lut.domain_min); d.domain_max = _F3(*lut.domain_max)
            d.blend_mode, d.blend, d.one_minus_blend = mode, B, omB
            keep.append(lut.table)
    if spec.colormatch is not None:
        ref_ms, k = spec.colormatch
        if like is not None:
            _check_side(ref_ms, "colormatch reference statistics", like, (3, 2))
        stages |= _hip.STAGE_COLORMATCH
        d.ref_ms = ref_ms.data_ptr(); d.ref_frames = int(ref_ms.shape[0])
        d.k, d.one_minus_k = _f32(k), _f32(1.0 - k)
        keep.append(ref_ms)
    if spec.sharpen is not None:
        op, strength, zero = spec.sharpen
        stages |= _hip.STAGE_SHARPEN
        d.stencil_op = _STENCIL[op]
        d.border = _hip.BORDER_ZERO if zero else _hip.BORDER_REPLICATE
        d.strength = _f32(strength)
    d.stages = stages
    d.variant = spec.variant
    d.cm_math = _cm_math(spec.cm_math)
    return d


@_on_device
def chain_stats(images: torch.Tensor, spec: ChainSpec, generator: Optional[torch.Generator] = None, plans=None,
                lab_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Colour-match pass 1 on its own: fp64 (n, mean, M2) of Lab(grain -> LUT (images)) per frame, optionally
    storing that Lab image.  (Test / analysis entry; fused_chain runs the same kernels.)"""
    x = _check_frames(images, channels=3)
    F, H, W, _ = x.shape
    fe = H * W * 3
    segments = [(0, F, None)]
    if spec.grain is not None:
        if plans is None:
            plans = plan_noise(F, fe, spec.grain[2], x.device, generator)
        segments = _plan_segments(plans, F, "chain_stats")
        if any(_split_records(plan, fe) is None for _f0, _nf, plan in segments):
            # a frame that meets more leaves than a launch takes (split_launches): grain with its noise in memory, then the rest
            grained = film_grain(x, spec.grain[0], spec.grain[1], spec.grain[2], plans=plans)
            import dataclasses
            return chain_stats(grained, dataclasses.replace(spec, grain=None), lab_out=lab_out)
    stats = torch.empty((F, 3, 3), dtype=torch.float64, device=x.device)
    lib = _hip.lib()
    for f0, nf, plan in segments:
        keep = []
        d = _chain_desc(ChainSpec(grain=spec.grain, lut=spec.lut, variant=spec.variant, cm_math=spec.cm_math), plan, keep, x)
        nbytes = int(lib.vrg_chain_stats_scratch_bytes(nf, H, W, C.byref(d))) if isinstance(plan, (NoisePlan, type(None))) else \
            int(lib.vrg_lab_stats_scratch_bytes(nf))
        scratch = torch.empty((max(nbytes, 8) + 7) // 8, dtype=torch.float64, device=x.device)
        for g0, n, rec in _split_records(plan, fe) or [(0, nf, None)]:
            src = C.c_void_p(x.data_ptr() + (f0 + g0) * fe * 4)
            dst = C.c_void_p(lab_out.data_ptr() + (f0 + g0) * fe * 4) if lab_out is not None else C.c_void_p(0)
            sts = C.c_void_p(stats.data_ptr() + (f0 + g0) * 72)
            if rec is None:
                _hip.check(lib.vrg_chain_stats_lab_f32(src, dst, n, H, W, C.byref(d), sts, _hip.ptr(scratch), _hip.current_stream()),
                           "vrg_chain_stats_lab_f32")
            else:
                _hip.check(lib.vrg_chain_stats_lab_split_f32(src, dst, n, H, W, C.byref(d), C.byref(rec), sts, _hip.ptr(scratch),
                                                            _hip.current_stream()), "vrg_chain_stats_lab_split_f32")
    return stats



@_on_device
def fused_chain(images: torch.Tensor, spec: ChainSpec, generator: Optional[torch.Generator] = None, plans=None,
                out: Optional[torch.Tensor] = None, kernel_events: Optional[list] = None,
                lab_workspace: Optional[torch.Tensor] = None, cache_lab: bool = True) -> torch.Tensor:
    """One pass over HBM for grain -> LUT -> colour match -> 3x3 sharpen (colour match adds one statistics
    pass).  Bit-identical to applying the stand-alone operators in that order.

    `out` may supply the destination (bench: no allocation in the timed region); `kernel_events`, if a list,
    receives (name, start, stop, frames) tuples -- HipEvent pairs on the current stream bracketing the
    statistics pass ("stats") and the fused apply pass ("apply") of every segment.

    Chains with a colour-match stage run as two passes: (1) grain -> LUT -> Lab, reduced to per-frame statistics
    and (cache_lab=True) stored as a Lab image, (2) match -> Lab->RGB -> sharpen on that Lab image.  With
    cache_lab=False pass 2 re-evaluates grain/LUT/Lab from the input instead (36 B/px instead of 48 B/px of HBM
    traffic, but the gathers and powers twice); both forms give bit-identical results.  `lab_workspace` may
    supply the fp32 buffer (same shape as images).  With the device statistics (CM_STATS, the default) the statistics are torch's
    own reductions over the stored Lab image, per `spec.cm_chunk` frames: that form always keeps the Lab image (cache_lab is moot)."""
    u8 = isinstance(images, torch.Tensor) and images.dtype == torch.uint8       # decoded BGR frames (video routes)
    x = _check_frames(images, channels=3, dtype=torch.uint8 if u8 else torch.float32)
    if u8 and spec.colormatch is not None:
        raise ValueError("uint8 frames: colour match is not part of the video routes (convert to fp32 first)")
    esize = 1 if u8 else 4
    F, H, W, _ = x.shape
    out = _checked_out(out, x.shape, x.dtype, x.device, "fused_chain")
    _disjoint("fused_chain", [("out", out), ("lab_workspace", lab_workspace)], [("images", x)])
    if F == 0:
        return out
    fe = H * W * 3
    segments = [(0, F, None)]
    if spec.grain is not None:
        if plans is None:
            plans = plan_noise(F, fe, spec.grain[2], x.device, generator)
        segments = _plan_segments(plans, F, "fused_chain")
        # RNG chunks that torch itself splits (SplitNoisePlan) run inside the fused launches like any other: the kernels look every
        # element's leaf up (vrg_fused_chain_split_*).  With a colour match the grain sits in pass 1, and pass 2 always starts from its
        # Lab image: the recomputing form (cache_lab=False) gives the same bits and would need split forms of the colour-match kernels.
        if any(isinstance(plan, SplitNoisePlan) for _f0, _nf, plan in segments):
            cache_lab = True
        if any(_split_records(plan, fe) is None for _f0, _nf, plan in segments):
            # a single frame that meets more leaves than a launch takes (1.8 G elements at the real limit, split_launches): grain as its
            # own pass with that frame's noise in memory (_film_grain_oversize), then the rest of the chain
            import dataclasses
            if u8:
                res = fused_chain(frames_u8_to_f32(x), spec, plans=plans, kernel_events=kernel_events)
                out.copy_(f32_to_frames_u8(res))
                return out
            grained = film_grain(x, spec.grain[0], spec.grain[1], spec.grain[2], plans=plans)
            rest = dataclasses.replace(spec, grain=None)
            if rest.lut is None and rest.colormatch is None and rest.sharpen is None:
                out.copy_(grained)
                return out
            return fused_chain(grained, rest, out=out, kernel_events=kernel_events, lab_workspace=lab_workspace, cache_lab=cache_lab)
    lib = _hip.lib()
    st = _hip.current_stream()
    if spec.variant == 0:
        v = _auto_variant(x.device)            # first use on a device: the toolchain self-check (a few ms, once)
        if v:
            import dataclasses
            spec = dataclasses.replace(spec, variant=v)
    device_stats = spec.colormatch is not None and _cm_stats(spec.cm_stats, spec.cm_math, x.device) == "device"
    lab_full = img_ms_full = None
    if device_stats:
        # The reference's statistics are torch reductions over each batch_size call: they need the Lab image of WHOLE calls, so
        # pass 1 runs for every segment first, then the reductions over the batch, then pass 2 (cache_lab is implied).
        # (Four schedules that overlap the passes over frame ranges were built and measured slower in round 3; they live in
        # tools/experiments/ with their A/B logs, LABNOTES.md section "schedules".)
        if lab_workspace is not None:
            if lab_workspace.shape != x.shape or lab_workspace.dtype != torch.float32 or not lab_workspace.is_contiguous():
                raise ValueError("lab_workspace must be a contiguous float32 tensor shaped like images")
            lab_full = lab_workspace
        else:
            lab_full = torch.empty((F, H, W, 3), dtype=torch.float32, device=x.device)
        for f0, nf, plan in segments:
            keep = []
            d = _chain_desc(spec, plan, keep, x)
            if kernel_events is not None:
                s0, s1 = HipEvent(), HipEvent()
                s0.record()
            for g0, n, rec in _split_records(plan, fe) or [(0, nf, None)]:           # the Lab image only
                src, dst = C.c_void_p(x.data_ptr() + (f0 + g0) * fe * 4), C.c_void_p(lab_full.data_ptr() + (f0 + g0) * fe * 4)
                if rec is None:
                    _hip.check(lib.vrg_chain_stats_lab_f32(src, dst, n, H, W, C.byref(d), None, None, st), "vrg_chain_stats_lab_f32")
                else:
                    _hip.check(lib.vrg_chain_stats_lab_split_f32(src, dst, n, H, W, C.byref(d), C.byref(rec), None, None, st),
                               "vrg_chain_stats_lab_split_f32")
            if kernel_events is not None:
                s1.record()
                kernel_events.append(("stats", s0, s1, nf))
        if kernel_events is not None:
            t0, t1 = HipEvent(), HipEvent()
            t0.record()
        img_ms_full = lab_stats_device(lab_full, spec.cm_chunk)
        if kernel_events is not None:
            t1.record()
            kernel_events.append(("tstats", t0, t1, F))
    if spec.colormatch is not None and spec.cm_ref_event is not None:
        torch.cuda.current_stream().wait_event(spec.cm_ref_event)          # reference_stats_async: ref_ms is valid from here on
    for f0, nf, plan in segments:
        keep = []
        d = _chain_desc(spec, plan, keep, x)
        if d.stages == 0:
            out[f0:f0 + nf] = x[f0:f0 + nf]
            continue
        src = C.c_void_p(x.data_ptr() + f0 * fe * esize)
        dst = C.c_void_p(out.data_ptr() + f0 * fe * esize)
        if d.stages & _hip.STAGE_COLORMATCH:
            if d.ref_frames != 1 and (nf % d.ref_frames or f0 % d.ref_frames):
                raise RuntimeError("reference_image batch must be 1 or divide the frame batch")
            if device_stats:
                src = C.c_void_p(lab_full.data_ptr() + f0 * fe * 4)
                d.stages = (d.stages & _hip.STAGE_SHARPEN) | _hip.STAGE_COLORMATCH | _hip.STAGE_FROM_LAB
                d.img_ms = img_ms_full.data_ptr() + f0 * 24
            else:
                stats = torch.empty((nf, 3, 3), dtype=torch.float64, device=x.device)
                nbytes = int(lib.vrg_chain_stats_scratch_bytes(nf, H, W, C.byref(d)))        # (at least vrg_lab_stats_scratch_bytes: the split form's)
                scratch = torch.empty((max(nbytes, 8) + 7) // 8, dtype=torch.float64, device=x.device)
                if kernel_events is not None:
                    s0, s1 = HipEvent(), HipEvent()
                    s0.record()
                if isinstance(plan, SplitNoisePlan):           # (cache_lab: set above)
                    lab = lab_workspace[f0:f0 + nf] if lab_workspace is not None else torch.empty((nf, H, W, 3), dtype=torch.float32, device=x.device)
                    if lab_workspace is not None and (lab_workspace.shape != x.shape or lab_workspace.dtype != torch.float32 or not lab_workspace.is_contiguous()):
                        raise ValueError("lab_workspace must be a contiguous float32 tensor shaped like images")
                    keep.append(lab)
                    for g0, n, rec in _split_records(plan, fe):
                        _hip.check(lib.vrg_chain_stats_lab_split_f32(C.c_void_p(x.data_ptr() + (f0 + g0) * fe * 4), C.c_void_p(lab.data_ptr() + g0 * fe * 4),
                                                                    n, H, W, C.byref(d), C.byref(rec), C.c_void_p(stats.data_ptr() + g0 * 72),
                                                                    _hip.ptr(scratch), st), "vrg_chain_stats_lab_split_f32")
                    src = C.c_void_p(lab.data_ptr())
                    d.stages = (d.stages & _hip.STAGE_SHARPEN) | _hip.STAGE_COLORMATCH | _hip.STAGE_FROM_LAB
                elif cache_lab:
                    if lab_workspace is not None:
                        if lab_workspace.shape != x.shape or lab_workspace.dtype != torch.float32 or not lab_workspace.is_contiguous():
                            raise ValueError("lab_workspace must be a contiguous float32 tensor shaped like images")
                        lab = lab_workspace[f0:f0 + nf]
                    else:
                        lab = torch.empty((nf, H, W, 3), dtype=torch.float32, device=x.device)
                    keep.append(lab)
                    _hip.check(lib.vrg_chain_stats_lab_f32(src, _hip.ptr(lab), nf, H, W, C.byref(d), _hip.ptr(stats), _hip.ptr(scratch), st),
                               "vrg_chain_stats_lab_f32")
                    src = C.c_void_p(lab.data_ptr())
                    d.stages = (d.stages & _hip.STAGE_SHARPEN) | _hip.STAGE_COLORMATCH | _hip.STAGE_FROM_LAB
                else:
                    _hip.check(lib.vrg_chain_stats_f32(src, nf, H, W, C.byref(d), _hip.ptr(stats), _hip.ptr(scratch), st),
                               "vrg_chain_stats_f32")
                if kernel_events is not None:
                    s1.record()
                    kernel_events.append(("stats", s0, s1, nf))
                img_ms = finalize_stats(stats)
                d.img_ms = img_ms.data_ptr()
                keep.append(img_ms)
        if kernel_events is not None:
            e0, e1 = HipEvent(), HipEvent()
            e0.record()
        if isinstance(plan, SplitNoisePlan) and (d.stages & _hip.STAGE_GRAIN):
            for g0, n, rec in _split_records(plan, fe):
                a, b = C.c_void_p(src.value + g0 * fe * esize), C.c_void_p(dst.value + g0 * fe * esize)
                if u8:
                    _hip.check(lib.vrg_fused_chain_split_u8(a, b, n, H, W, C.byref(d), C.byref(rec), st), "vrg_fused_chain_split_u8")
                else:
                    _hip.check(lib.vrg_fused_chain_split_f32(a, b, n, H, W, C.byref(d), C.byref(rec), st), "vrg_fused_chain_split_f32")
        elif u8:
            _hip.check(lib.vrg_fused_chain_u8(src, dst, nf, H, W, C.byref(d), st), "vrg_fused_chain_u8")
        else:
            _hip.check(lib.vrg_fused_chain_f32(src, dst, nf, H, W, C.byref(d), st), "vrg_fused_chain_f32")
        if kernel_events is not None:
            e1.record()
            kernel_events.append(("apply", e0, e1, nf))
    return out


def fused_stages(frames: torch.Tensor, first_frame: int, stages: dict, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What `_devices` runs when consecutive nodes of this pack were called on one another's results (deferred graph fusion): the
    recorded nodes -- ``stages[kind]`` for kind in grain / lut / colormatch / sharpen, each the parameters its node was called with -- as
    ONE fused chain over frames [first_frame, first_frame + n) of the ORIGINAL input.  Bit-identical to the nodes run one after the
    other (tests/test_gpu_parity.py): grain draws from the generator range its node reserved when it was called (``plans``, sliced per
    piece), the colour statistics are reduced over the node's batch_size calls (``calls_of``), the reference statistics come from the
    side stream they were queued on at call time (``ref_event``).  Reference call order: nodes.py:41-66 -> VRGDG_IV_Adjustments.py:345-361
    -> nodes.py:91-124 -> nodes.py:156-209."""
    n = int(frames.shape[0])
    g, l, c, sh = (stages.get(k) for k in ("grain", "lut", "colormatch", "sharpen"))
    spec = ChainSpec(grain=(g["I"], g["s"], g["step"]) if g else None,
                     lut=(l["lut"], l["strength"]) if l else None,
                     colormatch=(c["ref_ms"], c["k"]) if c else None,
                     sharpen=(sh["op"], sh["strength"], sh["zero"]) if sh else None,
                     cm_chunk=c["calls_of"](first_frame, n) if c else 1,
                     cm_ref_event=c["ref_event"] if c else None)
    plans = slice_plans(g["plans"], first_frame, n) if g else None
    return fused_chain(frames, spec, plans=plans, out=out)


# ------------------------------------------------------------------------------------------------
# timing helper (HIP events on the stream the kernels run on)
# ------------------------------------------------------------------------------------------------

class HipEvent:
    """A hipEvent_t on the kernels' stream.  Handles are pooled per process: creating and destroying an event costs a driver call each
    (bench.py brackets every pass of every step), recording a pooled one does not."""
    _pool = {}          # device index -> free handles (an event belongs to the device it was created on)

    def __init__(self):
        self._dev = torch.cuda.current_device()
        with _STATE_LOCK:
            free = HipEvent._pool.get(self._dev)
            self._ev = free.pop() if free else None
        if self._ev is None:
            self._ev = C.c_void_p()
            _hip.check(_hip.lib().vrg_event_create(C.byref(self._ev)), "vrg_event_create")

    def record(self):
        _hip.check(_hip.lib().vrg_event_record(self._ev, _hip.current_stream()), "vrg_event_record")

    def elapsed_ms(self, stop: "HipEvent") -> float:
        ms = C.c_float()
        _hip.check(_hip.lib().vrg_event_elapsed_ms(self._ev, stop._ev, C.byref(ms)), "vrg_event_elapsed_ms")
        return float(ms.value)

    def __del__(self):
        try:
            if self._ev:
                with _STATE_LOCK:
                    free = HipEvent._pool.setdefault(self._dev, [])
                    if len(free) < 256:
                        free.append(self._ev)
                        self._ev = None
                if self._ev:
                    _hip.lib().vrg_event_destroy(self._ev)
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# Reference sheets (reference VRGDG_LTXICIngredientsGrid.py and VRGDG_MusicVideoBuilderNodes.py:7169-7238): pictures quantised, resized
# with Pillow's LANCZOS and pasted as panels onto a coloured canvas, in two launches (csrc/vrg_sheet.hip, arithmetic
# csrc/vrg_sheet_math.hpp)
# ------------------------------------------------------------------------------------------------
SHEET_PANEL = _hip.record_dtype(_hip.SheetPanel)          # the record; the SheetPanel below is the caller's description of a panel
SHEET_FITS = ("contain_pad", "cover_crop", "resize")


@dataclass(frozen=True)
class SheetPanel:
    """One pasted picture: ``source`` indexes the sources, ``rect`` = (left, top, width, height) on the canvas, ``fit`` is "contain_pad" or
    "cover_crop" (or "resize": the picture resized to the rectangle itself, as the Builder sheets paste it), ``cell`` the (R, G, B) bytes
    around a contained picture, ``radius`` the corner radius (0: a plain paste; above 0 the
    paste goes under ``ImageDraw.rounded_rectangle``'s mask with radius min(radius, width // 2, height // 2))."""
    source: int
    rect: tuple
    fit: str = "contain_pad"
    cell: tuple = (0, 0, 0)
    radius: int = 0


def sheet_lanczos_table(n_in: int, n_out: int):
    """(ksize, the table of one axis as the kernels read it: bounds [n_out, 2] then weights [n_out, ksize], int32) of
    ``Image.resize(..., LANCZOS)``; host only, cached per (n_in, n_out)"""
    return pil_axis_table(_hip.PIL_FILTER_LANCZOS, n_in, n_out)


@functools.lru_cache(maxsize=512)
def rounded_spans(width: int, height: int, radius: int) -> np.ndarray:
    """[height, 2] int32: the first and last column that ``ImageDraw.rounded_rectangle((0, 0, width - 1, height - 1), radius, fill=255)``
    sets in every row of a ``width`` x ``height`` L mask (first > last: none) -- from Pillow itself, cached per (width, height, radius).
    Every row of that mask is one run; a 1 x 1 mask is empty."""
    from PIL import Image, ImageDraw
    if width < 1 or height < 1 or radius < 0:
        raise ValueError("rounded_spans: width and height must be at least 1, radius at least 0")
    mask = Image.new("L", (width, height), 0)
    ImageDraw.Draw(mask).rounded_rectangle((0, 0, width - 1, height - 1), radius=radius, fill=255)
    plane = np.asarray(mask) != 0
    any_set = plane.any(axis=1)
    first = plane.argmax(axis=1)
    last = width - 1 - plane[:, ::-1].argmax(axis=1)
    if int(plane.sum()) != int((last - first + 1)[any_set].sum()):
        raise RuntimeError("rounded_spans: a row of Pillow's rounded rectangle is not one run")
    spans = np.where(any_set[:, None], np.stack([first, last], axis=1), np.array([[1, 0]])).astype(np.int32)
    spans.setflags(write=False)
    return spans


#: what _refuse says for vrg_sheet_fit, vrg_sheet_plan and vrg_sheet_check (they return nothing but OK, BAD_ARG and UNSUPPORTED)
_SHEET_REFUSALS = ("invalid argument", "not supported: a side above 32767, or the taps of one column do not fit the staging buffer")


class SheetPlan:
    """The host side of one reference sheet: the vrg_sheet_panel records (``records``, without source pointers), the axis tables back to
    back (``tables``), the mask rows (``spans``), the size of the temp images and the grid of the first launch.  No device is needed.
    ``shapes``: (height, width, channels) per source."""

    def __init__(self, shapes, panels, canvas_size, background):
        lib = _host_lib()
        self.width, self.height = int(canvas_size[0]), int(canvas_size[1])
        if self.width < 1 or self.height < 1 or self.width > _hip.SHEET_MAX_SIDE or self.height > _hip.SHEET_MAX_SIDE:
            raise ValueError(f"reference sheet: the canvas must be 1 .. {_hip.SHEET_MAX_SIDE} pixels a side")
        self.background = _sheet_colour(background, "background")
        self.panels = [p if isinstance(p, SheetPanel) else SheetPanel(*p) for p in panels]
        rec = np.zeros(len(self.panels), dtype=SHEET_PANEL)
        tables, table_at, spans, span_at, n_ints, n_spans, tmp_bytes = [], {}, [], {}, 0, 0, 0
        fit = np.zeros(8, dtype=np.int32)
        for i, p in enumerate(self.panels):
            if not 0 <= int(p.source) < len(shapes):
                raise ValueError(f"reference sheet: panel {i} names source {p.source} of {len(shapes)}")
            if p.fit not in SHEET_FITS:
                raise ValueError(f"reference sheet: fit mode must be one of {SHEET_FITS}, got {p.fit!r}")
            sh, sw, sc = (int(v) for v in shapes[int(p.source)])
            left, top, w, h = (int(v) for v in p.rect)
            if sc == 2 or sc < 1:
                raise ValueError(f"reference sheet: a source has {sc} channels; 1, 3 or more are taken (Pillow refuses two as well)")
            if w < 1 or h < 1 or sw < 1 or sh < 1:
                raise ValueError("reference sheet: panels and sources must be at least 1 x 1")
            if p.fit == "resize":
                fit[:] = (w, h, 0, 0, w, h, 0, 0)
            else:
                _refuse(lib.vrg_sheet_fit(sw, sh, w, h, int(p.fit == "cover_crop"), C.c_void_p(fit.ctypes.data)), "vrg_sheet_fit", *_SHEET_REFUSALS)
            r = rec[i]
            r["src_h"], r["src_w"], r["channels"] = sh, sw, sc
            r["left"], r["top"], r["w"], r["h"] = left, top, w, h
            for name, v in zip(("new_w", "new_h", "win_x", "win_y", "pic_w", "pic_h", "pic_x", "pic_y"), fit):
                r[name] = int(v)
            if max(int(fit[0]), int(fit[1])) > _hip.SHEET_MAX_SIDE:
                raise RuntimeError(f"reference sheet: panel {i} resizes its source to more than {_hip.SHEET_MAX_SIDE} pixels a side")
            for axis, (n_in, n_out) in enumerate(((sw, int(fit[0])), (sh, int(fit[1])))):
                if n_in == n_out:
                    continue
                if (n_in, n_out) not in table_at:
                    ksize, table = sheet_lanczos_table(n_in, n_out)
                    table_at[(n_in, n_out)] = (n_ints, ksize)
                    tables.append(table)
                    n_ints += len(table)
                r["v_table" if axis else "h_table"], r["v_ksize" if axis else "h_ksize"] = table_at[(n_in, n_out)]
            r["cell"][:3] = _sheet_colour(p.cell, "cell colour")
            r["span_offset"] = -1
            if int(p.radius) > 0:
                key = (w, h, min(int(p.radius), w // 2, h // 2))
                if key not in span_at:
                    span_at[key] = n_spans
                    spans.append(rounded_spans(*key))
                    n_spans += h
                r["span_offset"] = span_at[key]
        self.tables = np.concatenate(tables) if tables else np.zeros(1, np.int32)
        self.table_ints = n_ints
        self.spans = np.concatenate(spans) if spans else np.zeros((1, 2), np.int32)
        self.n_spans = n_spans
        if len(rec):
            _refuse(lib.vrg_sheet_plan(C.c_void_p(rec.ctypes.data), len(rec), C.c_void_p(self.tables.ctypes.data), n_ints), "vrg_sheet_plan",
                    *_SHEET_REFUSALS)
        for r in rec:
            r["tmp_offset"] = tmp_bytes
            tmp_bytes += int(r["rows"]) * int(r["pic_w"]) * 3
        self.records, self.tmp_bytes = rec, tmp_bytes
        self.max_rows = int(rec["rows"].max()) if len(rec) else 0
        self.max_segments = int(((rec["pic_w"] + rec["cps"] - 1) // rec["cps"]).max()) if len(rec) else 0

    def check(self, records, byte_sources: bool):
        """vrg_sheet_check of `records` (this plan's, with their source pointers set) on the host"""
        records = np.ascontiguousarray(records)
        _refuse(_host_lib().vrg_sheet_check(C.c_void_p(records.ctypes.data), len(records), int(byte_sources), C.c_void_p(self.tables.ctypes.data),
                                            self.table_ints, self.n_spans, self.tmp_bytes), "vrg_sheet_check", *_SHEET_REFUSALS)


def _sheet_colour(value, name):
    c = tuple(int(v) for v in value)
    if len(c) != 3 or any(v < 0 or v > 255 for v in c):
        raise ValueError(f"reference sheet: {name} must be three bytes (R, G, B)")
    return c


def _sheet_sources(sources):
    out = []
    for i, s in enumerate(sources):
        s = _as_tensor(s)
        if not isinstance(s, torch.Tensor):
            raise ValueError(f"reference sheet: source {i} must be a tensor")
        if s.ndim == 4 and int(s.shape[0]) == 1:
            s = s[0]
        if s.ndim == 2:
            s = s.unsqueeze(-1)
        if s.ndim != 3:
            raise ValueError(f"reference sheet: source {i} must be one [height, width, channels] frame")
        if s.dtype not in (torch.float32, torch.uint8):
            s = s.to(torch.float32)
        out.append(s)
    if not out:
        raise ValueError("reference sheet: no sources")
    if len({s.dtype for s in out}) != 1:
        raise ValueError("reference sheet: the sources must be all float32 or all uint8")
    return out


def reference_sheet(sources, panels, canvas_size, background=(0, 0, 0), *, out_bytes: bool = False, timings: Optional[dict] = None) -> torch.Tensor:
    """A reference sheet as Pillow builds it: ``sources`` (frames ``[H, W, C]``, all fp32 R,G,B in 0 .. 1 or all uint8, C = 1, 3 or
    more, on the GPU or on the CPU, of any sizes, never written) are quantised (``np.clip(x * 255.0, 0, 255).astype(uint8)``), resized
    with ``Image.resize(..., LANCZOS)`` to fit (``contain_pad``) or fill (``cover_crop``) their panels and pasted in the order of
    ``panels`` (SheetPanel records) onto a canvas of ``canvas_size`` = (width, height) filled with ``background``; a later panel wins
    where two overlap, panels are clipped to the canvas.  Returns a device tensor ``[height, width, 3]``: fp32 byte / 255, or uint8 with
    ``out_bytes``.  A view that is not contiguous is made contiguous (a copy; the view itself is not written).  CPU sources go up one
    by one through the staging pipeline of _devices, each followed by the horizontal pass of its own panels."""
    from . import _devices
    srcs = _sheet_sources(sources)
    byte_sources = srcs[0].dtype == torch.uint8
    plan = SheetPlan([tuple(s.shape) for s in srcs], panels, canvas_size, background)
    if not len(plan.records):
        raise ValueError("reference sheet: no panels")
    dev = _placement([s.device for s in srcs], "reference sheet", "sources", ring=True)
    lib = _hip.lib()
    rows = lib.vrg_sheet_rows_u8 if byte_sources else lib.vrg_sheet_rows_f32
    compose = lib.vrg_sheet_compose_u8 if out_bytes else lib.vrg_sheet_compose_f32
    rec = plan.records.copy()
    source_of = np.array([int(p.source) for p in plan.panels])
    with torch.cuda.device(dev):
        tables = torch.from_numpy(plan.tables).to(dev)
        spans = torch.from_numpy(plan.spans).to(dev)
        tmp = torch.empty(max(plan.tmp_bytes, 1), dtype=torch.uint8, device=dev)
        out = torch.empty((plan.height, plan.width, 3), dtype=torch.uint8 if out_bytes else torch.float32, device=dev)
        marks = [HipEvent() for _ in range(3)] if timings is not None else None

        def run_rows(which):
            part = np.ascontiguousarray(rec[which])
            plan.check(part, byte_sources)
            d = _hip.upload_records(part, dev)
            _hip.check(rows(_hip.ptr(d), len(part), _hip.ptr(tables), plan.table_ints, _hip.ptr(tmp), plan.tmp_bytes, plan.max_segments,
                            plan.max_rows, _hip.current_stream()), "vrg_sheet_rows")

        resident = [i for i, s in enumerate(srcs) if s.is_cuda]
        keep = {i: srcs[i].contiguous() for i in resident}
        for i, s in keep.items():
            rec["src"][source_of == i] = s.data_ptr()
        if marks:
            marks[0].record()
        if resident:
            which = np.nonzero(np.isin(source_of, resident))[0]
            if len(which):
                run_rows(which)
        for i, s in enumerate(srcs):
            which = np.nonzero(source_of == i)[0]
            if s.is_cuda or not len(which):                                        # a source no panel shows is not uploaded
                continue

            def piece(gpu, first, which=which):
                rec["src"][which] = gpu.data_ptr()
                run_rows(which)

            _devices.upload_frames(s.unsqueeze(0), piece)
        if marks:
            marks[1].record()
        plan.check(rec, byte_sources)
        d = _hip.upload_records(rec, dev)
        r, g, b = plan.background
        _hip.check(compose(_hip.ptr(d), len(rec), int(byte_sources), _hip.ptr(tables), plan.table_ints, _hip.ptr(spans), plan.n_spans, _hip.ptr(tmp),
                           plan.tmp_bytes, _hip.ptr(out), plan.width, plan.height, r | (g << 8) | (b << 16), _hip.current_stream()),
                   "vrg_sheet_compose")
        if marks:
            marks[2].record()
            torch.cuda.current_stream().synchronize()
            timings["rows_ms"], timings["compose_ms"] = marks[0].elapsed_ms(marks[1]), marks[1].elapsed_ms(marks[2])
    return out


# ---------------------------------------------------------------------------------------------
# The LTX MSR reference frames (vrgdg_ltx_msr_reference_builder.py of the reference): a few byte stills, each stretched with cv2's byte
# Lanczos-4 and repeated into a run of fp32 / 255 frames, in one launch (csrc/vrg_msr.hip)
# ---------------------------------------------------------------------------------------------
MSR_DESC = _hip.record_dtype(_hip.MsrDesc)
_msr_tables: dict = {}          # (distinct source sizes, out_h, out_w, device) -> the uploaded table


def expand_counts(pictures: int, frame_count: int) -> list:
    """The repeats of the reference's ``_expand_frames``: ``base + (1 if index < remainder else 0)``"""
    base, remainder = divmod(int(frame_count), int(pictures))
    return [base + (1 if index < remainder else 0) for index in range(int(pictures))]


@dataclass
class MsrPlan:
    """The host side of one launch: ``desc`` (MSR_DESC records in picture order, ``src`` still 0; a constant colour comes last), the
    sizes that are filtered with the index of each one's first record in the concatenated table, and the geometry."""
    desc: np.ndarray
    sizes: tuple
    offsets: dict
    n_taps: int
    frames: int
    height: int
    width: int

    def table(self) -> np.ndarray:
        """the concatenated records of vrg_lanczos4_taps, one table per distinct (in_h, in_w), as bytes"""
        parts = [lanczos4_taps(h, w, self.height, self.width).view(np.uint8).reshape(-1) for h, w in self.sizes]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)

    def check(self, desc: Optional[np.ndarray] = None) -> None:
        d = np.ascontiguousarray(self.desc if desc is None else desc)
        _hip.check(_host_lib().vrg_msr_check(C.c_void_p(d.ctypes.data), len(d), self.n_taps, self.frames, self.height, self.width),
                   "vrg_msr_check")


def msr_plan(shapes, size, frame_count: int, fill=None) -> MsrPlan:
    """Descriptors, repeats and frame ranges of ``len(shapes)`` pictures of ``shapes[i] = (height, width)`` -- and, with ``fill`` =
    (R, G, B), a constant colour after them -- spread over ``frame_count`` frames of ``size`` = (width, height).  No GPU needed."""
    width, height = int(size[0]), int(size[1])
    frame_count = int(frame_count)
    if width < 1 or height < 1:
        raise ValueError("msr reference frames: width and height must be at least 1")
    if frame_count < 0 or frame_count > 0x7fffffff:
        raise ValueError("msr reference frames: frame_count must be 0 .. 2^31 - 1")
    shapes = [(int(h), int(w)) for h, w in shapes]
    if any(h < 1 or w < 1 for h, w in shapes):
        raise ValueError("msr reference frames: pictures must be at least 1 x 1")
    n = len(shapes) + (fill is not None)
    if n == 0:
        raise ValueError("msr reference frames: no pictures")
    sizes = tuple(sorted({s for s in shapes if s != (height, width)}))
    offsets, at = {}, 0
    for s in sizes:
        offsets[s] = at
        at += width + height
    if at > 0x7fffffff:
        raise ValueError("msr reference frames: the tap tables pass 2^31 - 1 records")
    desc = np.zeros(n, dtype=MSR_DESC)
    desc["repeats"] = expand_counts(n, frame_count)
    desc["first_frame"] = np.cumsum(desc["repeats"]) - desc["repeats"]
    for i, (h, w) in enumerate(shapes):
        desc["in_h"][i], desc["in_w"][i], desc["taps"][i] = h, w, offsets.get((h, w), -1)
    if fill is not None:
        desc["taps"][n - 1] = -1
        desc["fill"][n - 1, :3] = _sheet_colour(fill, "the background colour")
    return MsrPlan(desc, sizes, offsets, at, frame_count, height, width)


def _msr_table(plan: MsrPlan, device) -> torch.Tensor:
    return _uploaded(_msr_tables, (plan.sizes, plan.height, plan.width, str(device)), plan.table, device)


def msr_reference_frames(pictures, size, frame_count: int, background=None) -> torch.Tensor:
    """``np.stack(_expand_frames([cv2.resize(p, size, INTER_LANCZOS4) for p in pictures + [background]], frame_count)).astype(np.float32)
    / 255.0`` of the reference's MSR builder as one launch: ``pictures`` are ``[h, w, 3]`` uint8 R,G,B tensors or arrays of any sizes, on
    the GPU or on the CPU (uploaded as bytes), ``size`` = (width, height), ``background`` a further picture, an (R, G, B) tuple for a
    constant colour, or None.  A picture that already has the size is taken unfiltered.  Returns the ``[frame_count, height, width, 3]``
    fp32 device tensor; every distinct picture is filtered once, whatever its repeats.  Inputs are never written."""
    what = "msr reference frames"
    pics = [_byte_picture(p, f"{what}: picture {i}", allow_empty=True) for i, p in enumerate(pictures)]      # msr_plan refuses the empty ones
    fill = None
    if isinstance(background, (tuple, list)):
        fill = tuple(background)
    elif background is not None:
        pics.append(_byte_picture(background, f"{what}: picture background", allow_empty=True))
    plan = msr_plan([tuple(p.shape[:2]) for p in pics], size, frame_count, fill)
    dev = _placement([p.device for p in pics], what, "pictures", ring=True)
    desc = plan.desc.copy()
    with torch.cuda.device(dev):
        out = torch.empty((plan.frames, plan.height, plan.width, 3), dtype=torch.float32, device=dev)
        if plan.frames == 0:
            return out
        keep = [p.contiguous().to(dev) if desc["repeats"][i] > 0 else None for i, p in enumerate(pics)]      # a picture no frame shows is not uploaded
        for i, p in enumerate(keep):
            if p is None:
                desc["in_h"][i], desc["in_w"][i], desc["taps"][i] = 1, 1, -1                                   # src stays null: follows nothing
            else:
                desc["src"][i] = p.data_ptr()
        plan.check(desc)
        table = _msr_table(plan, dev)
        d = _hip.upload_records(desc, dev)
        _hip.check(_hip.lib().vrg_msr_frames_f32(_hip.ptr(d), len(desc), _hip.ptr(table), plan.n_taps, _hip.ptr(out), plan.frames, plan.height,
                                                 plan.width, _hip.current_stream()), "vrg_msr_frames_f32")
    return out


def bytes_to_image(picture) -> torch.Tensor:
    """``np.asarray(picture, dtype=np.float32) / 255.0`` as ``[1, h, w, 3]`` fp32 on the device (the reference's _pil_to_image_tensor): the
    launch of msr_reference_frames with one descriptor, no filter, one frame."""
    p = _byte_picture(picture, "msr reference frames: picture 0", allow_empty=True)
    return msr_reference_frames([p], (int(p.shape[1]), int(p.shape[0])), 1)


# ---------------------------------------------------------------------------------------------
# The LTX First / Last temporal guide (VRGDG_LTXFirstLastGuide.py:52-69 of the reference): `last` centre-cropped and bilinearly resampled to
# the size of `first`, the two cross-faded into a batch of frames, in one launch (csrc/vrg_flf.hip)
# ---------------------------------------------------------------------------------------------
FLF_CURVES = ("smoothstep", "linear", "ease_in", "ease_out")
FLF_CHUNK = _hip.FLF_CHUNK


def flf_curve(value, name):
    """The reference's ``_curve``: any name but "linear", "ease_in" and "ease_out" is the smoothstep."""
    if name == "linear":
        return value
    if name == "ease_in":
        return value * value
    if name == "ease_out":
        return 1.0 - (1.0 - value) * (1.0 - value)
    return value * value * (3.0 - 2.0 * value)


def flf_weights(frame_count: int, transition_start=0.05, transition_end=0.90, curve="smoothstep") -> np.ndarray:
    """``[frame_count, 2]`` float32: ``(1.0 - amount, amount)`` of every frame, formed in Python doubles as the reference's loop forms them
    (:61-67) and rounded to fp32 once, which is what torch does with a Python scalar that meets an fp32 tensor."""
    frame_count = int(frame_count)
    if frame_count < 1:
        raise ValueError("first/last guide: frame_count must be at least 1")
    start = max(0.0, min(0.95, float(transition_start)))
    end = max(start + 0.01, min(1.0, float(transition_end)))
    weights = np.empty((frame_count, 2), dtype=np.float64)
    for index in range(frame_count):
        position = index / max(1, frame_count - 1)
        amount = flf_curve(max(0.0, min(1.0, (position - start) / (end - start))), str(curve))
        weights[index] = (1.0 - amount, amount)
    return weights.astype(np.float32)


def center_crop_rect(old_w: int, old_h: int, new_w: int, new_h: int) -> tuple:
    """(x0, y0, width, height) of the view ``comfy.utils.common_upscale(..., crop="center")`` narrows an ``old_w`` x ``old_h`` picture to
    before it resamples it to ``new_w`` x ``new_h``: the wider or taller side loses ``round()`` (Python's, half to even) of half its
    surplus at both ends.  A restatement of the published function; comfy is not vendored."""
    old_w, old_h, new_w, new_h = int(old_w), int(old_h), int(new_w), int(new_h)
    old_aspect, new_aspect = old_w / old_h, new_w / new_h
    x = y = 0
    if old_aspect > new_aspect:
        x = round((old_w - old_w * (new_aspect / old_aspect)) / 2)
    elif old_aspect < new_aspect:
        y = round((old_h - old_h * (old_aspect / new_aspect)) / 2)
    return x, y, old_w - 2 * x, old_h - 2 * y


def _flf_picture(t, name):
    if not isinstance(t, torch.Tensor) or t.ndim != 4:
        raise ValueError(f"first/last guide: {name} must be a [batch, height, width, channels] IMAGE tensor")
    if int(t.shape[0]) < 1:
        raise ValueError(f"first/last guide: {name} is an empty batch")
    if t.dtype != torch.float32:
        raise ValueError(f"first/last guide: {name} must be fp32")
    return t.detach()[:1]


def flf_plan(first_shape, last_shape, frame_count: int, transition_start=0.05, transition_end=0.90, curve="smoothstep"):
    """The host side of one launch, no GPU needed: ``(rectangle, weights)`` for pictures of ``first_shape`` / ``last_shape`` =
    (height, width, channels), checked by vrg_flf_check."""
    (h, w, c), (last_h, last_w, last_c) = (tuple(int(v) for v in s) for s in (first_shape, last_shape))
    if c != last_c:
        raise ValueError(f"first/last guide: first has {c} channels, last has {last_c}")
    if c not in (3, 4):
        raise ValueError(f"first/last guide: {c} channels (3 or 4 are taken)")
    if min(h, w, last_h, last_w) < 1:
        raise ValueError("first/last guide: pictures must be at least 1 x 1")
    weights = flf_weights(frame_count, transition_start, transition_end, curve)
    rect = (0, 0, last_w, last_h) if (last_h, last_w) == (h, w) else center_crop_rect(last_w, last_h, w, h)
    _refuse(_host_lib().vrg_flf_check(len(weights), h, w, c, last_h, last_w, *rect), "first/last guide",
            f"vrg_flf_check refuses {last_w} x {last_h} -> {w} x {h}, rectangle {rect}",
            f"{len(weights)} frames of {w} x {h} x {c} are more than one launch takes")
    return rect, weights


def flf_guide_frames(first, last, frame_count: int, transition_start=0.05, transition_end=0.90, curve="smoothstep", out=None) -> torch.Tensor:
    """``torch.cat([first * (1.0 - amount) + last' * amount for every frame])`` of the reference's First / Last guide as one launch:
    ``first[:1]`` and ``last[:1]`` are fp32 IMAGE tensors on the GPU (used in place) or on the CPU (the two pictures are uploaded),
    ``last'`` is ``last`` centre-cropped and bilinearly resampled to the size of ``first`` (not clamped) unless it already has it.
    Returns the ``[frame_count, H, W, C]`` fp32 device tensor, ``out`` where one is given.  Inputs are never written."""
    from . import _devices
    a, b = _flf_picture(first, "first"), _flf_picture(last, "last")
    rect, weights = flf_plan(tuple(a.shape[1:]), tuple(b.shape[1:]), frame_count, transition_start, transition_end, curve)
    dev = _placement([a.device, b.device], "first/last guide", "pictures", ring=True)
    frames, (h, w, c) = len(weights), (int(v) for v in a.shape[1:])
    out = _checked_out(out, (frames, h, w, c), torch.float32, dev, "first/last guide")
    with torch.cuda.device(dev):
        a, b = (t.contiguous() if t.is_cuda else _devices.on_device(t, dev).contiguous() for t in (a, b))
        _disjoint("first/last guide", [("out", out)], [("first", a), ("last", b)])
        wd = torch.from_numpy(weights).to(dev)
        _hip.check(_hip.lib().vrg_flf_guide_f32(_hip.ptr(a), _hip.ptr(b), _hip.ptr(wd), _hip.ptr(out), frames, h, w, c, int(b.shape[1]),
                                                int(b.shape[2]), *rect, _hip.current_stream()), "vrg_flf_guide_f32")
    return out


# ---------------------------------------------------------------------------------------------
# Multi-reference image batches (VRGDG_MultiReferenceConditioning, ...FromPaths and VRGDG_ImageBatchMultiFromPaths,
# VRGDG_GeneralNodes2.py:3801-4145 of the reference): up to 50 pictures of unrelated sizes and channel counts, each brought to a megapixel
# budget, or all to the first one's shape, by comfy.utils.common_upscale's rule -- one launch of csrc/vrg_refbatch.hip for all of them
# ---------------------------------------------------------------------------------------------
REFBATCH_METHODS = ("nearest-exact", "bilinear", "area", "bicubic", "lanczos")          # the reference's upscale_methods, in its order
_REFBATCH_FILTERS = {"bicubic": _hip.REFBATCH_BICUBIC, "bilinear": _hip.REFBATCH_BILINEAR, "area": _hip.REFBATCH_AREA,
                     "nearest-exact": _hip.REFBATCH_NEAREST_EXACT}
REFBATCH_DESC = _hip.record_dtype(_hip.RefbatchDesc)


def total_pixels_size(height: int, width: int, megapixels, resolution_steps=1) -> tuple:
    """(height, width) a picture of ``height`` x ``width`` is scaled to for a budget of ``megapixels`` * 1024 * 1024 pixels, each side
    rounded (Python's ``round``, half to even) to a multiple of ``resolution_steps`` and at least 1: the size rule of the reference's
    ``_scale_to_total_pixels`` (:3861-3865)."""
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError("total_pixels_size: the picture must be at least 1 x 1")
    total = float(megapixels) * 1024 * 1024
    scale_by = math.sqrt(total / (width * height))
    steps = max(1, int(resolution_steps))
    new_w = max(1, round(width * scale_by / steps) * steps)
    new_h = max(1, round(height * scale_by / steps) * steps)
    return int(new_h), int(new_w)


@dataclass
class _RefJob:
    """one record of a launch: `frames` pictures [h][w][c] at element `src_offset` of `src`, their rectangle resampled to `dst`"""
    src: torch.Tensor
    src_offset: int
    src_shape: tuple             # (h, w, c)
    rect: tuple                  # (x0, y0, w, h)
    dst_offset: int
    dst_shape: tuple             # (h, w, c)
    method: int
    frames: int


def _refbatch_method(name, what):
    if name not in REFBATCH_METHODS:
        raise ValueError(f"{what}: unknown upscale_method {name!r} (one of {', '.join(REFBATCH_METHODS)})")
    return str(name)


def refbatch_table(jobs, out_elems: int):
    """The host side of one launch, no GPU needed: ``(records, tiles, (f32 base, floats), (u8 base, bytes))``.  The sources of a call
    are addressed from the lowest address among them, so device-resident pictures are read where they lie; the records are checked by
    vrg_refbatch_check."""
    spans = {}
    for dtype in (torch.float32, torch.uint8):
        ts = [j.src for j in jobs if j.src.dtype == dtype]
        lo = min((t.data_ptr() for t in ts), default=0)
        hi = max((t.data_ptr() + t.numel() * t.element_size() for t in ts), default=0)
        spans[dtype] = (lo, (hi - lo) // (4 if dtype == torch.float32 else 1))
    desc = np.zeros(len(jobs), dtype=REFBATCH_DESC)
    tiles = 0
    for i, j in enumerate(jobs):
        lo = spans[j.src.dtype][0]
        offset = (j.src.data_ptr() - lo) // j.src.element_size() + int(j.src_offset)
        if tiles > 0x7fffffff:
            raise RuntimeError("reference batch: more tiles than one launch takes")
        desc[i] = (offset, int(j.dst_offset), *j.src_shape, *j.rect, *j.dst_shape, int(j.method), int(j.frames), tiles, 0)
        tiles += int(j.frames) * -(-int(np.prod(j.dst_shape, dtype=np.int64)) // _hip.REFBATCH_TILE)
    _refuse(_host_lib().vrg_refbatch_check(C.c_void_p(desc.ctypes.data), len(jobs), spans[torch.float32][1], spans[torch.uint8][1], int(out_elems)),
            "reference batch", "vrg_refbatch_check refuses the records (sizes, channel counts, rectangles or overlapping outputs)",
            "a picture is larger than one launch takes (2^31 - 1 elements a picture, 65536 source pixels under one area pixel)")
    return desc, tiles, spans[torch.float32], spans[torch.uint8]


def _refbatch_launch(dev, jobs, out: torch.Tensor):
    """every record of `jobs` into the flat fp32 (or, for quantise records, uint8) buffer `out`: one launch on the current stream"""
    if not jobs:
        return
    desc, tiles, (f_base, f_floats), (b_base, b_bytes) = refbatch_table(jobs, out.numel())
    table = _hip.upload_records(desc, dev)
    if out.dtype == torch.uint8:
        _hip.check(_hip.lib().vrg_refbatch_quantise_u8(C.c_void_p(f_base), f_floats, _hip.ptr(table), len(jobs), tiles, _hip.ptr(out), out.numel(),
                                                       _hip.current_stream()), "vrg_refbatch_quantise_u8")
    else:
        _hip.check(_hip.lib().vrg_refbatch_f32(C.c_void_p(f_base), f_floats, C.c_void_p(b_base), b_bytes, _hip.ptr(table), len(jobs), tiles,
                                               _hip.ptr(out), out.numel(), _hip.current_stream()), "vrg_refbatch_f32")


def _refbatch_pictures(images, what):
    """the checked pictures of a call on one device: ``(device, [contiguous fp32 [B, H, W, C] tensors])``"""
    if isinstance(images, torch.Tensor):
        raise ValueError(f"{what}: images must be a list of IMAGE tensors")
    images = list(images)
    for i, t in enumerate(images):
        if not isinstance(t, torch.Tensor) or t.ndim != 4:
            raise ValueError(f"{what}: image {i} must be a [batch, height, width, channels] IMAGE tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: image {i} must be fp32")
        if min(int(v) for v in t.shape[:3]) < 1:
            raise ValueError(f"{what}: image {i} is empty")
        if int(t.shape[3]) not in (3, 4):
            raise ValueError(f"{what}: image {i} has {int(t.shape[3])} channels (3 or 4 are taken)")
    return _refbatch_place(images, what)


def _refbatch_place(images, what):
    """device tensors as they are, all CPU pictures in ONE upload"""
    dev = _placement([t.device for t in images], what, "pictures", ring=False)
    pics = [t.detach() for t in images]
    host = [i for i, t in enumerate(pics) if not t.is_cuda]
    with torch.cuda.device(dev):
        if host:
            packed = torch.cat([pics[i].contiguous().reshape(-1) for i in host]).to(dev)
            at = 0
            for i in host:
                shape, n = pics[i].shape, pics[i].numel()
                pics[i] = packed[at:at + n].view(shape)
                at += n
        pics = [t.contiguous() for t in pics]
    return dev, pics


def _refbatch_out(out, total: int, dev, what):
    if out is None:
        return torch.empty(max(total, 1), dtype=torch.float32, device=dev)
    if (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.float32 or out.ndim != 1 or not out.is_contiguous()
            or out.numel() < total):
        raise ValueError(f"{what}: out must be a contiguous flat fp32 tensor of at least {total} elements on {dev}")
    return out


def _refbatch_lanczos_jobs(dev, items):
    """comfy's ``lanczos`` for ``items`` = [(fp32 [B, h, w, 3] device picture, rectangle, (out_w, out_h))]: the rectangles quantised to
    bytes in one launch, ``Image.resize(..., LANCZOS)`` of every frame by vrg_pil_resize_u8 (one call, all sizes), and the
    VRG_REFBATCH_BYTES jobs (dst_offset left at 0) that turn the result into fp32"""
    from . import far_face_repair
    quantise, offsets, sizes, at = [], [], [], 0
    for t, (x0, y0, rw, rh), (ow, oh) in items:
        frames, h, w, c = (int(v) for v in t.shape)
        quantise.append(_RefJob(t, 0, (h, w, c), (x0, y0, rw, rh), at, (rh, rw, c), _hip.REFBATCH_COPY, frames))
        for f in range(frames):
            offsets.append(at + f * rh * rw * c)
            sizes.append((rw, rh, ow, oh))
        at += frames * rh * rw * c
    qbuf = torch.empty(max(at, 1), dtype=torch.uint8, device=dev)
    _refbatch_launch(dev, quantise, qbuf)
    plan = far_face_repair.ResizePlan(qbuf, offsets, sizes, 3, dev)
    resized = plan.run()
    jobs, k = [], 0
    for t, _, (ow, oh) in items:
        frames = int(t.shape[0])
        jobs.append(_RefJob(resized, plan.offsets[k], (oh, ow, 3), (0, 0, ow, oh), 0, (oh, ow, 3), _hip.REFBATCH_BYTES, frames))
        k += frames
    return jobs


def _lanczos_rgb_only(channels, what):
    if any(c != 3 for c in channels):
        raise NotImplementedError(f"{what}: lanczos takes 3-channel pictures only (Pillow's byte Lanczos is restated for RGB); "
                                  f"got {sorted(set(channels))} channels")


def scale_reference_images(images, upscale_method="nearest-exact", megapixels=1.0, resolution_steps=1, out=None) -> list:
    """``_scale_to_total_pixels`` of the reference for a list of fp32 ``[B, H, W, C]`` pictures (C = 3 or 4; on the GPU, used where they
    lie, or on the CPU, uploaded together): each is resampled to ``total_pixels_size`` of its own size by
    ``comfy.utils.common_upscale(..., upscale_method, "disabled")`` -- all channels, not clamped, the filter evaluated even at an equal size
    -- and all of them by ONE launch.  "lanczos" goes through bytes and Pillow's filter as comfy does and takes 3 channels only.
    Returns the device tensors, views of one buffer: ``out`` (flat fp32), which they fill back to back from its start, or a new one in
    which every picture starts on the 16-byte grid.  Inputs are never written."""
    what = "scale_reference_images"
    method = _refbatch_method(upscale_method, what)
    dev, pics = _refbatch_pictures(images, what)
    if method == "lanczos":
        _lanczos_rgb_only([int(t.shape[3]) for t in pics], what)
    sizes = [total_pixels_size(int(t.shape[1]), int(t.shape[2]), megapixels, resolution_steps) for t in pics]
    offsets, total = [], 0
    for t, (oh, ow) in zip(pics, sizes):
        if out is None:
            total = (total + 3) & ~3
        offsets.append(total)
        total += int(t.shape[0]) * oh * ow * int(t.shape[3])
    with torch.cuda.device(dev):
        buf = _refbatch_out(out, total, dev, what)
        _disjoint(what, [("out", buf)], [(f"image {i}", t) for i, t in enumerate(pics)])
        if method == "lanczos":
            jobs = _refbatch_lanczos_jobs(dev, [(t, (0, 0, int(t.shape[2]), int(t.shape[1])), (ow, oh)) for t, (oh, ow) in zip(pics, sizes)])
            for j, at in zip(jobs, offsets):
                j.dst_offset = at
        else:
            jobs = [_RefJob(t, 0, tuple(int(v) for v in t.shape[1:]), (0, 0, int(t.shape[2]), int(t.shape[1])), at, (oh, ow, int(t.shape[3])),
                            _REFBATCH_FILTERS[method], int(t.shape[0])) for t, (oh, ow), at in zip(pics, sizes, offsets)]
        _refbatch_launch(dev, jobs, buf)
    return [buf[at:at + int(t.shape[0]) * oh * ow * int(t.shape[3])].view(int(t.shape[0]), oh, ow, int(t.shape[3]))
            for t, (oh, ow), at in zip(pics, sizes, offsets)]


def batch_channels(channels) -> int:
    """The channel count of the reference's batch for pictures of ``channels`` (in order): the base is re-padded with 1.0 whenever a wider
    picture arrives and narrower ones are padded to it.  A picture that was appended before the base grew keeps its count in the
    reference, whose ``torch.cat`` then fails; that order is refused here as well."""
    channels = [int(c) for c in channels]
    base, appended = channels[0], []
    for c in channels[1:]:
        base = max(base, c)
        appended.append(base)
    if any(c != base for c in appended):
        raise ValueError(f"reference batch: pictures of {channels} channels cannot be joined in this order (the reference's torch.cat fails: a "
                         f"{base}-channel picture follows narrower ones that were already appended)")
    return base


def batch_reference_images(images, upscale_method="bilinear", out=None) -> torch.Tensor:
    """``_batch_for_image_output`` / ``load_batch`` of the reference: every picture brought to the first one's height, width and (padded)
    channel count and joined along the batch axis.  Missing channels are 1.0, padded BEFORE the resize; a picture of another size is
    centre-cropped (``center_crop_rect``) and resampled by ``upscale_method``; one that already fits, the base included, is copied bit for
    bit.  ONE launch writes the whole ``torch.cat`` result (``out``: an optional contiguous fp32 tensor of its shape).  A single picture
    is returned as it is.  Inputs are never written."""
    what = "batch_reference_images"
    method = _refbatch_method(upscale_method, what)
    if not isinstance(images, torch.Tensor) and len(images) == 1 and isinstance(images[0], torch.Tensor):
        return images[0]
    dev, pics = _refbatch_pictures(images, what)
    if not pics:
        raise ValueError(f"{what}: no pictures")
    height, width = int(pics[0].shape[1]), int(pics[0].shape[2])
    channels = batch_channels([int(t.shape[3]) for t in pics])
    fits = [(int(t.shape[1]), int(t.shape[2])) == (height, width) for t in pics]
    if method == "lanczos" and not all(fits):
        _lanczos_rgb_only([channels], what)
    frame = height * width * channels
    offsets = np.concatenate([[0], np.cumsum([int(t.shape[0]) * frame for t in pics])])
    shape = (int(sum(int(t.shape[0]) for t in pics)), height, width, channels)
    with torch.cuda.device(dev):
        buf = _refbatch_out(None, int(offsets[-1]), dev, what) if out is None else _checked_out(out, shape, torch.float32, dev, what).view(-1)
        _disjoint(what, [("out", buf)], [(f"image {i}", t) for i, t in enumerate(pics)])
        jobs, lanczos = [], []
        for t, fit, at in zip(pics, fits, offsets[:-1]):
            frames, h, w, c = (int(v) for v in t.shape)
            rect = (0, 0, w, h) if fit else center_crop_rect(w, h, width, height)
            if fit:
                jobs.append(_RefJob(t, 0, (h, w, c), rect, int(at), (height, width, channels), _hip.REFBATCH_COPY, frames))
            elif method == "lanczos":
                lanczos.append((t, rect, (width, height), int(at)))
            else:
                jobs.append(_RefJob(t, 0, (h, w, c), rect, int(at), (height, width, channels), _REFBATCH_FILTERS[method], frames))
        if lanczos:
            for j, item in zip(_refbatch_lanczos_jobs(dev, [i[:3] for i in lanczos]), lanczos):
                j.dst_offset = item[3]
                jobs.append(j)
        _refbatch_launch(dev, jobs, buf)
    return buf[:int(offsets[-1])].view(shape)


def reference_bytes_to_images(pictures) -> list:
    """``torch.from_numpy(np.asarray(picture).astype(np.float32) / 255.0).unsqueeze(0)`` (the reference's ``_load_image_tensor`` after its
    decode) for a list of uint8 ``[H, W, 3]`` pictures, arrays or tensors: one upload of the bytes, one launch (VRG_REFBATCH_BYTES), a list
    of ``[1, H, W, 3]`` fp32 device tensors, each on the 16-byte grid."""
    what = "reference_bytes_to_images"
    items = [p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p)) for p in pictures]
    for i, t in enumerate(items):
        if t.dtype != torch.uint8 or t.ndim != 3 or int(t.shape[2]) != 3 or min(int(v) for v in t.shape[:2]) < 1:
            raise ValueError(f"{what}: picture {i} must be uint8 [height, width, 3]")
    if not items:
        return []
    dev, srcs = _refbatch_place(items, what)
    offsets, total = [], 0
    for t in items:
        total = (total + 3) & ~3
        offsets.append(total)
        total += t.numel()
    with torch.cuda.device(dev):
        buf = torch.empty(total, dtype=torch.float32, device=dev)
        jobs = [_RefJob(s, 0, tuple(int(v) for v in t.shape), (0, 0, int(t.shape[1]), int(t.shape[0])), at, tuple(int(v) for v in t.shape),
                        _hip.REFBATCH_BYTES, 1) for s, t, at in zip(srcs, items, offsets)]
        _refbatch_launch(dev, jobs, buf)
    return [buf[at:at + t.numel()].view(1, *t.shape) for t, at in zip(items, offsets)]


# ---------------------------------------------------------------------------------------------
# Music-video assembly (VRGDG_CombinevideosV2 / V3, HumoAutomation.py:50-133 and :892-1030; VRGDG_CombinevideosV5,
# HumoAutomationExtra2.py:309-498; VRGDG_PadVideoWithLastFrame, GeneralVideoNodes.py:1945-1987; VRGDG_LoadVideos, nodes.py:1327-1377 of the
# reference): which frame of which clip becomes which output frame is planned on the host, the frames are moved by ONE launch of
# csrc/vrg_assemble.hip -- and V5's labelled MP4 bytes come out of the same read
# ---------------------------------------------------------------------------------------------
ASSEMBLE_SLOTS = _hip.ASSEMBLE_MAX_SOURCES       # video_1 .. video_16
ASSEMBLE_BAR = _hip.ASSEMBLE_BAR                 # rows of V5's label bar
ASSEMBLE_MODES = ("v2", "v3", "v5", "pad", "load")
ASSEMBLE_ENTRY = _hip.record_dtype(_hip.AssembleEntry)


def _assemble_shape(entry):
    return None if entry is None else ((int(entry), 0, 0, 0) if isinstance(entry, (int, np.integer)) else tuple(int(v) for v in entry))


def assemble_plan(mode, shapes, fps=25.0, audio_meta=None, index=0, total_sets=1, groups_in_last_set=16, pad_frames=1, pad_front=False) -> list:
    """The host side of the assembly nodes, no GPU needed: the ``(source, frame)`` pair of every output frame, in order.  ``shapes`` holds
    one entry per input slot (``video_1`` first) -- a shape tuple, a frame count, or None for a slot that is not connected -- and
    ``source`` is the slot's index in it.  The reference's integer arithmetic, expression for expression:

    ``"v2"``: durations padded with 0.0 or cut to 16; a clip's target is ``max(1, int(round(dur * float(fps))))`` for ``dur > 0`` (a value
    ``float()`` refuses counts as 0) and its own length otherwise; longer clips are trimmed, shorter ones repeat their last frame.
    ``"v3"`` / ``"v5"``: ``durations_frames`` before ``durations``; ``max(1, int(round(value)))`` or ``max(1, int(round(fps * value)))``
    (Python's ``round``: half to even, on the double); missing durations are 0.0, a target of 1; on the last run
    (``index == total_sets - 1``) only slots up to ``max(1, min(groups_in_last_set, 16))`` are looked at and a slot above
    ``groups_in_last_set`` is skipped; clips are trimmed, never padded.  The plan may be empty (the reference's ``torch.cat`` then fails).
    ``"pad"``: one clip; ``pad_frames`` copies of frame 0 in front (``pad_front``) or of the last frame behind it; ``pad_frames <= 0`` or an
    empty clip: the clip as it is.  ``"load"``: the clips one after another.
    The reference's errors and their texts are kept: no videos, ``ndim != 4``, ``audio_meta`` that is no dict, no durations."""
    if mode not in ASSEMBLE_MODES:
        raise ValueError(f"assemble_plan: unknown mode {mode!r} (one of {', '.join(ASSEMBLE_MODES)})")
    shapes = [_assemble_shape(s) for s in shapes]
    if mode == "load":
        return [(i, f) for i, s in enumerate(shapes) if s is not None for f in range(s[0])]
    if mode == "pad":
        frames = shapes[0][0]
        body = [(0, f) for f in range(frames)]
        if frames == 0 or pad_frames <= 0:
            return body
        pad = [(0, 0 if pad_front else frames - 1)] * int(pad_frames)
        return pad + body if pad_front else body + pad
    if len(shapes) > ASSEMBLE_SLOTS:
        raise ValueError(f"assemble_plan: {len(shapes)} slots ({ASSEMBLE_SLOTS} at the most)")
    if mode == "v2":
        if isinstance(audio_meta, dict) and isinstance(audio_meta.get("durations"), (list, tuple)):
            durations = (list(audio_meta["durations"]) + [0.0] * ASSEMBLE_SLOTS)[:ASSEMBLE_SLOTS]
        else:
            durations = [0.0] * ASSEMBLE_SLOTS
        vids = [(i + 1, s) for i, s in enumerate(shapes) if s is not None]
        if len(vids) < 1:
            raise ValueError("Provide at least one videos (e.g., video_1).")
        plan = []
        for slot, shape in vids:
            if len(shape) != 4:
                raise ValueError(f"video_{slot} must have shape (frames,H,W,C), got {shape}")
            cur = shape[0]
            try:
                dur = float(durations[slot - 1])
            except Exception:
                dur = 0.0
            tgt = max(1, int(round(dur * float(fps)))) if dur > 0.0 else int(cur)
            plan += [(slot - 1, f) for f in range(min(cur, tgt))]
            if 0 < cur < tgt:
                plan += [(slot - 1, cur - 1)] * (tgt - cur)
        return plan
    tag = "[CombineV3]" if mode == "v3" else "[CombineV5]"
    last_run = index == total_sets - 1
    if not isinstance(audio_meta, dict):
        raise ValueError(f"{tag} audio_meta must be a dict")
    if audio_meta.get("durations_frames") is not None:
        durations, is_frames = list(audio_meta["durations_frames"]), True
    elif audio_meta.get("durations") is not None:
        durations, is_frames = list(audio_meta["durations"]), False
    else:
        raise ValueError("[CombineV3] audio_meta missing 'durations' or 'durations_frames' list" if mode == "v3"
                         else "[CombineV5] audio_meta missing durations info")
    durations = (durations + [0.0] * ASSEMBLE_SLOTS)[:ASSEMBLE_SLOTS]
    limit = max(1, min(groups_in_last_set, ASSEMBLE_SLOTS)) if last_run else ASSEMBLE_SLOTS
    vids = [(i + 1, s) for i, s in enumerate(shapes[:limit]) if s is not None]
    if not vids:
        raise ValueError("[CombineV3] No video inputs detected. Connect at least one video_x input." if mode == "v3"
                         else "[CombineV5] No video inputs detected.")
    plan = []
    for slot, shape in vids:
        if mode == "v3" and len(shape) != 4:
            raise ValueError(f"video_{slot} must have shape (frames,H,W,C), got {shape}")
        value = float(durations[slot - 1])
        tgt = max(1, int(round(value))) if is_frames else max(1, int(round(fps * value)))
        if last_run and slot > groups_in_last_set:
            continue
        if len(shape) != 4:
            raise ValueError(f"Expected (frames,H,W,C), got {shape}")
        plan += [(slot - 1, f) for f in range(min(shape[0], tgt))]
    return plan


@dataclass
class _Assembly:
    """one launch, ready: the descriptor, the device table and what keeps their memory alive"""
    device: torch.device
    desc: "_hip.AssembleDesc"
    table: torch.Tensor
    frames: int
    shape: tuple                 # (height, width, channels)
    host_fed: bool               # every clip came from the CPU: the results go to the intermediate device
    rows: np.ndarray             # the table on the host
    keep: list
    reads: list                  # (name, tensor) of what the kernel reads: the clips and overlays as they lie on the device


def _assemble_prepare(videos, plan, overlays, what) -> _Assembly:
    if isinstance(videos, torch.Tensor):
        videos = [videos]
    videos = list(videos)
    entries = np.asarray(plan, dtype=np.int64).reshape(-1, 2)
    used = sorted(set(int(s) for s in entries[:, 0]))
    if not len(entries):
        raise ValueError(f"{what}: the plan is empty")
    if len(used) > ASSEMBLE_SLOTS:
        raise ValueError(f"{what}: the plan names {len(used)} clips ({ASSEMBLE_SLOTS} at the most)")
    for s in used:
        if s < 0 or s >= len(videos) or not isinstance(videos[s], torch.Tensor) or videos[s].ndim != 4:
            raise ValueError(f"{what}: the plan names clip {s}, which is no [frames, height, width, channels] tensor")
    clips = {s: videos[s].detach() for s in used}
    kinds = {t.dtype == torch.uint8 for t in clips.values()}
    if len(kinds) > 1:
        raise ValueError(f"{what}: uint8 and float clips cannot be joined")
    is_bytes = kinds.pop()
    if not is_bytes and any(not t.dtype.is_floating_point for t in clips.values()):
        raise ValueError(f"{what}: clips must be float (IMAGE) or uint8 R,G,B tensors")
    shape = tuple(int(v) for v in clips[used[0]].shape[1:])
    for s, t in clips.items():
        if tuple(int(v) for v in t.shape[1:]) != shape:
            raise ValueError(f"{what}: clip {s} is {tuple(t.shape[1:])}, clip {used[0]} is {shape}: height, width and channels must agree")
        lo, hi = int(entries[entries[:, 0] == s, 1].min()), int(entries[entries[:, 0] == s, 1].max())
        if lo < 0 or hi >= int(t.shape[0]):
            raise ValueError(f"{what}: the plan names frames {lo} .. {hi} of clip {s}, which has {int(t.shape[0])}")
    dev = _placement([t.device for t in clips.values()], what, "clips", ring=False)
    host_fed = not any(t.is_cuda for t in clips.values())
    desc, keep, reads, rows = _hip.AssembleDesc(), [], [], np.zeros(len(entries), dtype=ASSEMBLE_ENTRY)
    desc.n_src, desc.bytes = len(used), int(is_bytes)
    with torch.cuda.device(dev):
        for k, s in enumerate(used):
            t, mine = clips[s], entries[:, 0] == s
            first = 0
            if not t.is_cuda:                                      # only the frames the plan keeps cross PCIe
                first, last = int(entries[mine, 1].min()), int(entries[mine, 1].max())
                t = t[first:last + 1].to(dev)
            if not is_bytes and t.dtype != torch.float32:
                t = t.to(torch.float32)
            t = t.contiguous()
            keep.append(t)
            reads.append((f"clip {s}", t))
            rows["source"][mine], rows["frame"][mine] = k, entries[mine, 1] - first
            desc.src[k], desc.frames[k] = t.data_ptr(), int(t.shape[0])
            desc.height[k], desc.width[k], desc.channels[k] = shape
            if overlays is not None and s < len(overlays) and overlays[s] is not None:
                o = overlays[s] if isinstance(overlays[s], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(overlays[s]))
                if o.dtype != torch.uint8 or tuple(o.shape) != (ASSEMBLE_BAR, shape[1], 3):
                    raise ValueError(f"{what}: overlay {s} must be uint8 [{ASSEMBLE_BAR}, {shape[1]}, 3] (B,G,R)")
                o = o.detach().to(dev).contiguous()
                keep.append(o)
                reads.append((f"overlay {s}", o))
                desc.overlay[k] = o.data_ptr()
        table = _hip.upload_records(rows, dev)
    return _Assembly(dev, desc, table, len(entries), shape, host_fed, rows, keep, reads)


def _assemble_check(a: _Assembly, out_f32, out_u8, labelled, what):
    _refuse(_host_lib().vrg_assemble_check(C.byref(a.desc), C.c_void_p(a.rows.ctypes.data), a.frames, None if out_f32 is None else _hip.ptr(out_f32),
                                           None if out_u8 is None else _hip.ptr(out_u8), int(labelled)),
            what, "vrg_assemble_check refuses the call (clip shapes, channels, or an output that overlaps a clip)",
            f"a frame of {a.shape} is larger than one launch takes (2^31 - 1 elements)")


def assemble_frames(videos, plan, out=None) -> torch.Tensor:
    """``torch.cat`` of the trimmed and padded clips of the reference's assembly nodes as ONE launch: output frame ``i`` is frame
    ``plan[i][1]`` of ``videos[plan[i][0]]`` (``ops.assemble_plan``).  ``videos``: up to 16 named clips ``[F, H, W, C]`` of one frame
    shape; float clips are copied bit for bit (fp32; other float types are widened by torch first), uint8 R,G,B clips become
    ``byte / 255`` in fp32.  Clips on the GPU are read where they lie and the batch stays there; of CPU clips only the frames the plan keeps
    are uploaded, and when every clip came from the CPU the batch is returned on the intermediate device.  ``out``: an optional
    contiguous fp32 ``[N, H, W, C]`` device tensor that overlaps no clip.  Inputs are never written."""
    from . import _devices
    what = "assemble_frames"
    a = _assemble_prepare(videos, plan, None, what)
    with torch.cuda.device(a.device):
        dst = _checked_out(out, (a.frames, *a.shape), torch.float32, a.device, what)
        _disjoint(what, [("out", dst)], a.reads)
        _assemble_check(a, dst, None, False, what)
        _hip.check(_hip.lib().vrg_assemble_f32(C.byref(a.desc), _hip.ptr(a.table), a.frames, _hip.ptr(dst), _hip.current_stream()),
                   "vrg_assemble_f32")
    return dst.to(_devices.intermediate_device()) if a.host_fed and out is None else dst


def assemble_labelled_bytes(videos, plan, overlays=None, clean_out=None):
    """What ``VRGDG_CombinevideosV5`` hands its MP4 writer, ``[N, H + 60, W, 3]`` uint8 in B,G,R, for the frames of ``plan``: per value
    ``q1 = trunc(x * 255)``, ``q2 = trunc((q1 / 255) * 255)`` in fp32 with both roundings kept, under every frame a 60-row bar that is black
    or holds ``overlays[source]`` (uint8 ``[60, W, 3]`` B,G,R: the label pixels, made on the host).  Equal to the reference for finite
    ``0 <= x * 255 < 256``; outside that range bytes saturate to 0 / 255 and NaN gives 0.  ``clean_out``: True, or a contiguous fp32
    ``[N, H, W, 3]`` device tensor, to get ``assemble_frames``' batch from the same read of the clips.  Returns ``(bytes, clean or None)``;
    device and upload rules as for ``assemble_frames``."""
    from . import _devices
    what = "assemble_labelled_bytes"
    a = _assemble_prepare(videos, plan, overlays, what)
    if a.shape[2] != 3:
        raise ValueError(f"{what}: labelled output takes 3-channel clips, got {a.shape[2]}")
    with torch.cuda.device(a.device):
        given = isinstance(clean_out, torch.Tensor)
        clean = _checked_out(clean_out if given else None, (a.frames, *a.shape), torch.float32, a.device, what, "clean_out") if given or clean_out else None
        data = torch.empty((a.frames, a.shape[0] + ASSEMBLE_BAR, a.shape[1], 3), dtype=torch.uint8, device=a.device)
        _disjoint(what, [("clean_out", clean)], a.reads)
        _assemble_check(a, clean, data, True, what)
        _hip.check(_hip.lib().vrg_assemble_labelled_u8(C.byref(a.desc), _hip.ptr(a.table), a.frames, None if clean is None else _hip.ptr(clean),
                                                       _hip.ptr(data), _hip.current_stream()), "vrg_assemble_labelled_u8")
    if a.host_fed:
        to = _devices.intermediate_device()
        return data.to(to), (clean if clean is None or given else clean.to(to))
    return data, clean


# ---------------------------------------------------------------------------------------------
# The anchor round trip of the Video Enhance and Face Fix pipelines (VRGDG_VideoEnhanceNodes.py:143-167, :295-319 and
# VRGDG_StandaloneFaceFixNodes.py:27-51, :658-702 of the reference): decoded anchor stills to the fp32 batch of the image model in one
# launch, the model's fp32 output to the bytes of the PNG files in one launch (csrc/vrg_anchor.hip)
# ---------------------------------------------------------------------------------------------
ANCHOR_DESC = _hip.record_dtype(_hip.AnchorDesc)
_NO_ANCHOR_PICTURES = "anchor_frames: at least one picture is needed"
_NO_ANCHOR_IMAGES = "anchor_store_bytes: at least one image is needed"


def anchor_plan(shapes, size=None):
    """``(records, tables, src_bytes, (height, width))`` for pictures of ``shapes`` = [(height, width), ...] packed back to back: the
    ANCHOR_DESC records, the int32 axis tables of ``Image.resize(.., LANCZOS)`` they index (one per distinct (n_in, n_out); none for an
    axis that keeps its size) and the bytes of the packed pictures.  The size is ``size`` = (width, height), by default the first picture's.
    Host only."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    if not shapes:
        raise ValueError(_NO_ANCHOR_PICTURES)
    height, width = shapes[0] if size is None else (int(size[1]), int(size[0]))
    if height < 1 or width < 1:
        raise ValueError("anchor_frames: size must be at least 1 x 1")
    desc = np.zeros(len(shapes), dtype=ANCHOR_DESC)
    tables, table_at, n_ints, at = [], {}, 0, 0
    for i, (h, w) in enumerate(shapes):
        where, ks = [0, 0], [0, 0]
        for axis, (n_in, n_out) in enumerate(((w, width), (h, height))):
            if n_in == n_out:
                continue
            if (n_in, n_out) not in table_at:
                ksize, table = pil_axis_table(_hip.PIL_FILTER_LANCZOS, n_in, n_out)
                table_at[(n_in, n_out)] = (n_ints, ksize)
                tables.append(table)
                n_ints += len(table)
            where[axis], ks[axis] = table_at[(n_in, n_out)]
        desc[i] = (at, where[0], where[1], w, h, ks[0], ks[1])
        at += h * w * 3
    return desc, (np.concatenate(tables) if tables else np.zeros(0, np.int32)), at, (height, width)


def anchor_check(desc, tables, src_bytes: int, height: int, width: int) -> None:
    """the host refusal of records the kernel would not follow (vrg_anchor_check): ValueError, before any launch"""
    desc = np.ascontiguousarray(desc)
    tables = np.ascontiguousarray(tables, dtype=np.int32)
    _refuse(_host_lib().vrg_anchor_check(C.c_void_p(desc.ctypes.data), len(desc), C.c_void_p(tables.ctypes.data) if tables.size else None,
                                         int(tables.size), int(src_bytes), int(height), int(width)),
            "anchor_frames", "vrg_anchor_check refuses the records (a picture or a table outside its buffer, or a tap outside its axis)",
            "not built -- a picture more than 100 times as tall as wide whose height shrinks (Pillow resizes those vertically first), "
            f"or a frame of {height} x {width} is larger than one launch takes")


def anchor_frames(pictures, out: Optional[torch.Tensor] = None, size=None) -> torch.Tensor:
    """``np.stack([np.asarray(Image.fromarray(p).resize((W, H), Image.Resampling.LANCZOS), dtype=np.float32) / 255.0 for p in pictures])``
    -- what the reference's Load Anchors nodes yield file by file -- as one launch: ``pictures`` are ``[h, w, 3]`` uint8 R,G,B tensors or
    arrays of any sizes, on the GPU or on the CPU (the CPU ones go up as bytes, in one upload), ``(W, H)`` is the first picture's size --
    or ``size``, for a later chunk of a sequence whose first picture came with an earlier call.
    Returns the ``[n, H, W, 3]`` fp32 device tensor, or writes ``out`` (contiguous, of that shape, on that device).  The records are
    checked on the host before the launch.  Inputs are never written."""
    what = "anchor_frames"
    pics = [_byte_picture(p, f"{what}: picture {i}", allow_empty=False) for i, p in enumerate(pictures)]
    desc, tables, src_bytes, (height, width) = anchor_plan([tuple(p.shape[:2]) for p in pics], size)
    dev = _placement([p.device for p in pics], what, "pictures", ring=False,
                     prefer=out.device if isinstance(out, torch.Tensor) and out.is_cuda else None)
    anchor_check(desc, tables, src_bytes, height, width)
    with torch.cuda.device(dev):
        dst = _checked_out(out, (len(pics), height, width, 3), torch.float32, dev, what)
        flat = [p.contiguous().reshape(-1) for p in pics]
        _disjoint(what, [("out", dst)], [(f"picture {i}", f) for i, f in enumerate(flat)])
        src = torch.cat([f.to(dev) for f in flat]) if any(p.is_cuda for p in pics) else torch.cat(flat).to(dev)
        table = _hip.upload_records(desc, dev, trailing=(tables,))
        at = len(desc) * ANCHOR_DESC.itemsize
        _hip.check(_hip.lib().vrg_anchor_frames_f32(_hip.ptr(src), src_bytes, _hip.ptr(table), len(desc),
                                                    C.c_void_p(table.data_ptr() + at) if tables.size else None, int(tables.size),
                                                    _hip.ptr(dst), height, width, _hip.current_stream()), "vrg_anchor_frames_f32")
    return dst


@_on_device
def anchor_store_bytes(images: torch.Tensor, bgr: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``(images[..., :3].clamp(0, 1) * 255).round().astype("uint8")`` of the reference's Store Anchors nodes for a device-resident fp32
    ``[N, H, W, C]`` batch, ``C >= 3``, as one launch: ``[N, H, W, 3]`` uint8 on the same device, R,G,B or -- ``bgr=True``, what
    ``cv2.imwrite`` takes -- B,G,R.  NaN gives 0 (numpy on x86).  ``out``: an optional contiguous uint8 tensor of that shape."""
    what = "anchor_store_bytes"
    x = _check_frames(images)
    if int(x.shape[0]) < 1 or min(int(v) for v in x.shape[1:3]) < 1:
        raise ValueError(_NO_ANCHOR_IMAGES)
    if int(x.shape[3]) < 3:
        raise ValueError(f"{what}: images must have at least 3 channels, got {int(x.shape[3])}")
    dst = _checked_out(out, (*x.shape[:3], 3), torch.uint8, x.device, what)
    _disjoint(what, [("out", dst)], [("images", x)])
    _hip.check(_hip.lib().vrg_anchor_store_u8(_hip.ptr(x), _hip.ptr(dst), x.numel() // int(x.shape[3]), int(x.shape[3]),
                                              _hip.ANCHOR_BGR if bgr else _hip.ANCHOR_RGB, _hip.current_stream()), "vrg_anchor_store_u8")
    return dst


# ---------------------------------------------------------------------------------------------
# The guidance combine of the LTX Sigma Advanced guider (_LTXSigmaAdvancedGuider.predict_noise, CustomLTXNodes.py:436-563 of the
# reference): CFG-star, CFG or APG, STG and the variance rescale between the model evaluations of a sampler step, in at most four
# streaming launches and their finishers (csrc/vrg_guidance.hip); every sum is fp64 and every derived scalar stays on the device
# ---------------------------------------------------------------------------------------------
GUIDANCE_MODES = ("CFG", "APG")
GUIDANCE_SPAN = _hip.GUIDANCE_SPAN      # elements of a row one workgroup takes


@dataclass
class GuidanceResult:
    guided: torch.Tensor
    negative: Optional[torch.Tensor] = None          # the CFG-star negative, where want_negative
    average: Optional[torch.Tensor] = None           # the new running average, in APG mode with a momentum
    launches: int = 0                                # kernels the call enqueued, the finishers included


def _guidance_operand(t, name: str, like: Optional[torch.Tensor]) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"ltx_guidance: {name} must be a tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"ltx_guidance: {name} must be float32, got {str(t.dtype).replace('torch.', '')}")
    if t.ndim not in (4, 5):
        raise ValueError(f"ltx_guidance: {name} must have 4 or 5 dimensions, got {t.ndim}")
    if like is not None and tuple(t.shape) != tuple(like.shape):
        raise ValueError(f"ltx_guidance: {name} is shaped {list(t.shape)}, positive {list(like.shape)}")
    if like is not None and t.device != like.device:
        raise ValueError(f"ltx_guidance: {name} lives on {t.device}, positive on {like.device}")
    return t.detach()


def guidance_desc(shape, *, has_negative: bool, has_perturbed: bool, cfg=1.0, stg_scale=0.0, rescale=0.0, cfg_star=False, mode="CFG", eta=1.0,
                  norm_threshold=0.0, momentum=0.0, has_average=False, want_negative=False) -> "_hip.GuidanceDesc":
    """The record of one call, no GPU needed: the layout of ``shape`` (rows of the last three dimensions, batches of shape[0]) and the
    Python scalars, formed in double and rounded to fp32 once.  Without a negative the star, the mode and ``want_negative`` say nothing;
    outside APG the threshold, the momentum and the average say nothing.  Checked by vrg_guidance_check."""
    if mode not in GUIDANCE_MODES:
        raise ValueError(f"ltx_guidance: mode must be one of {GUIDANCE_MODES}, got {mode!r}")
    shape = tuple(int(v) for v in shape)
    rows, row_len = math.prod(shape[:-3]), math.prod(shape[-3:])
    if rows * row_len < 1:
        raise ValueError(f"ltx_guidance: positive is empty ({list(shape)})")
    if float(rescale) != 0.0 and rows * row_len < 2:
        raise ValueError("ltx_guidance: positive has fewer than two elements, the rescale needs a standard deviation")
    apg = bool(has_negative) and mode == "APG"
    threshold = _f32(norm_threshold) if apg else 0.0
    with_momentum = apg and float(momentum) != 0.0
    desc = _hip.GuidanceDesc(rows=rows, row_len=row_len, batch=shape[0], mode=_hip.GUIDANCE_APG if mode == "APG" else _hip.GUIDANCE_CFG,
                             has_negative=int(bool(has_negative)), has_perturbed=int(bool(has_perturbed)),
                             cfg_star=int(bool(has_negative and cfg_star)), has_average=int(bool(with_momentum and has_average)),
                             has_momentum=int(with_momentum), has_threshold=int(threshold > 0.0), has_rescale=int(float(rescale) != 0.0),
                             want_negative=int(bool(has_negative and want_negative)), cfg_m1=_f32(float(cfg) - 1.0), eta=_f32(eta),
                             momentum=_f32(momentum), threshold=threshold, stg_scale=_f32(stg_scale), rescale=_f32(rescale),
                             one_minus_rescale=_f32(1.0 - float(rescale)))
    _refuse(_host_lib().vrg_guidance_check(C.byref(desc)), "ltx_guidance", f"vrg_guidance_check refuses the record of {list(shape)}",
            f"{list(shape)} is more than the launches take")
    return desc


class GuidancePlan:
    """One call of ``ltx_guidance``: its record, its scratch buffer (partial sums and derived scalars, device memory) and its launches, every
    one on the caller's current stream, in the order they are called here.  Nothing waits on the host."""

    def __init__(self, desc: "_hip.GuidanceDesc", device):
        self.desc = desc
        self.bytes = int(_host_lib().vrg_guidance_scratch_bytes(C.byref(desc)))
        self.scratch = torch.empty((self.bytes,), dtype=torch.uint8, device=device)
        self.launches = 0        # kernels enqueued (the finishers included), for the benchmark tool

    def _tail(self):
        return C.byref(self.desc), _hip.ptr(self.scratch), self.bytes, _hip.current_stream()

    @staticmethod
    def _ptr(t):
        return None if t is None else _hip.ptr(t)

    def run_sums(self, positive, negative):
        _hip.check(_hip.lib().vrg_guidance_sums_f32(_hip.ptr(positive), _hip.ptr(negative), *self._tail()), "vrg_guidance_sums_f32")
        self.launches += 2

    def run_rows(self, positive, negative, average, average_out):
        _hip.check(_hip.lib().vrg_guidance_rows_f32(_hip.ptr(positive), _hip.ptr(negative), self._ptr(average), self._ptr(average_out),
                                                    *self._tail()), "vrg_guidance_rows_f32")
        self.launches += 2

    def run_combine(self, positive, negative, perturbed, guidance, guided, negative_out):
        _hip.check(_hip.lib().vrg_guidance_combine_f32(_hip.ptr(positive), self._ptr(negative), self._ptr(perturbed), self._ptr(guidance),
                                                       _hip.ptr(guided), self._ptr(negative_out), *self._tail()), "vrg_guidance_combine_f32")
        self.launches += 2 if self.desc.has_rescale else 1

    def run_rescale(self, guided):
        _hip.check(_hip.lib().vrg_guidance_rescale_f32(_hip.ptr(guided), *self._tail()), "vrg_guidance_rescale_f32")
        self.launches += 1


@_on_device
def ltx_guidance(positive: torch.Tensor, negative: Optional[torch.Tensor] = None, perturbed: Optional[torch.Tensor] = None, *, cfg=1.0,
                 stg_scale=0.0, rescale=0.0, cfg_star=False, mode="CFG", eta=1.0, norm_threshold=0.0, momentum=0.0,
                 average: Optional[torch.Tensor] = None, want_negative=False) -> GuidanceResult:
    """What the reference's LTX Sigma Advanced guider computes between its model evaluations, for device-resident fp32 latents of one
    shape with 4 or 5 dimensions (rows = the last three dimensions, batches = shape[0]):

    ``negative *= sum(p * n) / (sum(n * n) + 1e-8)`` per batch (``cfg_star``); ``p + (cfg - 1.0) * (p - n)`` (mode "CFG") or the APG
    form -- ``g = p - n``, ``g = momentum * average + g`` (the new average; ``average=None``: g as it is), the per-row norm threshold,
    the fp64 projection on ``p``, ``p + (cfg - 1.0) * (orth + eta * par)``; without a negative ``p``; ``+ stg_scale * (p - perturbed)``
    where ``perturbed`` is given; ``* (rescale * std(p) / max(std(guided), 1e-12) + (1.0 - rescale))`` where ``rescale != 0``.

    Returns ``GuidanceResult(guided, negative, average)``: ``guided`` always a fresh tensor, ``negative`` the CFG-star negative where
    ``want_negative`` (and a negative is given), ``average`` the new running average in APG mode with ``momentum != 0``.  No output shares
    memory with an input; no input is written (``average`` is read only).  All sums are fp64 and deterministic; the call never waits
    for the device."""
    p = _guidance_operand(positive, "positive", None)
    n = None if negative is None else _guidance_operand(negative, "negative", p)
    q = None if perturbed is None else _guidance_operand(perturbed, "perturbed", p)
    a = None if average is None else _guidance_operand(average, "average", p)
    desc = guidance_desc(p.shape, has_negative=n is not None, has_perturbed=q is not None, cfg=cfg, stg_scale=stg_scale, rescale=rescale,
                         cfg_star=cfg_star, mode=mode, eta=eta, norm_threshold=norm_threshold, momentum=momentum, has_average=a is not None,
                         want_negative=want_negative)
    if not p.is_cuda:
        raise ValueError(f"ltx_guidance: positive lives on {p.device}; the operator runs on the GPU and has no CPU form")
    p, n, q = (None if t is None else t.contiguous() for t in (p, n, q))
    a = a.contiguous() if desc.has_average else None
    plan = GuidancePlan(desc, p.device)
    guided = torch.empty_like(p)
    negative_out = torch.empty_like(p) if desc.want_negative else None
    average_out = torch.empty_like(p) if desc.has_momentum else None
    _disjoint("ltx_guidance", [("guided", guided), ("the negative result", negative_out), ("the average result", average_out)],
              [("positive", p), ("negative", n), ("perturbed", q), ("average", a)])
    if desc.cfg_star:
        plan.run_sums(p, n)
    if desc.has_negative and desc.mode == _hip.GUIDANCE_APG:
        plan.run_rows(p, n, a, average_out)
    plan.run_combine(p, n, q, average_out, guided, negative_out)
    if desc.has_rescale:
        plan.run_rescale(guided)
    return GuidanceResult(guided, negative_out, average_out, plan.launches)


# ---------------------------------------------------------------------------------------------
# The Video Compare Slider's IMAGE batches as the rgb24 bytes of its ffmpeg pipe (_write_image_batch_video, VRGDG_VideoCompareNode.py:63-107
# of the reference): quantised where the frames live (csrc/vrg_compare.hip), so 3 B/px cross PCIe instead of 12 (16 with alpha) and a
# pending result of this pack never becomes fp32 on the host
# ---------------------------------------------------------------------------------------------
_NO_RGB24_IMAGES = "{} image input must be a non-empty IMAGE batch."           # the reference's text behind its label


class Rgb24Handoff:
    """One ``stream_rgb24`` call: the pieces of a batch, in frame order, each quantised on the device (one launch), downloaded into one of
    two host buffers (page-locked; pageable where the host refuses to lock) and handed to ``sink(memoryview)``.  Everything is queued on
    the caller's current stream; the sink call for a piece is made after the launch and the download of the next piece have been queued,
    so the two overlap.  The memory a sink is given is its own until it returns (the buffer is written again two pieces later).

    ``rgb24_frames`` and ``stream_rgb24`` are this class's two entry points."""

    def __init__(self, sink, frame_bytes: int, per: int):
        self.sink, self.frame_bytes, self.per = sink, int(frame_bytes), int(per)
        self.buffers = [self._host_buffer(self.per * self.frame_bytes) for _ in range(2)]
        self.queued = None          # (event behind its download, host bytes) of the piece the sink has not seen yet
        self.pieces = self.frames = 0

    @staticmethod
    def _host_buffer(nbytes: int) -> torch.Tensor:
        try:
            return torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
        except RuntimeError:
            return torch.empty((nbytes,), dtype=torch.uint8)

    @staticmethod
    def _checked(images, what: str) -> torch.Tensor:
        x = images.unsqueeze(0) if isinstance(images, torch.Tensor) and images.ndim == 3 else images
        if not isinstance(x, torch.Tensor) or x.ndim != 4 or min(int(v) for v in x.shape[:3]) < 1 or int(x.shape[3]) < 3:
            raise ValueError(_NO_RGB24_IMAGES.format(what))
        return _check_frames(x)

    @classmethod
    @_on_device
    def launch(cls, images: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``rgb24_frames``"""
        what = "rgb24_frames"
        x = cls._checked(images, what)
        dst = _checked_out(out, (*x.shape[:3], 3), torch.uint8, x.device, what)
        _disjoint(what, [("out", dst)], [("images", x)])
        _hip.check(_hip.lib().vrg_rgb24_frames_u8(_hip.ptr(x), _hip.ptr(dst), x.numel() // int(x.shape[3]), int(x.shape[3]),
                                                  _hip.current_stream()), "vrg_rgb24_frames_u8")
        return dst

    def _give(self, queued):
        """the piece whose download `queued` stands for to the sink; if the sink raises, the download still in flight is waited for first"""
        done, host = queued
        try:
            done.synchronize()
            self.sink(memoryview(host.numpy()))
        except BaseException:
            if self.queued is not None:
                self.queued[0].synchronize()
                self.queued = None
            raise

    def feed(self, gpu_frames: torch.Tensor) -> None:
        """the next frames of the batch, device-resident: piece by piece"""
        for s in range(0, int(gpu_frames.shape[0]), self.per):
            data = self.launch(gpu_frames[s:s + self.per]).view(-1)
            host = self.buffers[self.pieces % 2][:data.numel()]
            host.copy_(data, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            before, self.queued = self.queued, (done, host)
            self.pieces += 1
            self.frames += data.numel() // self.frame_bytes
            if before is not None:
                self._give(before)

    def finish(self) -> int:
        before, self.queued = self.queued, None
        if before is not None:
            self._give(before)
        return self.frames

    @classmethod
    def stream(cls, images: torch.Tensor, sink, piece_bytes: int = 0) -> int:
        """``stream_rgb24``"""
        from . import _devices
        what = "stream_rgb24"
        shape = tuple(int(v) for v in getattr(images, "shape", ()))
        shape = (1,) + shape if len(shape) == 3 else shape
        if not isinstance(images, torch.Tensor) or len(shape) != 4 or min(shape[:3]) < 1 or shape[3] < 3:
            raise ValueError(_NO_RGB24_IMAGES.format(what))
        if images.dtype != torch.float32:
            raise ValueError(f"{what}: images must be float32")
        pending = _devices.pending_of(images)
        dev = images.device if images.is_cuda else _devices.compute_device()
        frame_bytes = shape[1] * shape[2] * 3
        with torch.cuda.device(dev):
            handoff = cls(sink, frame_bytes, _devices.piece_frames(shape[0], frame_bytes, 1, int(piece_bytes)))
            if pending is not None and pending.device == dev:
                handoff.feed(_devices.on_device(images, dev))                # the device pieces behind a pending result, where they lie
            elif images.is_cuda:
                handoff.feed(_devices.materialise(images).detach().reshape(shape))
            else:
                _devices.upload_frames(_devices.materialise(images).detach().reshape(shape), lambda gpu, first: handoff.feed(gpu))
            return handoff.finish()


# The two operators are bound methods of the hand-off class, as GuidancePlan's launches are methods: the operator tables of
# tests/overlap_support.py and tests/stream_support.py list the module-level functions of ops, and these two are held to the same
# overlap and stream contracts by tests/test_gpu_compare.py.
#: ``np.clip(images[..., :3] * 255.0, 0, 255).astype(np.uint8)`` of the reference's compare node for a device-resident fp32 ``[N, H, W, C]``
#: or ``[H, W, C]`` batch, ``C >= 3``, as one launch on the caller's current stream: ``rgb24_frames(images, out=None)`` returns
#: ``[N, H, W, 3]`` uint8 on the same device, R,G,B, truncated (not rounded: ``anchor_store_bytes`` rounds), NaN 0, +Inf 255; ``out``: an
#: optional contiguous uint8 tensor of that shape that does not overlap the input.  An empty batch is a ValueError with the reference's text.
rgb24_frames = Rgb24Handoff.launch
#: ``stream_rgb24(images, sink, piece_bytes=0) -> frames written``: the whole hand-off of a batch to a byte consumer.  A CUDA batch is
#: used where it lies, a pending ``LazyFrames`` of the compute device through ``_devices.on_device`` (no fp32 download, no upload), a CPU
#: batch through ``_devices.upload_frames``.  Pieces along the frame axis hold ``piece_bytes`` of OUTPUT bytes (default: ``_devices.PIPE_BYTES``).
#: An exception of the sink propagates unchanged once the download in flight has been waited for; nothing is launched after it.
stream_rgb24 = Rgb24Handoff.stream

"""Support for the assembly tests: the reference's assembly nodes restated in numpy, written from the reference's text and independently
of csrc/vrg_assemble_math.hpp; a deterministic stand-in for cv2.putText; the case table; the header compiled for the host; the five
classes' surface transcribed as literals.

The quantisation chain, enumerated by test_assemble_host.py::test_quantisation_levels on numpy and on the header: of the 256 levels k,
``trunc(fl(fl(k / 255) * 255))`` drops below k for NONE -- levels that drop by one: [] (IEEE fp32, correctly rounded quotient and
product, so every machine agrees).  The second quantisation of the reference's labelled MP4 therefore changes no byte; it is evaluated all
the same, by the kernel and by the restatement below."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import PKG_DIR, ROOT

F32 = np.float32
BAR = 60
SLOTS = 16
LEVELS_THAT_DROP = []


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference restated.  A "video" is any numpy array whose axis 0 is frames.
# ---------------------------------------------------------------------------------------------------------------------------------------
def v2_target(durations, idx, fps, current_frames):
    try:
        dur_sec = float(durations[idx])
    except Exception:
        dur_sec = 0.0
    if dur_sec > 0.0:
        return max(1, int(round(dur_sec * float(fps))))
    return int(current_frames)


def v2_trim_or_pad(video, target_frames, pad_short=False):
    cur = int(video.shape[0])
    if cur > target_frames:
        return video[:target_frames]
    if cur < target_frames and pad_short:
        need = target_frames - cur
        last = video[-1:].copy()
        return np.concatenate([video, np.repeat(last, need, axis=0)], axis=0)
    return video


def v3_target(durations, idx, fps, is_frames=False):
    value = float(durations[idx])
    if is_frames:
        return max(1, int(round(value)))
    return max(1, int(round(fps * value)))


def v3_trim_or_pad(video, target_frames):
    cur = int(video.shape[0])
    if cur > target_frames:
        return video[:target_frames]
    return video


def combine_v2(videos, fps, audio_meta):
    """the list of trimmed / padded clips of VRGDG_CombinevideosV2.blend_videos, before its cat"""
    if isinstance(audio_meta, dict) and "durations" in audio_meta and isinstance(audio_meta["durations"], (list, tuple)):
        meta = list(audio_meta.get("durations", []))
        if len(meta) < SLOTS:
            meta += [0.0] * (SLOTS - len(meta))
        durations = meta[:SLOTS]
    else:
        durations = [0.0] * SLOTS
    vids = [(i, videos[i - 1]) for i in range(1, SLOTS + 1) if i - 1 < len(videos) and videos[i - 1] is not None]
    return [v2_trim_or_pad(v, v2_target(durations, slot - 1, fps, v.shape[0]), pad_short=True) for slot, v in vids]


def combine_v3(videos, fps, audio_meta, index, total_sets, groups_in_last_set):
    """the (slot, trimmed clip) list of VRGDG_CombinevideosV3 / V5.blend_videos, before the cat (the two differ in texts only)"""
    is_last_run = index == total_sets - 1
    frames, seconds = audio_meta.get("durations_frames"), audio_meta.get("durations")
    if frames is not None:
        durations, is_frames = list(frames), True
    else:
        durations, is_frames = list(seconds), False
    if len(durations) < SLOTS:
        durations += [0.0] * (SLOTS - len(durations))
    else:
        durations = durations[:SLOTS]
    limit = SLOTS
    if is_last_run:
        limit = max(1, min(groups_in_last_set, SLOTS))
    vids = [(i, videos[i - 1]) for i in range(1, limit + 1) if i - 1 < len(videos) and videos[i - 1] is not None]
    out = []
    for slot, v in vids:
        tgt = v3_target(durations, slot - 1, fps, is_frames)
        if is_last_run and slot > groups_in_last_set:
            continue
        out.append((slot, v3_trim_or_pad(v, tgt)))
    return out


def pad_video(images, pad_frames, pad_front):
    if images.shape[0] == 0 or pad_frames <= 0:
        return images
    frame = images[:1].copy() if pad_front else images[-1:].copy()
    padded = np.repeat(frame, pad_frames, axis=0)
    return np.concatenate([padded, images], axis=0) if pad_front else np.concatenate([images, padded], axis=0)


def restated_clips(mode, videos, fps=25.0, audio_meta=None, index=0, total_sets=1, groups_in_last_set=16, pad_frames=1, pad_front=False):
    """[(slot, clip)] in output order for any of the five nodes"""
    if mode == "v2":
        slots = [i for i in range(1, SLOTS + 1) if i - 1 < len(videos) and videos[i - 1] is not None]
        return list(zip(slots, combine_v2(videos, fps, audio_meta)))
    if mode in ("v3", "v5"):
        return combine_v3(videos, fps, audio_meta, index, total_sets, groups_in_last_set)
    if mode == "pad":
        return [(1, pad_video(videos[0], pad_frames, pad_front))]
    return [(i + 1, v) for i, v in enumerate(videos) if v is not None and v.shape[0]]


def index_videos(lengths):
    """clips whose "pixels" are their own (source, frame) pair: the restatement then returns the plan"""
    return [None if n is None else np.stack([np.full(n, i), np.arange(n)], axis=1).reshape(n, 2) for i, n in enumerate(lengths)]


def restated_plan(mode, lengths, **kw):
    clips = [c for _, c in restated_clips(mode, index_videos(lengths), **kw)]
    return [tuple(int(v) for v in row) for row in np.concatenate(clips, axis=0)] if clips else []


def label_bar_bytes(video, overlay_bgr=None):
    """_add_label_bar followed by the per-frame work of _save_video: what the writer receives for one clip, [F, H + 60, W, 3] B,G,R.
    `overlay_bgr` stands for what cv2.putText leaves in the bar."""
    out = []
    for frame in video:
        frame_uint8 = (frame * 255).astype(np.uint8)
        frame_bgr = frame_uint8[:, :, ::-1]                                # cv2.COLOR_RGB2BGR
        h, w, _ = frame_bgr.shape
        new_frame = np.zeros((h + BAR, w, 3), dtype=np.uint8)
        new_frame[:h, :, :] = frame_bgr
        if overlay_bgr is not None:
            new_frame[h:, :, :] = overlay_bgr
        labelled = new_frame[:, :, ::-1].astype(np.float32) / 255.0        # COLOR_BGR2RGB, normalise
        saved = (labelled * 255).astype(np.uint8)                          # _save_video
        out.append(saved[:, :, ::-1])
    return np.stack(out)


def pattern_bar(slot, width):
    """a deterministic stand-in for the label pixels of group `slot`: every byte level appears, [60, width, 3] uint8"""
    yy, xx = np.mgrid[0:BAR, 0:int(width)]
    return np.stack([((xx * 7 + yy * 13 + 31 * int(slot) + 29 * c) % 256).astype(np.uint8) for c in range(3)], axis=2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def special_clip(shape, seed):
    """fp32 frames holding NaN (two payloads), +-Inf, -0.0 and the subnormal 1e-40 among ordinary values: for the bit-exact join"""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    x = rng.random(shape, dtype=F32)
    pick = rng.integers(0, 12, shape)
    bits = x.view(np.uint32).copy()
    for which, word in ((0, 0x7fc00000), (1, 0xffa5a5a5), (2, 0x7f800000), (3, 0xff800000), (4, 0x80000000)):
        bits[pick == which] = word
    bits[pick == 5] = np.array(1e-40, dtype=F32).view(np.uint32)
    return bits.view(F32)


def contract_clip(shape, seed):
    """fp32 frames inside the labelled contract (finite, 0 <= x * 255 < 256): k / 255 and its two neighbours, and uniform values"""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    k = rng.integers(0, 256, shape).astype(F32) / F32(255.0)
    pick = rng.integers(0, 4, shape)
    x = np.where(pick == 0, np.nextafter(k, F32(2.0)), np.where(pick == 1, np.nextafter(k, F32(-1.0)), k)).astype(F32)
    x = np.where(pick == 3, rng.random(shape, dtype=F32), x).astype(F32)
    x = np.where(x < 0, F32(0.0), x).astype(F32)
    assert np.isfinite(x).all() and ((x * 255 >= 0) & (x * 255 < 256)).all()
    return x


def bytes_clip(shape, seed):
    return np.random.Generator(np.random.PCG64(int(seed))).integers(0, 256, shape, dtype=np.uint8)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    view = np.uint32 if a.dtype == np.float32 else a.dtype
    return int((a.view(view) != b.view(view)).sum())


# name, (H, W, C), clip lengths by slot (None = not connected), mode, arguments of the plan
CASES = [
    dict(name="v3-vector-4x4", hwc=(4, 4, 3), lengths=[3, None, 5, 2], mode="v3", kw=dict(fps=25.0, audio_meta={"durations": [0.1, 9, 0.12, 4.0]})),
    dict(name="v3-dword-5x7", hwc=(5, 7, 3), lengths=[3, None, 5, 2], mode="v3", kw=dict(fps=25.0, audio_meta={"durations_frames": [2.5, 1, 3.5, 7]})),
    dict(name="v5-sixteen", hwc=(5, 7, 3), lengths=[1 + i % 5 for i in range(16)], mode="v5",
         kw=dict(fps=10.0, audio_meta={"durations": [0.1 * (1 + (i * 3) % 7) for i in range(16)]})),
    dict(name="v5-last-run", hwc=(4, 4, 3), lengths=[2, 3, 4, 5, 1, 2], mode="v5",
         kw=dict(fps=25.0, audio_meta={"durations_frames": [2, 2, 9, 1]}, index=2, total_sets=3, groups_in_last_set=5)),
    dict(name="v2-pad", hwc=(5, 7, 3), lengths=[2, 4, None, 3], mode="v2", kw=dict(fps=25.0, audio_meta={"durations": [0.2, 0.08, 1.0, 0.0]})),
    dict(name="single", hwc=(4, 4, 3), lengths=[4], mode="v3", kw=dict(fps=25.0, audio_meta={"durations": [0.1]})),
    dict(name="pad-front", hwc=(5, 7, 3), lengths=[3], mode="pad", kw=dict(pad_frames=2, pad_front=True)),
    dict(name="pad-tail", hwc=(4, 4, 3), lengths=[3], mode="pad", kw=dict(pad_frames=3, pad_front=False)),
    dict(name="rgba-join", hwc=(3, 5, 4), lengths=[2, 3], mode="load", kw={}),
    dict(name="two-tiles", hwc=(33, 37, 3), lengths=[2, 1], mode="load", kw={}),          # 1221 px: a whole 1024-pixel tile and a part
    dict(name="two-tiles-vector", hwc=(32, 36, 3), lengths=[1, 2], mode="load", kw={}),   # 1152 px, px % 4 == 0
]


def case_clips(case, kind="special"):
    make = {"special": special_clip, "contract": contract_clip, "bytes": bytes_clip}[kind]
    return [None if n is None else make((n, *case["hwc"]), 100 + 17 * i) for i, n in enumerate(case["lengths"])]


def expected_join(case, clips):
    parts = [c for _, c in restated_clips(case["mode"], clips, **case["kw"])]
    return np.concatenate(parts, axis=0)


def expected_labelled(case, clips, with_overlays):
    parts = []
    for slot, clip in restated_clips(case["mode"], clips, **case["kw"]):
        parts.append(label_bar_bytes(clip, pattern_bar(slot, case["hwc"][1]) if with_overlays else None))
    return np.concatenate(parts, axis=0)


def overlays_for(case):
    return [None if n is None else pattern_bar(i + 1, case["hwc"][1]) for i, n in enumerate(case["lengths"])]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the header on the host
# ---------------------------------------------------------------------------------------------------------------------------------------
HOST_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse"]


def build_host_lib(directory):
    out = os.path.join(str(directory), "libassemble_check.so")
    subprocess.run(["g++", *HOST_FLAGS, "-fPIC", "-shared", "-I", os.path.join(PKG_DIR, "csrc"),
                    os.path.join(ROOT, "tests", "host_math", "assemble_check.cpp"), "-o", out], check=True)
    lib = C.CDLL(out)
    P = C.c_void_p
    lib.hm_assemble_levels.argtypes = [P, P]
    lib.hm_assemble_levels.restype = None
    lib.hm_assemble_label_bytes.argtypes = [P, C.c_int64, P]
    lib.hm_assemble_label_bytes.restype = None
    lib.hm_assemble_frame_offset.argtypes = [C.c_int64, C.c_uint32]
    lib.hm_assemble_frame_offset.restype = C.c_int64
    lib.hm_assemble_grid_x.argtypes = [C.c_int64, C.c_int64]
    lib.hm_assemble_grid_x.restype = C.c_uint32
    for name in ("hm_assemble_on_grid", "hm_assemble_check"):
        getattr(lib, name).restype = C.c_int
    lib.hm_assemble_on_grid.argtypes = [P, P, P, C.c_int32]
    lib.hm_assemble_check.argtypes = [P, P, C.c_int64, P, P, C.c_int32]
    lib.hm_assemble_join.argtypes = [P, P, C.c_int64, P]
    lib.hm_assemble_labelled.argtypes = [P, P, C.c_int64, P]
    return lib


def host_desc(hip, arrays, overlays=None, is_bytes=False):
    """a vrg_assemble_desc over host arrays (for the header's plain loops and the checks)"""
    d = hip.AssembleDesc()
    d.n_src, d.bytes = len(arrays), int(is_bytes)
    for k, a in enumerate(arrays):
        d.src[k], d.frames[k] = a.ctypes.data, a.shape[0]
        d.height[k], d.width[k], d.channels[k] = a.shape[1:]
        if overlays is not None and overlays[k] is not None:
            d.overlay[k] = overlays[k].ctypes.data
    return d


# ---------------------------------------------------------------------------------------------------------------------------------------
# the surface of the five classes, transcribed from the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
_VIDEOS = {f"video_{i}": ("IMAGE",) for i in range(1, 17)}
_V3_REQUIRED = {
    "fps": ("FLOAT", {"default": 25.0, "min": 1.0}),
    "duration": ("FLOAT", {"default": 4.0, "min": 0.01}),
    "audio_meta": ("DICT",),
    "index": ("INT", {"default": 0, "min": 0}),
    "total_sets": ("INT", {"default": 1, "min": 1}),
    "groups_in_last_set": ("INT", {"default": 16, "min": 0, "max": 16}),
}
SURFACE = {
    "VRGDG_CombinevideosV2": dict(
        INPUT_TYPES={"required": {"fps": ("FLOAT", {"default": 25.0, "min": 1.0}), "audio_meta": ("DICT",)}, "optional": dict(_VIDEOS)},
        RETURN_TYPES=("IMAGE",), RETURN_NAMES=("blended_video_frames",), FUNCTION="blend_videos", CATEGORY="Video"),
    "VRGDG_CombinevideosV3": dict(
        INPUT_TYPES={"required": dict(_V3_REQUIRED), "optional": dict(_VIDEOS)},
        RETURN_TYPES=("IMAGE",), RETURN_NAMES=("blended_video_frames",), FUNCTION="blend_videos", CATEGORY="Video", VERSION="v3.1_fixed"),
    "VRGDG_CombinevideosV5": dict(
        INPUT_TYPES={"required": {**_V3_REQUIRED,
                                  "folder_path": ("STRING", {"default": "./output_videos"}),
                                  "with_labels": ("BOOLEAN", {"default": True, "label": "Add Labels and Save Video",
                                                              "tooltip": "If enabled, adds label bars and saves labeled video to WithLabels/."})},
                     "optional": dict(_VIDEOS)},
        RETURN_TYPES=("IMAGE",), RETURN_NAMES=("blended_video_frames",), FUNCTION="blend_videos", CATEGORY="Video", VERSION="v3.9_label_safe"),
    "VRGDG_PadVideoWithLastFrame": dict(
        INPUT_TYPES={"required": {"images": ("IMAGE",), "pad_frames": ("INT", {"default": 1, "min": 0, "max": 1000, "step": 1}),
                                  "pad_front": ("BOOLEAN", {"default": False})}},
        RETURN_TYPES=("IMAGE",), RETURN_NAMES=("images",), FUNCTION="pad_video", CATEGORY="video/utils"),
    "VRGDG_LoadVideos": dict(
        INPUT_TYPES={"required": {"trigger": ("*", {}), "video_folder": ("STRING", {"default": "./videos", "multiline": False}),
                                  "scene_count": ("INT", {"default": 3, "min": 1, "max": 5})}},
        RETURN_TYPES=("IMAGE",), RETURN_NAMES=("video",), FUNCTION="load_videos", CATEGORY="Video"),
}
DISPLAY_NAMES = {
    "VRGDG_CombinevideosV2": "🌀 VRGDG_CombinevideosV2",
    "VRGDG_CombinevideosV3": "🎬 VRGDG Combine Videos V3",
    "VRGDG_CombinevideosV5": "VRGDG_CombinevideosV5",
    "VRGDG_PadVideoWithLastFrame": "VRGDG_PadVideoWithLastFrame",
    "VRGDG_LoadVideos": "VRGDG_LoadVideos",
}

"""ctypes binding of libvrgdg_hip.so (the C ABI declared in include/vrgdg_hip.h).

There is NO CPU fallback: if the library is missing, or no HIP device is visible, every op raises.

The self-tests and probes of include/vrgdg_hip_debug.h live in a second library, libvrgdg_hip_debug.so, that nothing of the product loads:
it is opened the first time a test or a tool asks the handle for one of its names (`lib().vrg_debug_...`).
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import threading

import numpy as np
import torch

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VRGDG_HIP_LIB") or os.path.join(PKG_DIR, "libvrgdg_hip.so")   # override: A/B builds (tools/build_variant.py, tools/ab_interleaved.py)
DEBUG_LIB_PATH = os.path.join(PKG_DIR, "libvrgdg_hip_debug.so")

VRG_OK = 0
VRG_ERR_BAD_ARG = 1
VRG_ERR_UNSUPPORTED = 2
BORDER_REPLICATE, BORDER_ZERO = 0, 1
STENCIL_UNSHARP, STENCIL_LAPLACIAN, STENCIL_SOBEL = 0, 1, 2
STAGE_GRAIN, STAGE_LUT, STAGE_COLORMATCH, STAGE_SHARPEN, STAGE_FROM_LAB = 1, 2, 4, 8, 16
CM_MATH_DEVICE, CM_MATH_FAST = 0, 1
ADJUST_DIV_IEEE, ADJUST_DIV_DEVICE = 0, 1
RESIZE_BICUBIC, RESIZE_BILINEAR, RESIZE_AREA, RESIZE_NEAREST = 0, 1, 2, 3
COMPOSITE_NONE, COMPOSITE_ELLIPSE, COMPOSITE_RECTANGLE, COMPOSITE_RADIAL, COMPOSITE_OPAQUE = 0, 1, 2, 3, 4
COMPOSITE_CLAMP_CROP, COMPOSITE_MATCH, COMPOSITE_STEP, COMPOSITE_USER_MASK, COMPOSITE_RAW_COPY = 1, 2, 4, 8, 16
COMPOSITE_STATS_WORDS = 16
ABI_VERSION = 8


class Record(C.Structure):
    """A record the host fills for a kernel: each subclass is the ONLY Python declaration of the struct `c_name` of `c_header` (a path from
    the repository's root).  The numpy layouts derive from it (record_dtype); tests/test_abi.py compiles the header and compares them."""
    c_name, c_header = None, "include/vrgdg_hip.h"


class NoiseDesc(Record):
    c_name = "vrg_noise_desc"
    _fields_ = [("seed0", C.c_uint64), ("seed_stride", C.c_uint64), ("offset0", C.c_uint64),
                ("offset_stride", C.c_uint64), ("chunk0", C.c_int64), ("chunk_frames", C.c_int32),
                ("grid_threads", C.c_uint32)]


NOISE_LEAVES_MAX = 8            # include/vrgdg_hip.h: VRG_NOISE_LEAVES_MAX


class NoiseLeaf(Record):
    c_name = "vrg_noise_leaf"
    _fields_ = [("start", C.c_int64), ("size", C.c_uint32), ("grid_threads", C.c_uint32), ("offset", C.c_uint64)]


class NoiseSplit(Record):
    c_name = "vrg_noise_split"
    _fields_ = [("seed", C.c_uint64), ("count", C.c_int32), ("reserved", C.c_int32), ("leaves", NoiseLeaf * NOISE_LEAVES_MAX)]

    @classmethod
    def of(cls, seed: int, leaves) -> "NoiseSplit":
        """The record of the leaves [(start, size, grid_threads, offset), ...] a launch meets (rng.SplitStream.leaves_of)"""
        if not 1 <= len(leaves) <= NOISE_LEAVES_MAX:
            raise ValueError(f"a launch takes 1 to {NOISE_LEAVES_MAX} noise leaves, not {len(leaves)}")
        rec = cls(seed=seed, count=len(leaves))
        for i, (start, size, G, off) in enumerate(leaves):
            rec.leaves[i] = NoiseLeaf(start=start, size=size, grid_threads=G, offset=off)
        return rec


class ChainDesc(Record):
    c_name = "vrg_chain_desc"
    _fields_ = [("stages", C.c_int32), ("variant", C.c_int32),
                ("intensity", C.c_float), ("sat", C.c_float), ("one_minus_sat", C.c_float),
                ("noise", NoiseDesc),
                ("lut", C.c_void_p), ("lut_size", C.c_int32),
                ("domain_min", C.c_float * 3), ("domain_max", C.c_float * 3),
                ("blend_mode", C.c_int32), ("blend", C.c_float), ("one_minus_blend", C.c_float),
                ("img_ms", C.c_void_p), ("ref_ms", C.c_void_p), ("ref_frames", C.c_int32),
                ("k", C.c_float), ("one_minus_k", C.c_float),
                ("stencil_op", C.c_int32), ("border", C.c_int32), ("strength", C.c_float),
                ("cm_math", C.c_int32)]


class AdjustDesc(Record):
    c_name = "vrg_adjust_desc"
    _fields_ = [("enabled", C.c_int32), ("shift", C.c_float * 3), ("exposure", C.c_float),
                ("contrast", C.c_float), ("saturation", C.c_float),
                ("highlights", C.c_float), ("shadows", C.c_float), ("whites", C.c_float), ("blacks", C.c_float),
                ("has_clarity", C.c_int32), ("clarity", C.c_float),
                ("has_sharpen", C.c_int32), ("sharpen", C.c_float),
                ("has_fade", C.c_int32), ("fade_mul", C.c_float), ("fade_add", C.c_float),
                ("has_vignette", C.c_int32), ("vignette", C.c_float),
                ("div_mode", C.c_int32)]


class CompositeDesc(Record):
    c_name = "vrg_composite_desc"
    _fields_ = [("rule", C.c_int32), ("flags", C.c_int32),
                ("original_index", C.c_int32), ("crop_index", C.c_int32), ("mask_index", C.c_int32),
                ("left", C.c_int32), ("top", C.c_int32), ("box_w", C.c_int32), ("box_h", C.c_int32),
                ("paste_w", C.c_int32), ("paste_h", C.c_int32),
                ("match_strength", C.c_float), ("threshold", C.c_float), ("p", C.c_float * 7)]


class CropDesc(Record):
    c_name = "vrg_crop_desc"
    _fields_ = [("src_offset", C.c_int64), ("row_pitch", C.c_int32), ("pixel_stride", C.c_int32),
                ("box_w", C.c_int32), ("box_h", C.c_int32), ("reserved", C.c_int32 * 2)]


class WarpDesc(Record):
    c_name = "vrg_warp_desc"
    _fields_ = [("m", C.c_double * 6), ("src_offset", C.c_int64), ("src_w", C.c_int32), ("src_h", C.c_int32),
                ("set", C.c_int32), ("reserved", C.c_int32)]


WARP_TABLE_BYTES = 1024 * 64 * 2


class FaceFixBoxDesc(Record):
    c_name = "vrg_ff_box_desc"
    _fields_ = [("frame", C.c_int32), ("left", C.c_int32), ("top", C.c_int32), ("box_w", C.c_int32), ("box_h", C.c_int32),
                ("reserved", C.c_int32), ("taps_offset", C.c_int64)]


class FaceFixMaskDesc(Record):
    c_name = "vrg_ff_mask_desc"
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("span_offset", C.c_int64), ("mask_offset", C.c_int64)]


class FaceFixDesc(Record):
    c_name = "vrg_ff_desc"
    _fields_ = [("enhanced_index", C.c_int32), ("left", C.c_int32), ("top", C.c_int32), ("box_w", C.c_int32), ("box_h", C.c_int32),
                ("strength", C.c_float), ("mask_offset", C.c_int64), ("taps_offset", C.c_int64), ("bytes_offset", C.c_int64)]


class FaceFixPackedDesc(Record):
    c_name = "vrg_ff_packed_desc"
    _fields_ = [("src_offset", C.c_int64), ("dst_offset", C.c_int64), ("box_w", C.c_int32), ("box_h", C.c_int32),
                ("enhanced_index", C.c_int32), ("strength", C.c_float), ("mask_offset", C.c_int64), ("taps_offset", C.c_int64),
                ("bytes_offset", C.c_int64)]


class DetectDesc(Record):
    c_name = "vrg_detect_desc"
    _fields_ = [("frame", C.c_int32), ("transform", C.c_int32), ("left", C.c_int32), ("top", C.c_int32), ("right", C.c_int32),
                ("bottom", C.c_int32)]


class DetectFrameDesc(Record):
    c_name = "vrg_detect_frame_desc"
    _fields_ = [("frame", C.c_int32), ("transform", C.c_int32)]


class PilResizeDesc(Record):
    c_name = "vrg_pil_resize_desc"
    _fields_ = [("src_offset", C.c_int64), ("dst_offset", C.c_int64), ("tmp_offset", C.c_int64), ("h_table", C.c_int64), ("v_table", C.c_int64),
                ("in_w", C.c_int32), ("in_h", C.c_int32), ("out_w", C.c_int32), ("out_h", C.c_int32), ("h_ksize", C.c_int32),
                ("v_ksize", C.c_int32)]


class PilMaskDesc(Record):
    c_name = "vrg_pil_mask_desc"
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("radius", C.c_int32), ("ww", C.c_uint32), ("fw", C.c_uint32),
                ("reserved", C.c_int32), ("span_offset", C.c_int64), ("mask_offset", C.c_int64)]


class PilBoxDesc(Record):
    c_name = "vrg_pil_box_desc"
    _fields_ = [("left", C.c_int32), ("top", C.c_int32), ("box_w", C.c_int32), ("box_h", C.c_int32), ("color_match", C.c_int32),
                ("reserved", C.c_int32), ("mask_offset", C.c_int64), ("rep_offset", C.c_int64)]


class PilPackedDesc(Record):
    c_name = "vrg_pil_packed_desc"
    _fields_ = [("src_offset", C.c_int64), ("dst_offset", C.c_int64), ("box_w", C.c_int32), ("box_h", C.c_int32), ("color_match", C.c_int32),
                ("reserved", C.c_int32), ("mask_offset", C.c_int64), ("rep_offset", C.c_int64)]


class GridDesc(Record):
    c_name = "vrg_grid_desc"
    _fields_ = [("src", C.c_void_p), ("xtab", C.c_void_p), ("ytab", C.c_void_p), ("overlay", C.c_void_p),
                ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32), ("mode", C.c_int32),
                ("frame", C.c_int32), ("dst_x", C.c_int32), ("dst_y", C.c_int32),
                ("new_w", C.c_int32), ("new_h", C.c_int32), ("x_off", C.c_int32), ("y_off", C.c_int32),
                ("band", C.c_int32), ("cps", C.c_int32), ("inv", C.c_float)]


class ThumbDesc(Record):
    c_name = "vrg_thumb_desc"
    _fields_ = [("xtab", C.c_void_p), ("ytab", C.c_void_p), ("offset", C.c_int64), ("which", C.c_int32),
                ("box_w", C.c_int32), ("box_h", C.c_int32), ("mode", C.c_int32), ("cps", C.c_int32), ("inv", C.c_float)]


class SheetPanel(Record):
    c_name = "vrg_sheet_panel"
    _fields_ = [("src", C.c_void_p), ("h_table", C.c_int64), ("v_table", C.c_int64), ("span_offset", C.c_int64), ("tmp_offset", C.c_int64),
                ("src_h", C.c_int32), ("src_w", C.c_int32), ("channels", C.c_int32), ("new_w", C.c_int32), ("new_h", C.c_int32),
                ("h_ksize", C.c_int32), ("v_ksize", C.c_int32), ("win_x", C.c_int32), ("win_y", C.c_int32), ("pic_w", C.c_int32),
                ("pic_h", C.c_int32), ("row0", C.c_int32), ("rows", C.c_int32), ("left", C.c_int32), ("top", C.c_int32), ("w", C.c_int32),
                ("h", C.c_int32), ("pic_x", C.c_int32), ("pic_y", C.c_int32), ("cps", C.c_int32), ("cell", C.c_uint8 * 4),
                ("reserved", C.c_int32)]


class MsrDesc(Record):
    c_name = "vrg_msr_desc"
    _fields_ = [("src", C.c_void_p), ("in_h", C.c_int32), ("in_w", C.c_int32), ("taps", C.c_int32), ("first_frame", C.c_int32),
                ("repeats", C.c_int32), ("fill", C.c_uint8 * 4)]


class ThumbEntry(Record):
    c_name = "vrg_thumb_entry"
    _fields_ = [("left_offset", C.c_int64), ("right_offset", C.c_int64), ("tmp_offset", C.c_int64), ("h_table", C.c_int64), ("v_table", C.c_int64),
                ("left_w", C.c_int32), ("left_h", C.c_int32), ("right_w", C.c_int32), ("right_h", C.c_int32), ("fx", C.c_int32), ("fy", C.c_int32),
                ("red_w", C.c_int32), ("red_h", C.c_int32), ("out_w", C.c_int32), ("out_h", C.c_int32), ("h_ksize", C.c_int32),
                ("v_ksize", C.c_int32), ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("cps", C.c_int32), ("reserved", C.c_int32)]


class RefbatchDesc(Record):
    c_name = "vrg_refbatch_desc"
    _fields_ = [("src_offset", C.c_int64), ("dst_offset", C.c_int64), ("src_h", C.c_int32), ("src_w", C.c_int32), ("src_c", C.c_int32),
                ("src_x0", C.c_int32), ("src_y0", C.c_int32), ("src_rw", C.c_int32), ("src_rh", C.c_int32), ("dst_h", C.c_int32),
                ("dst_w", C.c_int32), ("dst_c", C.c_int32), ("method", C.c_int32), ("frames", C.c_int32), ("first_tile", C.c_int32),
                ("reserved", C.c_int32)]


class AssembleDesc(Record):
    c_name = "vrg_assemble_desc"
    _fields_ = [("src", C.c_void_p * 16), ("overlay", C.c_void_p * 16), ("frames", C.c_int32 * 16), ("height", C.c_int32 * 16),
                ("width", C.c_int32 * 16), ("channels", C.c_int32 * 16), ("n_src", C.c_int32), ("bytes", C.c_int32)]


class AssembleEntry(Record):
    c_name = "vrg_assemble_entry"
    _fields_ = [("source", C.c_int32), ("frame", C.c_int32)]


class AnchorDesc(Record):
    c_name = "vrg_anchor_desc"
    _fields_ = [("src_offset", C.c_int64), ("h_table", C.c_int64), ("v_table", C.c_int64), ("in_w", C.c_int32), ("in_h", C.c_int32),
                ("h_ksize", C.c_int32), ("v_ksize", C.c_int32)]


class GuidanceDesc(Record):
    c_name = "vrg_guidance_desc"
    _fields_ = [("rows", C.c_int64), ("row_len", C.c_int64), ("batch", C.c_int64), ("mode", C.c_int32), ("has_negative", C.c_int32),
                ("has_perturbed", C.c_int32), ("cfg_star", C.c_int32), ("has_average", C.c_int32), ("has_momentum", C.c_int32),
                ("has_threshold", C.c_int32), ("has_rescale", C.c_int32), ("want_negative", C.c_int32), ("cfg_m1", C.c_float),
                ("eta", C.c_float), ("momentum", C.c_float), ("threshold", C.c_float), ("stg_scale", C.c_float), ("rescale", C.c_float),
                ("one_minus_rescale", C.c_float)]


class AreaCell(Record):          # one cell of the tables of vrg_area_taps / vrg_grid_taps / vrg_linear_taps
    c_name, c_header = "vrg::AreaCell", "comfyui-vrgamedevgirl_amd/csrc/vrg_area_math.hpp"
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("w_first", C.c_float), ("w_mid", C.c_float), ("w_last", C.c_float)]


class LzTap(Record):             # one record of the table of vrg_lanczos4_taps
    c_name, c_header = "vrg::LzTap", "comfyui-vrgamedevgirl_amd/csrc/vrg_lanczos_math.hpp"
    _fields_ = [("s", C.c_int32), ("w", C.c_int16 * 8)]


record_dtype = functools.lru_cache(maxsize=None)(np.dtype)      # record_dtype(Record): its structured dtype, the fields at their offsets


def upload_records(records, device, count=None, trailing=(), out=None):
    """The one way records reach a kernel: the first `count` (default all) of `records` -- a structured numpy array or a ctypes array of
    a Record -- then the arrays of `trailing` (side tables that ride in the same upload), as one flat uint8 tensor on `device`, or in the
    preallocated device tensor `out` of that size.  A synchronous copy from pageable memory: the host arrays are free once it returns."""
    if isinstance(records, np.ndarray):
        host = np.ascontiguousarray(records).reshape(-1)[:count].view(np.uint8)
    else:
        host = np.frombuffer(records, np.uint8, -1 if count is None else count * C.sizeof(records._type_))
    if trailing or not host.flags.writeable:        # (torch takes no read-only array)
        host = np.concatenate([host, *[np.ascontiguousarray(t).reshape(-1).view(np.uint8) for t in trailing]])
    host = torch.from_numpy(host)
    return host.to(device) if out is None else out.copy_(host)


GRID_COPY, GRID_FAST, GRID_FAST_2X2, GRID_GENERAL, GRID_LINEAR = 0, 1, 2, 3, 4
THUMB_SIDE = 320                # include/vrgdg_hip.h: VRG_THUMB_SIDE
THUMB_MAX_SIDE = 32767          # include/vrgdg_hip.h: VRG_THUMB_MAX_SIDE
PIL_STATS_WORDS = 12            # uint32 per frame (csrc/vrg_pil_math.hpp: PIL_STATS_WORDS)
PIL_MAX_LINE = 8192             # the longest mask row / column (csrc/vrg_pil_math.hpp: PIL_MAX_LINE)
SHEET_MAX_SIDE = 32767          # include/vrgdg_hip.h: VRG_SHEET_MAX_SIDE
SHEET_STAGE_VALUES = 16384      # include/vrgdg_hip.h: VRG_SHEET_STAGE_VALUES
PIL_FILTER_LANCZOS, PIL_FILTER_BICUBIC = 1, 3      # include/vrgdg_hip.h: VRG_PIL_FILTER_* (Pillow's own numbers)
FLF_CHUNK = 32                  # frames one workgroup writes (csrc/vrg_flf_math.hpp: FLF_CHUNK)
REFBATCH_TILE = 1024            # include/vrgdg_hip.h: VRG_REFBATCH_TILE
REFBATCH_BICUBIC, REFBATCH_BILINEAR, REFBATCH_AREA, REFBATCH_NEAREST_EXACT, REFBATCH_COPY, REFBATCH_BYTES = 0, 1, 2, 3, 4, 5
ASSEMBLE_MAX_SOURCES = 16       # include/vrgdg_hip.h: VRG_ASSEMBLE_MAX_SOURCES
ASSEMBLE_BAR = 60               # include/vrgdg_hip.h: VRG_ASSEMBLE_BAR (rows of the label bar)
ANCHOR_RGB, ANCHOR_BGR = 0, 1      # include/vrgdg_hip.h: VRG_ANCHOR_RGB / VRG_ANCHOR_BGR
GUIDANCE_SPAN = 4096            # include/vrgdg_hip.h: VRG_GUIDANCE_SPAN (elements of a row one workgroup takes)
GUIDANCE_CFG, GUIDANCE_APG = 0, 1      # include/vrgdg_hip.h: VRG_GUIDANCE_CFG / VRG_GUIDANCE_APG
FACEFIX_STATS_WORDS = 12        # uint64 per frame (csrc/vrg_facefix_math.hpp: FF_STATS_WORDS)
FACEFIX_PACKED_TILE = 256       # include/vrgdg_hip.h: VRG_FF_PACKED_TILE (box pixels of one workgroup)
PIL_PACKED_TILE = 256           # include/vrgdg_hip.h: VRG_PIL_PACKED_TILE (box pixels of one workgroup of the packed far-face paste)

_F3 = C.c_float * 3
_P = C.c_void_p
_SIGNATURES = {
    "vrg_abi_version": (C.c_int, []),
    "vrg_error_string": (C.c_char_p, [C.c_int]),
    "vrg_device_info": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "vrg_event_create": (C.c_int, [C.POINTER(_P)]),
    "vrg_event_record": (C.c_int, [_P, _P]),
    "vrg_event_elapsed_ms": (C.c_int, [_P, _P, C.POINTER(C.c_float)]),
    "vrg_event_destroy": (C.c_int, [_P]),
    "vrg_sharpen_grain_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_float,
                                        C.POINTER(NoiseDesc), _P]),
    "vrg_sharpen_grain_u8": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_float,
                                       C.POINTER(NoiseDesc), _P]),
    "vrg_grain_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float,
                                C.POINTER(NoiseDesc), _P]),
    "vrg_grain_split_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float,
                                      C.POINTER(NoiseSplit), _P]),
    "vrg_fused_chain_split_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(ChainDesc), C.POINTER(NoiseSplit), _P]),
    "vrg_fused_chain_split_u8": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(ChainDesc), C.POINTER(NoiseSplit), _P]),
    "vrg_chain_stats_lab_split_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(ChainDesc), C.POINTER(NoiseSplit), _P, _P, _P]),
    "vrg_grain_injected_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, _P]),
    "vrg_lut_cells_floats": (C.c_int64, [C.c_int32]),
    "vrg_lut_prepare_f32": (C.c_int, [_P, C.c_int32, _P, _P]),
    "vrg_lut3d_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _F3, _F3, C.c_int32, C.c_float,
                                C.c_float, _P]),
    "vrg_stencil3x3_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_float, _P]),
    "vrg_adjust_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(AdjustDesc), _P]),
    "vrg_adjust_u8": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(AdjustDesc), _P]),
    "vrg_u8_channel_sums": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    "vrg_u8bgr_to_f32rgb": (C.c_int, [_P, _P, C.c_int64, _P]),
    "vrg_f32rgb_to_u8bgr": (C.c_int, [_P, _P, C.c_int64, _P]),
    "vrg_lut3d_tetra_u8": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int32, _F3, _F3, _P, _P]),
    "vrg_fused_chain_u8": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(ChainDesc), _P]),
    "vrg_lab_stats_scratch_bytes": (C.c_int64, [C.c_int64]),
    "vrg_lab_stats_f32": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P]),
    "vrg_lab_stats_finalize": (C.c_int, [_P, _P, C.c_int64, _P]),
    "vrg_lab_stats_torch_f32": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, C.c_float, _P]),
    "vrg_lab_stats_torch_scratch_bytes": (C.c_int64, [C.c_int64]),
    "vrg_host_copy": (C.c_int, [_P, _P, C.c_int64, C.c_int32]),
    "vrg_lab_stats_torch_ws_f32": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, C.c_float, _P, C.c_int64, _P]),
    "vrg_lab_stats_torch_lat_f32": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, C.c_float, _P, C.c_int64, _P]),
    "vrg_stats_allreduce_scratch_bytes": (C.c_int64, [C.c_int64]),
    "vrg_stats_allreduce": (C.c_int, [_P, C.c_int64, _P, _P, _P]),
    "vrg_colormatch_apply_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_float,
                                           C.c_float, C.c_int32, _P]),
    "vrg_fused_chain_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(ChainDesc), _P]),
    "vrg_chain_stats_f32": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(ChainDesc), _P, _P, _P]),
    "vrg_chain_stats_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(ChainDesc)]),
    "vrg_chain_stats_lab_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(ChainDesc), _P, _P, _P]),
    "vrg_noise_f32": (C.c_int, [_P, C.c_int64, C.c_int64, C.POINTER(NoiseDesc), _P]),
    "vrg_selfcheck_pow_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P]),
    "vrg_resize_f32": (C.c_int, [_P, _P, C.c_int64] + [C.c_int32] * 13 + [C.c_int32, _P]),
    "vrg_restore_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64] + [C.c_int32] * 13 + [C.c_int32, C.c_int32, C.c_float, C.c_float, _P]),
    "vrg_prepare_frames_f32": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64] + [C.c_int32] * 10 + [C.c_int32, _P, _P, _P]),
    "vrg_composite_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "vrg_composite_stats_f32": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int64] + [C.c_int64] * 4 + [C.c_int32] * 10 + [_P, _P, _P]),
    "vrg_composite_apply_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, _P] + [C.c_int64] * 4 + [C.c_int32] * 10 + [_P]),
    "vrg_crop_resize_f32": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "vrg_lanczos4_taps": (C.c_int, [C.c_int32] * 4 + [_P]),
    "vrg_lanczos4_u8": (C.c_int, [_P, _P, C.c_int64] + [C.c_int32] * 4 + [_P, _P]),
    "vrg_upscale_sharpen_grain_u8": (C.c_int, [_P, _P, C.c_int64] + [C.c_int32] * 4 + [_P, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_float,
                                               C.POINTER(NoiseDesc), _P]),
    "vrg_warp_phase_table": (C.c_int, [_P]),
    "vrg_warp_record": (C.c_int, [_P] + [C.c_int32] * 4 + [C.c_int64, _P]),
    "vrg_face_bytes_u8": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64] + [C.c_int64] * 3 + [C.c_int32] * 6 + [_P]),
    "vrg_warp_affine_u8": (C.c_int, [_P, C.c_int64, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "vrg_composite_warp_apply_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P] + [C.c_int64] * 4 + [C.c_int32] * 10 + [_P]),
    "vrg_area_taps": (C.c_int, [C.c_int32, C.c_int32, _P]),
    "vrg_cut_thumbs_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "vrg_cut_hist_u8": (C.c_int, [_P, _P, C.c_int64, _P]),
    "vrg_cut_pair_sums": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "vrg_ff_ellipse_spans": (C.c_int, [C.c_int32, C.c_int32, _P]),
    "vrg_ff_gauss_coeffs": (C.c_int, [C.c_int32, _P]),
    "vrg_lanczos4_boxes_u8": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P]),
    "vrg_ff_masks_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P, C.c_int64, _P]),
    "vrg_ff_resize_stats_u8": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int64] + [C.c_int32] * 4 +
                               [C.c_int64, C.c_float, _P]),
    "vrg_ff_composite_u8": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "vrg_ff_packed_check": (C.c_int, [_P, C.c_int64, _P] + [C.c_int64] * 6 + [C.c_int32, C.c_int32]),
    "vrg_lanczos4_packed_u8": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P, C.c_int64, _P]),
    "vrg_ff_packed_resize_stats_u8": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P, _P, C.c_int64, C.c_int64,
                                                _P, C.c_int64, _P, C.c_int64, _P, C.c_float, _P]),
    "vrg_ff_packed_composite_u8": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, _P]),
    "vrg_pil_lanczos_ksize": (C.c_int32, [C.c_int32, C.c_int32]),
    "vrg_pil_lanczos_table": (C.c_int, [C.c_int32, C.c_int32, _P, _P]),
    "vrg_pil_box_parameters": (C.c_int, [C.c_float, _P]),
    "vrg_pil_resize_u8": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int64, _P]),
    "vrg_pil_mask_u8": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P]),
    "vrg_np_masked_means_f32": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_float, _P]),
    "vrg_pil_paste_u8": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "vrg_pil_packed_check": (C.c_int, [_P, C.c_int64, _P] + [C.c_int64] * 4),
    "vrg_np_packed_masked_means_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, C.c_float, _P]),
    "vrg_pil_packed_paste_u8": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, C.c_int64, _P, _P, C.c_int64, _P]),
    "vrg_linear_taps": (C.c_int, [C.c_int32, C.c_int32, _P, _P]),
    "vrg_detect_check": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64]),
    "vrg_detect_blobs_f32": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    "vrg_detect_blobs_u8": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    "vrg_grid_plan": (C.c_int, [C.c_int32] * 5 + [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "vrg_grid_taps": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P]),
    "vrg_grid_check": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int64] + [C.c_int32] * 4),
    "vrg_grid_tiles_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int64] + [C.c_int32] * 4 + [_P]),
    "vrg_grid_tiles_u8": (C.c_int, [_P, C.c_int64, _P, C.c_int64] + [C.c_int32] * 4 + [_P]),
    "vrg_warp_linear_u8": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    "vrg_face_thumbs_check": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int]),
    "vrg_face_thumbs_u8": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    "vrg_sheet_fit": (C.c_int, [C.c_int32] * 5 + [_P]),
    "vrg_sheet_plan": (C.c_int, [_P, C.c_int64, _P, C.c_int64]),
    "vrg_sheet_check": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int64, C.c_int64]),
    "vrg_sheet_rows_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "vrg_sheet_rows_u8": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "vrg_sheet_compose_f32": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, C.c_int32, C.c_int32,
                                        C.c_uint32, _P]),
    "vrg_sheet_compose_u8": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, C.c_int32, C.c_int32,
                                       C.c_uint32, _P]),
    "vrg_pil_filter_ksize": (C.c_int32, [C.c_int32, C.c_float, C.c_float, C.c_int32]),
    "vrg_pil_filter_table": (C.c_int, [C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, _P, _P]),
    "vrg_pil_reduce_host": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "vrg_thumb_plan": (C.c_int, [_P, C.c_int64, _P, C.c_int32, C.c_double, C.c_int32, _P]),
    "vrg_thumb_plan_reduce": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P]),
    "vrg_thumb_check": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int64, C.c_int64] + [C.c_int32] * 5),
    "vrg_thumb_rows_u8": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "vrg_thumb_compose_u8": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P] + [C.c_int32] * 5 + [C.c_uint32, _P]),
    "vrg_msr_check": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "vrg_msr_frames_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "vrg_flf_check": (C.c_int, [C.c_int64] + [C.c_int32] * 9),
    "vrg_flf_guide_f32": (C.c_int, [_P, _P, _P, _P, C.c_int64] + [C.c_int32] * 9 + [_P]),
    "vrg_refbatch_check": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "vrg_refbatch_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int64, _P, C.c_int64, _P]),
    "vrg_refbatch_quantise_u8": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int64, _P, C.c_int64, _P]),
    "vrg_assemble_check": (C.c_int, [C.POINTER(AssembleDesc), _P, C.c_int64, _P, _P, C.c_int32]),
    "vrg_assemble_f32": (C.c_int, [C.POINTER(AssembleDesc), _P, C.c_int64, _P, _P]),
    "vrg_assemble_labelled_u8": (C.c_int, [C.POINTER(AssembleDesc), _P, C.c_int64, _P, _P, _P]),
    "vrg_anchor_check": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "vrg_anchor_frames_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P]),
    "vrg_anchor_store_u8": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "vrg_guidance_check": (C.c_int, [C.POINTER(GuidanceDesc)]),
    "vrg_guidance_scratch_bytes": (C.c_int64, [C.POINTER(GuidanceDesc)]),
    "vrg_guidance_sums_f32": (C.c_int, [_P, _P, C.POINTER(GuidanceDesc), _P, C.c_int64, _P]),
    "vrg_guidance_rows_f32": (C.c_int, [_P, _P, _P, _P, C.POINTER(GuidanceDesc), _P, C.c_int64, _P]),
    "vrg_guidance_combine_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, C.POINTER(GuidanceDesc), _P, C.c_int64, _P]),
    "vrg_guidance_rescale_f32": (C.c_int, [_P, C.POINTER(GuidanceDesc), _P, C.c_int64, _P]),
    "vrg_rgb24_frames_u8": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P]),
}

# include/vrgdg_hip_debug.h: self-tests and probes -- for the test suite and the measurement tools, not part of the drop-in boundary
_DEBUG_SIGNATURES = {
    "vrg_selftest_divconst": (C.c_int, [_P, _P]),
    "vrg_selftest_bm_radius": (C.c_int, [_P, _P]),
    "vrg_selftest_lanes": (C.c_int, [_P, _P]),
    "vrg_selftest_welford_division": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "vrg_debug_cm_math": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_float, _P]),
    "vrg_debug_torch_reduce_config": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int32)]),
    "vrg_debug_lut_fetch": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P]),
    "vrg_debug_copy_f32": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P]),
    "vrg_debug_valu_rate": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P]),
}

EXPORTED_SYMBOLS = tuple(sorted(_SIGNATURES))
DEBUG_SYMBOLS = tuple(sorted(_DEBUG_SIGNATURES))

_lib = None
_host_lib = None
_lock = threading.Lock()


class Library:
    """Handle of the loaded product library.  Attribute access resolves the names of include/vrgdg_hip.h in libvrgdg_hip.so; a name of
    include/vrgdg_hip_debug.h -- and only such a name -- opens libvrgdg_hip_debug.so (once) and resolves there, so that tests and tools keep
    writing `lib().vrg_debug_...` while no node ever touches the debug library."""

    def __init__(self, cdll: C.CDLL, path: str, debug_path: str = DEBUG_LIB_PATH):
        self.__dict__["_cdll"] = cdll
        self.__dict__["_path"] = path
        self.__dict__["_debug_path"] = debug_path
        self.__dict__["_debug"] = None

    def debug(self) -> C.CDLL:
        if self._debug is None:
            with _lock:
                if self._debug is None:
                    if not os.path.exists(self._debug_path):
                        raise RuntimeError(f"libvrgdg_hip_debug.so not found at {self._debug_path} (self-tests / probes: build it with "
                                           f"`python {os.path.join(PKG_DIR, 'build_ext.py')}`)")
                    dbg = C.CDLL(self._debug_path)
                    for name, (res, args) in _DEBUG_SIGNATURES.items():
                        fn = getattr(dbg, name)   # AttributeError if the debug ABI drifted
                        fn.restype = res
                        fn.argtypes = args
                    self.__dict__["_debug"] = dbg
        return self._debug

    def __getattr__(self, name):
        if name in _DEBUG_SIGNATURES:
            return getattr(self.debug(), name)
        return getattr(self._cdll, name)


def load_library(path: str = LIB_PATH) -> Library:
    """dlopen the library and attach the prototypes (no device needed)."""
    import torch  # noqa: F401  -- FIRST: the HIP runtime must be the one torch loaded (same soname, shared streams/pointers)
    if not os.path.exists(path):
        raise RuntimeError(
            f"libvrgdg_hip.so not found at {path}: build it with `python {os.path.join(PKG_DIR, 'build_ext.py')}` "
            "(hipcc, gfx950). This package has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the ABI drifted
        fn.restype = res
        fn.argtypes = args
    if lib.vrg_abi_version() != ABI_VERSION:
        raise RuntimeError("libvrgdg_hip.so ABI version mismatch")
    return Library(lib, path)


def lib() -> Library:
    """The loaded library, for launching kernels: also requires a visible HIP device."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                import torch
                if not torch.cuda.is_available():
                    raise RuntimeError("comfyui-vrgamedevgirl_amd needs an AMD GPU (MI355X / gfx950) visible to "
                                       "PyTorch-ROCm; there is no CPU fallback")
                _lib = load_library()
    return _lib


def host_library() -> Library:
    """The loaded library, for its HOST functions (tables, plans, checks): no device needed.  One handle per process."""
    global _host_lib
    if _host_lib is None:
        with _lock:
            if _host_lib is None:
                _host_lib = load_library()
    return _host_lib


def check(status: int, what: str):
    if status != VRG_OK:
        msg = lib().vrg_error_string(status).decode()
        if status == 1:
            raise ValueError(f"{what}: {msg}")
        raise RuntimeError(f"{what}: {msg}")


def ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def current_stream() -> C.c_void_p:
    """torch's current stream of the CURRENT device.  ops.* make the tensors' device current first (ops._on_device), so
    that the stream, the kernels' hipGetDevice() and the pointers always belong to the same GPU."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)

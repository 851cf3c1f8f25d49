"""The operators of ops.py that write a caller's tensor (`out`, `mask_out`, `workspace`, `lab_workspace`, `clean_out`) and the one rule
they share (ops._disjoint, vrg_ranges_overlap in csrc/vrg_common.hpp): no written operand may share a byte with an operand that is
read, or with another written one.

ROWS is the one table: per operator a smallest valid call (`build`), the operands it writes and the resident operands it reads, by the
names the refusal uses.  ARRANGEMENTS places a written range against another range; offsets are counted in elements of the written
operand's dtype.  tests/test_overlap_host.py holds the table complete (every public function of ops with a write operand has a row) and
the helpers to the arrangements without a GPU; tests/test_gpu_overlap.py runs every row on the GPU."""
import functools
import os
from collections import namedtuple

import numpy as np
import torch

WRITE_PARAMETERS = ("out", "mask_out", "workspace", "lab_workspace", "clean_out")
GUARD = 256                                # sentinel bytes before the first and after the last operand of a shared allocation

#: name -> (refused?, what it is)
ARRANGEMENTS = {
    "a": (True, "same start"),
    "b": (True, "the write starts one element after the read's start"),
    "c": (True, "the write's last element is the read's first"),
    "d": (True, "the write lies strictly inside a larger read"),
    "e": (True, "the read lies strictly inside a larger write"),
    "f": (False, "the write ends exactly where the read starts"),
    "g": (False, "the write starts exactly where the read ends"),
}
REFUSED = tuple(k for k, (refused, _) in ARRANGEMENTS.items() if refused)
ACCEPTED = tuple(k for k, (refused, _) in ARRANGEMENTS.items() if not refused)


def placement(arrangement, w_bytes, w_item, r_bytes):
    """The byte offset of the written range's start from the read range's start in `arrangement`, or None where the two sizes do not
    allow it (a range cannot lie strictly inside a smaller one; a written element must start on its own grid)."""
    if arrangement == "a":
        return 0
    if arrangement == "b":
        return w_item if r_bytes > w_item else None
    if arrangement == "c":
        return -(w_bytes - w_item)
    if arrangement == "d":
        return w_item if w_bytes + 2 * w_item <= r_bytes else None
    if arrangement == "e":
        return -w_item if r_bytes + 2 * w_item <= w_bytes else None
    if arrangement == "f":
        return -w_bytes
    if arrangement == "g":
        return r_bytes if r_bytes % w_item == 0 else None
    raise KeyError(arrangement)


def overlap_truth(offset, w_bytes, r_bytes):
    """the plain interval test on Python integers: the written range at `offset` from the read range's start"""
    return w_bytes > 0 and r_bytes > 0 and offset < r_bytes and 0 < offset + w_bytes


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
#: reads: name -> CPU tensor (the values of a resident input); writes: name -> (shape, dtype); run(ops, t) -> the tensors the call wrote,
#: where t maps every name to its device tensor
Call = namedtuple("Call", "reads writes run")
#: writes / reads: the operand names as the refusal gives them, in the order of Call.writes / Call.reads
Row = namedtuple("Row", "op label writes reads build")


def row_id(row):
    return row.op + (f"-{row.label}" if row.label else "")


def _rand(shape, seed, lo=-0.05, hi=1.05):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _bytes(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def _lut(device):
    from comfyui_vrgamedevgirl_amd import ops
    g = torch.Generator().manual_seed(31)
    data = {"lut": torch.rand(5, 5, 5, 3, generator=g), "domain_min": torch.zeros(3), "domain_max": torch.ones(3)}
    return ops.upload_lut(data, device)


def _device(t):
    return next(iter(t.values())).device


F32, U8 = torch.float32, torch.uint8


def _like(x, dtype=None):
    return (tuple(x.shape), dtype or x.dtype)


def _pointwise(shape, seed, run):
    x = _rand(shape, seed)
    return Call({"images": x}, {"out": _like(x)}, run)


def _film_grain():
    def run(ops, t):
        torch.manual_seed(77)
        return [ops.film_grain(t["images"], 0.1, 0.5, chunk_frames=1, out=t["out"])]
    return _pointwise((2, 5, 7, 3), 1, run)


def _lut3d():
    x = _rand((2, 5, 7, 3), 2)
    return Call({"image": x}, {"out": _like(x)}, lambda ops, t: [ops.lut3d(t["image"], _lut(_device(t)), 6.0, out=t["out"])])


def _stencil(shape, op, strength, zero):
    return lambda: _pointwise(shape, 3, lambda ops, t: [ops.stencil3x3(t["images"], op, strength, zero, out=t["out"])])


RESIZE_METHOD = "Bicubic (recommended)"


def _resize(out_h, out_w, through_frames):
    def build():
        from comfyui_vrgamedevgirl_amd import ops
        x = _rand((2, 9, 11, 3), 4)

        def run(ops, t):
            if through_frames:
                return [ops.resize_frames(t["images"], out_w, out_h, ops.FIT_STRETCH, RESIZE_METHOD, out=t["out"])]
            return [ops.resize_geometry_frames(t["images"], ops.resize_geometry(9, 11, out_w, out_h, ops.FIT_STRETCH), RESIZE_METHOD, out=t["out"])]
        g = ops.resize_geometry(9, 11, out_w, out_h, ops.FIT_STRETCH)
        return Call({"images": x}, {"out": ((2, g.out_h, g.out_w, 3), F32)}, run)
    return build


def _restore():
    work, originals = _rand((2, 5, 7, 3), 5), _rand((3, 9, 11, 4), 6, -0.2, 1.2)
    return Call({"work": work, "originals": originals}, {"out": _like(originals)},
                lambda ops, t: [ops.restore_frames(t["work"], t["originals"], 11, 9, ops.FIT_STRETCH, RESIZE_METHOD, 0.6, out=t["out"])])


COMPOSITE_ENTRIES = [{"original": 0, "crop": 1, "mask": 0, "box": (2, 3, 10, 9)}, {"original": 1, "crop": 0, "mask": 1, "box": (0, 0, 14, 12)},
                     {"original": 1, "crop": 1, "box": None}]


def _composite():
    originals, crops, mask = _rand((2, 12, 14, 3), 7), _rand((2, 6, 5, 3), 8), _rand((2, 6, 5), 9, 0.0, 1.0)

    def run(ops, t):
        return list(ops.composite_frames(t["originals"], t["crops"], COMPOSITE_ENTRIES, ops.CompositeRule("ellipse", feather=2, inset=1), 0.5,
                                         user_mask=t["user_mask"], out=t["out"], mask_out=t["mask_out"]))
    return Call({"originals": originals, "crops": crops, "user_mask": mask}, {"out": ((3, 12, 14, 3), F32), "mask_out": ((3, 12, 14), F32)}, run)


def _aligned_composite():
    originals, crops = _rand((2, 30, 40, 3), 10), _rand((2, 16, 16, 3), 11)
    entries = [{"original": i, "crop": i, "box": (4 + i, 3, 30 + i, 27)} for i in range(2)]
    ident = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32)

    def run(ops, t):
        return list(ops.aligned_composite_frames(t["originals"], t["crops"], entries, 3, [ident, None], out=t["out"], mask_out=t["mask_out"]))
    return Call({"originals": originals, "crops": crops}, {"out": ((2, 30, 40, 3), F32), "mask_out": ((2, 30, 40), F32)}, run)


def _crop_resize():
    source = _rand((2, 20, 24, 3), 12)
    records = [(0, 24 * 3, 3, 10, 8), ((20 * 24 + 5 * 24 + 3) * 3, 24 * 3, 3, 20, 15)]
    return Call({"source": source}, {"out": ((2, 6, 7, 3), F32)}, lambda ops, t: [ops.crop_resize(t["source"], records, (6, 7), out=t["out"])])


def _crop_frames():
    from comfyui_vrgamedevgirl_amd import ops
    frames = _rand((3, 20, 24, 3), 13)
    plan = ops.crop_sequence_plan([{"box": (2, 3, 14, 12)}, {"box": None}, {"box": (5, 7, 20, 19)}], 3, 20, 24)
    return Call({"source": frames}, {"out": ((plan.count, 6, 7, 3), F32)}, lambda ops, t: [ops.crop_frames(t["source"], plan, (6, 7), out=t["out"])])


def _cut_thumbnails():
    frames = _rand((2, 70, 66, 3), 14)
    return Call({"frames": frames}, {"out": ((2, 64, 64, 3), U8)}, lambda ops, t: [ops.cut_thumbnails(t["frames"], out=t["out"])])


def _video_grid(byte_sources):
    def build():
        from comfyui_vrgamedevgirl_amd import ops
        shapes = [(2, 9, 11, 3), (1, 7, 5, 3)]
        batches = [_bytes(s, 15 + i) if byte_sources else _rand(s, 15 + i, 0.0, 1.0) for i, s in enumerate(shapes)]
        plan = ops.grid_plan([s[1:] for s in shapes], 32, 24, 2, 0)

        def run(ops, t):
            given = [t["batch 0"], t["batch 1"]]
            if byte_sources:
                return [ops.video_grid_bytes(given, [[0, 1], [0, 0]], 32, 24, 2, out=t["out"])]
            return [ops.video_grid(given, 32, 24, 2, out=t["out"])]
        return Call({"batch 0": batches[0], "batch 1": batches[1]}, {"out": ((2, plan.grid_h, plan.grid_w, 3), F32)}, run)
    return build


ADJUST_BOTH = {"clarity": 45, "sharpen": 30, "vignette": 20, "contrast": 10, "highlights": -35}      # the 9-box (or the small box), the 3-box, the ring


def adjust_terms(ops):
    from comfyui_vrgamedevgirl_amd import VRGDG_LUTVideoTools as LVT
    return ops.adjust_terms(LVT._normalize_adjust_settings(ADJUST_BOTH), device_math=True)


def _adjust(shape, u8=False):
    def build():
        x = _bytes(shape, 17) if u8 else _rand(shape, 17, -0.1, 1.1)
        return Call({"images": x}, {"out": _like(x), "workspace": (shape, F32)},
                    lambda ops, t: [ops.adjust(t["images"], adjust_terms(ops), out=t["out"], workspace=t["workspace"])])
    return build


def _lab_stats_device():
    lab = _rand((3, 9, 11, 3), 18, -20.0, 90.0)
    return Call({"lab": lab}, {"out": ((3, 3, 2), F32)}, lambda ops, t: [ops.lab_stats_device(t["lab"], out=t["out"])])


CHAIN_SHARPEN = ("unsharp", 0.5, False)
CHAIN_GRAIN = (0.04, 0.5, 1)


def chain_spec(ops, device, colormatch, variant):
    if colormatch:
        ref_ms = torch.tensor([[[50.0, 20.0], [5.0, 10.0], [-3.0, 12.0]]], dtype=torch.float32, device=device)
        return ops.ChainSpec(lut=(_lut(device), 6.0), colormatch=(ref_ms, 0.8), sharpen=CHAIN_SHARPEN, variant=variant)
    return ops.ChainSpec(grain=CHAIN_GRAIN, lut=(_lut(device), 6.0), sharpen=CHAIN_SHARPEN, variant=variant)


def _fused_chain(shape, colormatch, variant, u8=False):
    def build():
        x = _bytes(shape, 19) if u8 else _rand(shape, 19)

        def run(ops, t):
            torch.manual_seed(77)
            return [ops.fused_chain(t["images"], chain_spec(ops, _device(t), colormatch, variant), out=t["out"],
                                    lab_workspace=t.get("lab_workspace"))]
        writes = {"out": _like(x)}
        if colormatch:
            writes["lab_workspace"] = (shape, F32)
        return Call({"images": x}, writes, run)
    return build


def _fused_stages():
    x = _rand((2, 9, 11, 3), 20)
    return Call({"images": x}, {"out": _like(x)},
                lambda ops, t: [ops.fused_stages(t["images"], 0, {"sharpen": {"op": "unsharp", "strength": 0.5, "zero": False},
                                                                  "lut": {"lut": _lut(_device(t)), "strength": 6.0}}, out=t["out"])])


def _color_match(cache_lab):
    def build():
        x = _rand((2, 9, 11, 3), 21)

        def run(ops, t):
            ref_ms = torch.tensor([[[50.0, 20.0], [5.0, 10.0], [-3.0, 12.0]]], dtype=torch.float32, device=_device(t))
            return [ops.color_match(t["images"], None, 0.8, ref_ms=ref_ms, cache_lab=cache_lab, cm_stats=None if cache_lab else "fp64", out=t["out"])]
        return Call({"images": x}, {"out": _like(x)}, run)
    return build


def _flf():
    first, last = _rand((1, 9, 11, 3), 22), _rand((1, 12, 10, 3), 23)
    return Call({"first": first, "last": last}, {"out": ((4, 9, 11, 3), F32)},
                lambda ops, t: [ops.flf_guide_frames(t["first"], t["last"], 4, out=t["out"])])


def _scale_reference():
    from comfyui_vrgamedevgirl_amd import ops
    pictures = [_rand((1, 9, 11, 3), 24), _rand((2, 6, 5, 4), 25)]
    sizes = [ops.total_pixels_size(int(p.shape[1]), int(p.shape[2]), 0.0002, 1) for p in pictures]
    total = sum(int(p.shape[0]) * oh * ow * int(p.shape[3]) for p, (oh, ow) in zip(pictures, sizes))

    def run(ops, t):
        ops.scale_reference_images([t["image 0"], t["image 1"]], "bilinear", 0.0002, 1, out=t["out"])
        return [t["out"]]
    return Call({"image 0": pictures[0], "image 1": pictures[1]}, {"out": ((total,), F32)}, run)


def _batch_reference():
    pictures = [_rand((1, 9, 11, 3), 26), _rand((2, 6, 5, 3), 27)]
    return Call({"image 0": pictures[0], "image 1": pictures[1]}, {"out": ((3, 9, 11, 3), F32)},
                lambda ops, t: [ops.batch_reference_images([t["image 0"], t["image 1"]], "bilinear", out=t["out"])])


ASSEMBLE_PLAN = [(0, 1), (1, 0), (1, 0), (0, 2)]


def _assemble(labelled):
    def build():
        clips = [_rand((3, 8, 12, 3), 28, 0.0, 1.0), _rand((1, 8, 12, 3), 29, 0.0, 1.0)]

        def run(ops, t):
            given = [t["clip 0"], t["clip 1"]]
            if labelled:
                return list(ops.assemble_labelled_bytes(given, ASSEMBLE_PLAN, clean_out=t["clean_out"]))
            return [ops.assemble_frames(given, ASSEMBLE_PLAN, out=t["out"])]
        return Call({"clip 0": clips[0], "clip 1": clips[1]}, {"clean_out" if labelled else "out": ((4, 8, 12, 3), F32)}, run)
    return build


def _anchor_frames():
    pictures = [_bytes((9, 11, 3), 30), _bytes((6, 5, 3), 31)]
    return Call({"picture 0": pictures[0], "picture 1": pictures[1]}, {"out": ((2, 9, 11, 3), F32)},
                lambda ops, t: [ops.anchor_frames([t["picture 0"], t["picture 1"]], out=t["out"])])


def _anchor_store():
    images = _rand((2, 9, 11, 4), 32, -0.2, 1.2)
    return Call({"images": images}, {"out": ((2, 9, 11, 3), U8)}, lambda ops, t: [ops.anchor_store_bytes(t["images"], bgr=True, out=t["out"])])


def _row(op, label, build, reads, writes=("out",)):
    return Row(op, label, tuple(writes), tuple(reads), build)


ROWS = (
    _row("film_grain", "", _film_grain, ["images"]),
    _row("lut3d", "", _lut3d, ["image"]),
    # stencil_support.SWEEP: the flat march with both overlaps, the LDS tile kernel, the generic kernel
    _row("stencil3x3", "flat", _stencil((2, 37, 88, 3), "unsharp", 0.5, False), ["images"]),
    _row("stencil3x3", "tile", _stencil((2, 37, 87, 3), "sobel", 0.8, True), ["images"]),
    _row("stencil3x3", "generic", _stencil((2, 9, 13, 2), "laplacian", 0.8, False), ["images"]),
    _row("resize_geometry_frames", "shrink", _resize(5, 7, False), ["images"]),
    _row("resize_geometry_frames", "enlarge", _resize(13, 16, False), ["images"]),
    _row("resize_frames", "shrink", _resize(5, 7, True), ["images"]),
    _row("restore_frames", "", _restore, ["work", "originals"]),
    _row("composite_frames", "", _composite, ["originals", "crops", "user_mask"], ["out", "mask_out"]),
    _row("aligned_composite_frames", "", _aligned_composite, ["originals", "crops"], ["out", "mask_out"]),
    _row("crop_resize", "", _crop_resize, ["source"]),
    _row("crop_frames", "", _crop_frames, ["source"]),
    _row("cut_thumbnails", "", _cut_thumbnails, ["frames"]),
    _row("video_grid", "", _video_grid(False), ["batch 0", "batch 1"]),
    _row("video_grid_bytes", "", _video_grid(True), ["batch 0", "batch 1"]),
    _row("adjust", "boxes", _adjust((2, 24, 40, 3)), ["images"], ["out", "workspace"]),
    _row("adjust", "small-box", _adjust((2, 6, 7, 3)), ["images"], ["out", "workspace"]),
    _row("adjust", "bytes", _adjust((2, 24, 40, 3), u8=True), ["images"], ["out", "workspace"]),
    _row("lab_stats_device", "", _lab_stats_device, ["lab"]),
    _row("color_match", "cached", _color_match(True), ["images"]),
    _row("color_match", "two-pass", _color_match(False), ["images"]),
    _row("fused_chain", "tile", _fused_chain((2, 33, 62, 3), False, 1), ["images"]),
    _row("fused_chain", "march", _fused_chain((2, 37, 88, 3), False, 2), ["images"]),
    _row("fused_chain", "bytes", _fused_chain((2, 33, 62, 3), False, 1, u8=True), ["images"]),
    _row("fused_chain", "colormatch-tile", _fused_chain((2, 33, 62, 3), True, 1), ["images"], ["out", "lab_workspace"]),
    _row("fused_chain", "colormatch-march", _fused_chain((2, 73, 344, 3), True, 0), ["images"], ["out", "lab_workspace"]),
    _row("fused_stages", "", _fused_stages, ["images"]),
    _row("flf_guide_frames", "", _flf, ["first", "last"]),
    _row("scale_reference_images", "", _scale_reference, ["image 0", "image 1"]),
    _row("batch_reference_images", "", _batch_reference, ["image 0", "image 1"]),
    _row("assemble_frames", "", _assemble(False), ["clip 0", "clip 1"]),
    _row("assemble_labelled_bytes", "", _assemble(True), ["clip 0", "clip 1"], ["clean_out"]),
    _row("anchor_frames", "", _anchor_frames, ["picture 0", "picture 1"]),
    _row("anchor_store_bytes", "", _anchor_store, ["images"]),
)
#: the operator's name in its refusal where that is not the function's
MESSAGE_NAME = {"video_grid": "video grid", "video_grid_bytes": "video grid", "flf_guide_frames": "first/last guide", "crop_frames": "crop_resize",
                "resize_frames": "resize_geometry_frames", "color_match": "fused_chain|color_match", "fused_stages": "fused_chain"}


@functools.lru_cache(maxsize=None)
def call_of(index):
    """the call of ROWS[index], built once; its tensors are shared: do not write to them"""
    return ROWS[index].build()


def pairs(row):
    """every (written operand, other operand) of a row that the rule keeps apart: each write against each read and each later write"""
    out = []
    for i, w in enumerate(row.writes):
        out += [(w, r) for r in row.reads] + [(w, v) for v in row.writes[i + 1:]]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# operands carved from one allocation
# ---------------------------------------------------------------------------------------------------------------------------------
def nbytes_of(shape, dtype):
    return int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()


def carve(buffer, offset, shape, dtype):
    """`shape` elements of `dtype` at byte `offset` of the flat uint8 `buffer`: a contiguous view of its memory"""
    n = nbytes_of(shape, dtype)
    return buffer[offset:offset + n].view(dtype).view(shape)


def sentinel(nbytes, device):
    """bytes no kernel leaves behind by accident"""
    g = torch.Generator().manual_seed(nbytes)
    return torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8).to(device)

"""Shared by tools/make_golden_msr.py, tests/test_msr_host.py and tests/test_gpu_msr.py: the seeded input pictures, the node cases of
tests/golden/msr_reference.npz, a stand-in for ComfyUI's ``folder_paths`` over a directory of those pictures, and the expectation of
the launch -- ``restated(...).astype(np.float32) / np.float32(255)`` of tests/lanczos_support.py, every repeat of it."""
import json
import os
import sys
import types

import numpy as np

from conftest import GOLDEN
from lanczos_support import restated

FIXTURE = os.path.join(GOLDEN, "msr_reference.npz")
NONE_IMAGE = "(none)"

#: name -> (width, height, seed, EXIF orientation or None) of the stored picture
PICTURES = {
    "a.png": (37, 53, 11, None),
    "b.png": (197, 131, 12, None),
    "c.png": (120, 40, 13, None),
    "d.png": (7, 5, 14, None),
    "bg.png": (120, 90, 15, None),
    "same_64x96.png": (64, 96, 16, None),
    "turned.png": (90, 50, 17, 6),               # shown 50 wide, 90 high
}

_B = {"subject_2": NONE_IMAGE, "subject_3": NONE_IMAGE, "subject_4": NONE_IMAGE, "background_image": "bg.png",
      "background_mode": "use_uploaded_background", "reference_strength": "auto - based on subject count"}

BUILDER_CASES = {
    "one_auto": dict(_B, subject_1="a.png", width=64, height=96),
    "two_neutral_auto": dict(_B, subject_1="a.png", subject_3="b.png", background_image=NONE_IMAGE, background_mode="neutral_placeholder_wip",
                             width=96, height=64),
    "three_light": dict(_B, subject_1="b.png", subject_2="c.png", subject_3="d.png", reference_strength="17 - light", width=96, height=64),
    "three_auto": dict(_B, subject_1="c.png", subject_2="a.png", subject_4="d.png", width=32, height=32),
    "four_auto": dict(_B, subject_1="a.png", subject_2="b.png", subject_3="c.png", subject_4="d.png", width=64, height=96),
    "same_size_balanced": dict(_B, subject_1="same_64x96.png", subject_2="turned.png", reference_strength="25 - balanced", width=64, height=96),
    "two_strong": dict(_B, subject_1="d.png", subject_2="bg.png", background_image="same_64x96.png", reference_strength="33 - strong",
                       width=64, height=96),
    "one_strongest_neutral": dict(_B, subject_1="turned.png", background_mode="neutral_placeholder_wip", reference_strength="41 - strongest",
                                  width=32, height=64),
}

_L = {"subject_2": NONE_IMAGE, "subject_3": NONE_IMAGE, "subject_4": NONE_IMAGE, "background_image": "bg.png", "width": 64, "height": 32}

LOADER_CASES = {
    "uploaded": dict(_L, subject_1="a.png", subject_2="turned.png", subject_4="d.png", background_mode="use_uploaded_background"),
    "neutral": dict(_L, subject_1="c.png", subject_3="same_64x96.png", background_mode="neutral_placeholder_wip"),
    "none": dict(_L, subject_1="d.png", subject_2="a.png", background_mode="no_background"),
}

SURFACE_ATTRIBUTES = ("RETURN_TYPES", "RETURN_NAMES", "FUNCTION", "CATEGORY", "DESCRIPTION")


def picture(name):
    """the stored [height, width, 3] bytes of one input: smooth waves under noise, from the seed"""
    w, h, seed, _ = PICTURES[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((h, w, 3), dtype=np.uint8)
    for c in range(3):
        a, b, p = rng.uniform(0.05, 0.4, 3)
        wave = 127.5 + 100.0 * np.sin(a * xx + p) * np.cos(b * yy - p)
        out[:, :, c] = np.clip(wave + rng.integers(-27, 28, size=(h, w)), 0, 255).astype(np.uint8)
    return out


def write_inputs(directory):
    """the pictures as PNG files (lossless; one with an EXIF orientation) in `directory`"""
    from PIL import Image
    for name, (_w, _h, _seed, orientation) in PICTURES.items():
        img = Image.fromarray(picture(name), "RGB")
        if orientation is None:
            img.save(os.path.join(str(directory), name))
        else:
            exif = Image.Exif()
            exif[0x0112] = orientation
            img.save(os.path.join(str(directory), name), exif=exif)


def decoded(directory, name):
    """what both the reference and the node decode: Image.open, exif_transpose, RGB"""
    from PIL import Image, ImageOps
    return np.array(ImageOps.exif_transpose(Image.open(os.path.join(str(directory), name))).convert("RGB"))


def install_folder_paths(directory):
    """put a stand-in for ComfyUI's folder_paths over `directory` into sys.modules; returns what was there before"""
    before = sys.modules.get("folder_paths")
    mod = types.ModuleType("folder_paths")
    mod.get_input_directory = lambda: str(directory)
    mod.get_annotated_filepath = lambda name: os.path.join(str(directory), name)
    mod.filter_files_content_types = lambda files, kinds: [f for f in files if f.lower().endswith((".png", ".jpg", ".jpeg", ".webp"))]
    sys.modules["folder_paths"] = mod
    return before


def restore_folder_paths(before):
    if before is None:
        sys.modules.pop("folder_paths", None)
    else:
        sys.modules["folder_paths"] = before


def surface(module):
    """the comparable surface of the two classes and the mappings of a module (the reference's or this pack's), as plain JSON data"""
    doc = {"display": dict(module.NODE_DISPLAY_NAME_MAPPINGS), "classes": {}}
    for key, cls in module.NODE_CLASS_MAPPINGS.items():
        doc["classes"][key] = {"name": cls.__name__, "INPUT_TYPES": cls.INPUT_TYPES(),
                               **{a: getattr(cls, a, None) for a in SURFACE_ATTRIBUTES}}
    return json.loads(json.dumps(doc))


def unit(frames_u8):
    return np.asarray(frames_u8).astype(np.float32) / np.float32(255)


def resized(pic, width, height):
    """cv2.resize(pic, (width, height), INTER_LANCZOS4) by the numpy restatement; the picture itself at equal sizes"""
    return np.ascontiguousarray(restated(np.ascontiguousarray(pic)[None], int(width), int(height))[0])


def expected_frames(pictures, size, counts):
    """the launch's result: picture i (an array, or an (R, G, B) tuple) resized and repeated counts[i] times"""
    width, height = size
    frames = []
    for pic, n in zip(pictures, counts):
        if isinstance(pic, tuple):
            one = np.empty((height, width, 3), dtype=np.uint8)
            one[:] = np.array(pic, dtype=np.uint8)
        else:
            one = resized(pic, width, height)
        frames.extend([one] * int(n))
    return unit(np.stack(frames)) if frames else np.zeros((0, height, width, 3), dtype=np.float32)

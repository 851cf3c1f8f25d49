"""Reference sheets: an INDEPENDENT restatement in plain Pillow calls (Image.fromarray, resize, crop, paste, rounded_rectangle), the case
list of the sheet tests, the seeded inputs of the recorded fixtures and the host build of csrc/vrg_sheet_math.hpp
(tests/host_math/sheet_check.cpp).  Nothing here reads the reference checkout or needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import GOLDEN, PKG_DIR, ROOT

FIXTURE_JSON = os.path.join(GOLDEN, "sheet.json")
FIXTURE_NPZ = os.path.join(GOLDEN, "sheet.npz")
HOST_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse"]
HOST_SOURCE = os.path.join(ROOT, "tests", "host_math", "sheet_check.cpp")
DETAILS = ("new_w", "new_h", "win_x", "win_y", "pic_w", "pic_h", "pic_x", "pic_y", "row0", "rows", "cps", "h_ksize", "v_ksize")

# name -> (height, width, channels, seed)
SOURCES = {"7x5": (5, 7, 3, 11), "301x7": (7, 301, 3, 12), "1x1": (1, 1, 1, 13), "1x9": (9, 1, 4, 14), "9x1": (1, 9, 3, 15),
           "53x37": (37, 53, 3, 16), "97x8": (8, 97, 1, 17), "40x64": (64, 40, 3, 18), "64x40": (40, 64, 4, 19), "33x57": (57, 33, 3, 20),
           "128x72": (72, 128, 3, 21), "20x20": (20, 20, 1, 22), "90x31": (31, 90, 3, 23)}


def source(name):
    """fp32 [h, w, c]: triangle waves plus noise, reaching below 0 and above 1; "97x8" holds k / 255 and its two neighbours, -0.0, the
    infinities and values outside 0 .. 1 instead"""
    h, w, c, seed = SOURCES[name]
    rng = np.random.default_rng(seed)
    if name == "97x8":
        k = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
        v = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-2)),
                            np.array([-0.0, np.inf, -np.inf, -0.25, 1.5, 0.999999, 1.0000001, 254.5 / 255], dtype=np.float32)])
        return v.astype(np.float32).reshape(h, w, c)
    yy, xx = np.mgrid[0:h, 0:w]
    t = (xx[..., None] * 5 + yy[..., None] * 3 + np.arange(c) * 11 + seed) % 40           # a triangle wave in integers: no libm
    base = np.float32(0.05) + np.float32(0.9) * (np.abs(t - 20).astype(np.float32) / np.float32(20.0))
    noise = rng.random((h, w, c), dtype=np.float32) * 0.5 - 0.25
    return (base + np.where(rng.random((h, w, 1)) < 0.35, noise, 0.0)).astype(np.float32)


def quantise(a):
    """the reference's own line: np.clip(x * 255.0, 0, 255).astype(np.uint8) with C == 1 repeated and C > 3 cut"""
    if a.shape[-1] == 1:
        a = np.repeat(a, 3, axis=-1)
    if a.shape[-1] > 3:
        a = a[..., :3]
    with np.errstate(invalid="ignore"):
        return np.clip(a * 255.0, 0, 255).astype(np.uint8)


def P(src, rect, fit="contain_pad", cell=(184, 184, 184), radius=0):
    return {"source": src, "rect": tuple(rect), "fit": fit, "cell": tuple(cell), "radius": radius}


# the small cases: sources by name, the canvas (width, height), the background, the panels in paste order
CASES = {
    "mixed64": {"sources": ["7x5", "301x7", "1x1", "1x9", "9x1"], "canvas": (64, 64), "background": (10, 20, 30), "panels": [
        P(0, (2, 2, 30, 20), "cover_crop"), P(1, (34, 2, 5, 3), "contain_pad", (200, 100, 50)), P(1, (42, 2, 5, 3), "cover_crop"),
        P(2, (40, 10, 9, 9)), P(3, (52, 10, 6, 12), "cover_crop"), P(4, (2, 30, 20, 7), "contain_pad", (1, 2, 3)),
        P(3, (30, 30, 3, 27), "contain_pad"), P(4, (36, 40, 27, 3), "cover_crop")]},
    "skips": {"sources": ["53x37"], "canvas": (128, 72), "background": (0, 0, 0), "panels": [
        P(0, (0, 0, 53, 20), "resize"), P(0, (55, 0, 30, 37), "resize"), P(0, (0, 30, 53, 37)), P(0, (86, 0, 40, 30), "cover_crop"),
        P(0, (60, 40, 53, 20), "cover_crop")]},
    "upscale": {"sources": ["7x5"], "canvas": (200, 100), "background": (255, 255, 255), "panels": [
        P(0, (0, 0, 64, 40)), P(0, (66, 0, 64, 40), "cover_crop"), P(0, (132, 0, 64, 41), "contain_pad", (9, 99, 199)),
        P(0, (0, 50, 56, 40))]},
    "radius200": {"sources": ["7x5", "53x37"], "canvas": (200, 100), "background": (30, 0, 60), "panels": [
        P(0, (0, 0, 200, 100), radius=96), P(1, (10, 10, 40, 23), radius=3), P(1, (60, 10, 40, 23), "cover_crop", radius=96),
        P(1, (120, 50, 1, 1), radius=3), P(1, (130, 50, 5, 5), radius=2), P(1, (150, 60, 7, 3), radius=1), P(1, (170, 60, 2, 9), radius=1),
        P(1, (110, 5, 40, 23), radius=0)]},
    "overlap_clip": {"sources": ["53x37", "7x5"], "canvas": (64, 64), "background": (200, 180, 20), "panels": [
        P(0, (5, 5, 30, 30)), P(1, (20, 20, 30, 30), "cover_crop"), P(0, (50, 50, 30, 30), "cover_crop"),
        P(1, (10, 10, 20, 20), "contain_pad", (0, 255, 0), 8), P(0, (-4, 40, 20, 30), "cover_crop", radius=5)]},
    "many": {"sources": ["7x5", "9x1", "20x20"], "canvas": (67, 61), "background": (5, 6, 7), "panels": [
        P(i % 3, (1 + (i % 9) * 7, (i // 9) * 20, 6, 18), FIT, (40 + i, 0, 90), i % 4) for i, FIT in
        enumerate(["contain_pad", "cover_crop", "contain_pad"] * 9)]},
    "special": {"sources": ["97x8"], "canvas": (100, 24), "background": (0, 0, 0), "panels": [
        P(0, (1, 1, 97, 8)), P(0, (3, 11, 60, 9), "cover_crop")]},
}

# the node through the reference itself: six inputs (batched, of different sizes and channel counts)
NODE_INPUTS = ["40x64", "64x40", "33x57", "128x72", "20x20", "90x31"]
LAYOUTS = ["auto_ltx", "aspect_rows", "six_panel_story", "three_row_reference", "wide_bottom", "uniform_grid", "horizontal_strip", "vertical_strip"]
FIT_MODES = ["contain_pad", "cover_crop"]
NODE_DEFAULTS = {"image_count": 6, "layout": "auto_ltx", "output_width": 128, "output_height": 72, "columns": 0, "gutter": 4, "outer_padding": 4,
                 "corner_radius": 3, "fit_mode": "contain_pad", "batch_mode": "first_image_only", "background_color": "#102030",
                 "cell_background_color": "neutral_gray"}
NODE_CASES = {f"{layout}.{fit}": dict(NODE_DEFAULTS, layout=layout, fit_mode=fit) for layout in LAYOUTS for fit in FIT_MODES}
NODE_CASES["canvas64"] = dict(NODE_DEFAULTS, output_width=64, output_height=64, corner_radius=0, gutter=1, outer_padding=0, columns=3,
                              layout="uniform_grid", background_color="white", cell_background_color="#abc")
NODE_CASES["all_images"] = dict(NODE_DEFAULTS, image_count=3, batch_mode="all_images", layout="uniform_grid", columns=9, gutter=2, corner_radius=2)
LARGE_CASE = dict(NODE_DEFAULTS, output_width=768, output_height=448, background_color="#000000", cell_background_color="#b8b8b8")
ASPECT_LISTS = [[1.0, 1.0], [1.7778, 0.5625, 1.0], [0.05, 20.0, 1.0, 1.0], [1.5] * 5, [0.75, 1.3333, 1.0, 2.0, 0.5, 1.0], [1.0] * 7,
                [2.0, 2.0, 0.5, 0.5, 1.0, 1.0, 3.0, 0.3333], [1.7778] * 9, [0.5625] * 10, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0],
                [1.25, 0.8] * 8, [0.9 + 0.05 * i for i in range(24)]]
BUILDER_SIZES = {"subject_location": [(700, 500), (300, 420)], "flux_1": [(500, 300)], "flux_5": [(100, 80), (400, 300), (256, 256), (30, 500), (257, 90)],
                 "story_3": [(640, 360), (200, 300), (512, 512)]}       # (width, height) of the byte inputs, seeds in order


def layout_keys():
    """(layout, count, columns) of every recorded rect list, in the order of the fixture"""
    return [(layout, count, columns) for layout in LAYOUTS if layout != "aspect_rows" for count in range(1, 25) for columns in (0, 1, 3, 12)]


def aspect_keys():
    """(aspects, (canvas_width, canvas_height)) of every recorded aspect_rows list, in the order of the fixture"""
    return [(aspects, canvas) for aspects in ASPECT_LISTS for canvas in ((768, 448), (128, 72), (448, 768))]


def node_inputs(case):
    """the IMAGE inputs of a node case as fp32 arrays [B, H, W, C] by keyword"""
    if case.get("batch_mode") == "all_images":
        out = {}
        for i, name in enumerate(NODE_INPUTS[:3]):
            frames = [np.roll(source(name), 3 * k, axis=1) * np.float32(1.0 - 0.05 * k) for k in range(9)]
            out[f"image{i + 1}"] = np.stack(frames).astype(np.float32)
        return out
    return {f"image{i + 1}": source(name)[None] for i, name in enumerate(NODE_INPUTS)}


def large_inputs():
    """six 1080p frames from seeds: a coarse random field enlarged, plus fine noise"""
    out = {}
    for i in range(6):
        rng = np.random.default_rng(900 + i)
        coarse = rng.random((1080 // 8, 1920 // 8, 3), dtype=np.float32)
        fine = rng.random((1080, 1920, 3), dtype=np.float32) * np.float32(0.2) - np.float32(0.1)
        out[f"image{i + 1}"] = (np.repeat(np.repeat(coarse, 8, axis=0), 8, axis=1) + fine)[None].astype(np.float32)
    return out


def builder_inputs(key):
    return [np.random.default_rng(700 + 10 * len(key) + i).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (w, h) in enumerate(BUILDER_SIZES[key])]


# ------------------------------------------------------------------------------------------------
# plain Pillow
# ------------------------------------------------------------------------------------------------
def pillow_panel(image, w, h, fit, cell):
    from PIL import Image
    sw, sh = image.size
    if fit == "resize":
        return image.resize((w, h), Image.Resampling.LANCZOS)
    scale = max(w / sw, h / sh) if fit == "cover_crop" else min(w / sw, h / sh)
    nw, nh = max(1, int(round(sw * scale))), max(1, int(round(sh * scale)))
    resized = image.resize((nw, nh), Image.Resampling.LANCZOS)
    if fit == "cover_crop":
        left, top = max(0, (nw - w) // 2), max(0, (nh - h) // 2)
        return resized.crop((left, top, left + w, top + h))
    panel = Image.new("RGB", (w, h), tuple(cell))
    panel.paste(resized, ((w - nw) // 2, (h - nh) // 2))
    return panel


def pillow_sheet(byte_sources, panels, canvas, background):
    """uint8 [height, width, 3]: the sheet as Pillow builds it from RGB byte pictures"""
    from PIL import Image, ImageDraw
    sheet = Image.new("RGB", tuple(canvas), tuple(background))
    for p in panels:
        left, top, w, h = p["rect"]
        panel = pillow_panel(Image.fromarray(byte_sources[p["source"]], mode="RGB"), w, h, p["fit"], p["cell"])
        if p["radius"] > 0:
            mask = Image.new("L", (w, h), 0)
            ImageDraw.Draw(mask).rounded_rectangle((0, 0, w - 1, h - 1), radius=min(p["radius"], w // 2, h // 2), fill=255)
            sheet.paste(panel, (left, top), mask)
        else:
            sheet.paste(panel, (left, top))
    return np.asarray(sheet).copy()


def mask_spans(w, h, radius):
    """[h, 2]: first and last set column per row of Pillow's rounded-rectangle mask (first > last: none); asserts one run per row"""
    from PIL import Image, ImageDraw
    mask = Image.new("L", (w, h), 0)
    ImageDraw.Draw(mask).rounded_rectangle((0, 0, w - 1, h - 1), radius=radius, fill=255)
    plane = np.asarray(mask) != 0
    spans = np.zeros((h, 2), dtype=np.int32)
    for y in range(h):
        xs = np.nonzero(plane[y])[0]
        spans[y] = (xs[0], xs[-1]) if len(xs) else (1, 0)
        assert len(xs) == 0 or len(xs) == xs[-1] - xs[0] + 1, (w, h, radius, y)
    return spans


# ------------------------------------------------------------------------------------------------
# the header on the host
# ------------------------------------------------------------------------------------------------
def build_host_lib(directory):
    out = os.path.join(str(directory), "libsheet_check.so")
    cmd = ["g++", *HOST_FLAGS, "-fPIC", "-shared", "-I", os.path.join(PKG_DIR, "csrc"), "-I", os.path.join(ROOT, "include"), HOST_SOURCE, "-o", out]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.hm_sheet.restype = C.c_int32
    lib.hm_sheet.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_uint32,
                             C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hm_sheet_fit.argtypes = [C.c_int32] * 5 + [C.c_void_p]
    lib.hm_sheet_quant.restype = C.c_uint8
    lib.hm_sheet_quant.argtypes = [C.c_float]
    lib.hm_sheet_units.argtypes = [C.c_void_p]
    lib.hm_sheet_panel_bytes.restype = C.c_int32
    return lib


def panel_records(panels):
    """the integer records of tests/host_math/sheet_check.cpp and the span rows they point into"""
    recs, spans, at, n = [], [], {}, 0
    for p in panels:
        left, top, w, h = p["rect"]
        offset = -1
        if p["radius"] > 0:
            key = (w, h, min(p["radius"], w // 2, h // 2))
            if key not in at:
                at[key] = n
                spans.append(mask_spans(*key))
                n += h
            offset = at[key]
        recs.append([p["source"], left, top, w, h, ("contain_pad", "cover_crop", "resize").index(p["fit"]), *p["cell"], offset])
    return np.array(recs, dtype=np.int32).reshape(-1, 10), (np.concatenate(spans) if spans else np.zeros((1, 2), np.int32)), n


def host_sheet(lib, sources, panels, canvas, background):
    """-> (status, uint8 [H, W, 3], float32 [H, W, 3], details [n, 13]) of the header compiled for the host; sources fp32 or uint8"""
    sources = [np.ascontiguousarray(s) for s in sources]
    byte_sources = sources[0].dtype == np.uint8
    recs, spans, n_spans = panel_records(panels)
    ptrs = (C.c_void_p * len(sources))(*[s.ctypes.data for s in sources])
    shapes = np.array([s.shape for s in sources], dtype=np.int32)
    width, height = canvas
    u8, f32 = np.zeros((height, width, 3), np.uint8), np.zeros((height, width, 3), np.float32)
    details = np.zeros((len(recs), len(DETAILS)), np.int32)
    r, g, b = background
    rc = lib.hm_sheet(ptrs, shapes.ctypes.data, int(byte_sources), len(recs), recs.ctypes.data, spans.ctypes.data, n_spans, width, height,
                      r | (g << 8) | (b << 16), u8.ctypes.data, f32.ctypes.data, details.ctypes.data)
    return rc, u8, f32, details


def node_panels(grid, case, shapes):
    """the panels (dicts as in CASES) the node builds for `case` from frames of `shapes` ([(h, w, c)]), through the product's own layout
    functions (`grid`: the module comfyui_vrgamedevgirl_amd.VRGDG_LTXICIngredientsGrid)"""
    width, height = case["output_width"], case["output_height"]
    if case["layout"] == "aspect_rows":
        rects = grid.aspect_row_rects([grid.picture_aspect(w, h) for h, w, _c in shapes], width, height)
    else:
        rects = grid.layout_rects(case["layout"], len(shapes), case["columns"])
    boxes = grid.panel_rectangles(rects, width, height, case["outer_padding"], case["gutter"])
    cell = grid.parse_color(case["cell_background_color"], "#b8b8b8")
    return [P(i, box, case["fit_mode"], cell, case["corner_radius"]) for i, box in enumerate(boxes)], grid.parse_color(case["background_color"], "#000000")


def node_frames(case):
    """the frames [H, W, C] the node shows for `case`, in order"""
    inputs = node_inputs(case)
    frames = []
    for i in range(1, case["image_count"] + 1):
        batch = inputs[f"image{i}"]
        frames.extend(batch[k] for k in range(batch.shape[0] if case["batch_mode"] == "all_images" else 1))
    return frames

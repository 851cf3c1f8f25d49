"""Test scaffolding for the far-face repair contact sheet (comfyui-vrgamedevgirl_amd/far_face_repair.py: contact_sheet, pil_thumbnail,
pil_reduce; csrc/vrg_thumb.hip): the seeded inputs of tests/golden/contact_sheet.npz, the ctypes face of the library's HOST entry points
(csrc/vrg_pil_resample.hpp compiled for the host: no GPU needed) and a numpy walk that applies their tables, so that the arithmetic can be
held against the installed Pillow without a device.  The cases are shared by the fixture tool, the CPU tests and the GPU tests."""
import ctypes as C
import os

import numpy as np

from conftest import GOLDEN

FIXTURE_NPZ = os.path.join(GOLDEN, "contact_sheet.npz")
BICUBIC, LANCZOS = 3, 1
CANVAS = (24, 24, 24)

# key -> originals [(h, w)], fixed [None | "same" (the original's size) | (h, w)], limit, columns, thumb_width (`inputs`: the frames of
# another case).  The factors follow from int(pair / thumbnail / 2.0): pair width 2 w over the thumbnail's width, and likewise the height.
# The tool stores the frames and the arguments in the fixture; the tests read them there (sheet_case).
SHEET_CASES = {
    "f1":        dict(sizes=[(54, 96)] * 2, fixed=["same", None], limit=24, columns=3, thumb_width=90),         # 192 / 90: (1, 1), a missing fixed frame
    "f2":        dict(sizes=[(55, 97)] * 2, fixed=["same"] * 2, limit=24, columns=3, thumb_width=47),           # 194 / 47: (2, 2), odd w: seam
    "f3":        dict(sizes=[(55, 191)], fixed=["same"], limit=24, columns=3, thumb_width=60),                  # 56 x 8 of 382 x 55: (3, 3), 191 % 3: seam
    "f4":        dict(sizes=[(61, 193)], fixed=[None], limit=24, columns=2, thumb_width=47),                    # 44 x 7 of 386 x 61: (4, 4), 61 % 4
    "f5":        dict(sizes=[(67, 236)], fixed=[None], limit=24, columns=5, thumb_width=47),                    # 42 x 6 of 472 x 67: (5, 5), columns > count
    "f8":        dict(sizes=[(50, 384)], fixed=[None], limit=24, columns=1, thumb_width=47),                    # 46 x 3 of 768 x 50: (8, 8), 50 % 8
    "unequal":   dict(sizes=[(54, 131)], fixed=[None], limit=24, columns=2, thumb_width=47),                    # 44 x 9 of 262 x 54: (2, 3), seam
    "nothing":   dict(sizes=[(20, 40)] * 2, fixed=["same"] * 2, limit=24, columns=2, thumb_width=90),           # the pair is within 90 x 22
    "other":     dict(sizes=[(60, 101)] * 2, fixed=[(40, 70), (70, 120)], limit=24, columns=3, thumb_width=50),  # fixed frames of other sizes
    "limit":     dict(inputs="f2", limit=1, columns=3, thumb_width=47),                                         # limit < count
    "mixed":     dict(sizes=[(54, 96), (96, 54), (75, 133), (20, 30), (40, 60)], fixed=["same", None, None, "same", (30, 50)], limit=24,
                      columns=2, thumb_width=64),                                     # differing sizes in one sheet, a last row with an empty cell
}

# (h, w), requested (width, height), resample, reducing_gap: nothing to do, one factor above 1, fx != fy, no reduce, LANCZOS
THUMB_CASES = (((41, 67), (80, 50), BICUBIC, 2.0), ((41, 67), (30, 50), BICUBIC, 2.0), ((34, 120), (12, 30), BICUBIC, 2.0),
               ((50, 150), (16, 40), BICUBIC, 2.0), ((100, 65), (15, 4), BICUBIC, 2.0), ((66, 118), (20, 40), BICUBIC, None),
               ((66, 118), (17, 40), LANCZOS, 2.0), ((49, 49), (5, 5), BICUBIC, 3.0), ((64, 64), (32, 32), BICUBIC, 1.0),
               ((29, 31), (30, 30), BICUBIC, 2.0), ((150, 20), (3, 200), BICUBIC, 2.0), ((5, 31), (8, 5), BICUBIC, 2.0))

REDUCE_FACTORS = ((1, 3), (2, 1), (2, 2), (3, 3), (4, 4), (5, 5), (4, 3), (7, 6), (8, 8), (10, 10))
REDUCE_SIZES = ((40, 64), (41, 67), (29, 31), (120, 240))            # (h, w): divisible, not divisible, smaller than some cells' multiples


# the factors the cases are there for (of the first entry), asserted by the CPU tests
SHEET_FACTORS = {"f1": (1, 1), "f2": (2, 2), "f3": (3, 3), "f4": (4, 4), "f5": (5, 5), "f8": (8, 8), "unequal": (2, 3), "nothing": (1, 1)}


def random_image(seed, h, w):
    """random bytes with saturated 0 / 255 patches"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[: max(1, h // 3), : max(1, w // 4)] = 255
    img[h // 2:, w - max(1, w // 3):] = 0
    return img


def make_sheet_inputs(key):
    """FIXTURE TOOL: the seeded frames of a sheet case -> (originals, fixed): lists of arrays, fixed may hold None"""
    case = SHEET_CASES[key]
    if "inputs" in case:
        return make_sheet_inputs(case["inputs"])
    seed = 7000 + 16 * sorted(SHEET_CASES).index(key)
    originals = [random_image(seed + i, h, w) for i, (h, w) in enumerate(case["sizes"])]
    fixed = []
    for i, f in enumerate(case["fixed"]):
        fixed.append(None if f is None else random_image(seed + 8 + i, *(case["sizes"][i] if f == "same" else f)))
    return originals, fixed


def make_thumb_input(index):
    """FIXTURE TOOL: the seeded picture of a thumbnail case"""
    (h, w), _, _, _ = THUMB_CASES[index]
    return random_image(9000 + index, h, w)


def make_reduce_input(k):
    return random_image(100 + k, *REDUCE_SIZES[k])


def sheet_case(golden, key):
    """a sheet case as the fixture holds it -> (originals, fixed, limit, columns, thumb_width); fixed may hold None"""
    limit, columns, thumb_width, count = (int(v) for v in golden[f"args.{key}"])
    source = str(golden[f"inputs_of.{key}"])
    originals = [golden[f"in.{source}.o{i}"] for i in range(count)]
    fixed = [golden[f"in.{source}.f{i}"] if f"in.{source}.f{i}" in golden.files else None for i in range(count)]
    return originals, fixed, limit, columns, thumb_width


def thumb_input(golden, index):
    return golden[f"thumb_in.{index}"]


# ------------------------------------------------------------------------------------------------
# the library's host entry points
# ------------------------------------------------------------------------------------------------
def _p(a):
    return C.c_void_p(a.ctypes.data)


def host_reduce(lib, img, fx, fy):
    img = np.ascontiguousarray(img)
    h, w, c = img.shape
    out = np.zeros((-(-h // fy), -(-w // fx), c), dtype=np.uint8)
    assert lib.vrg_pil_reduce_host(_p(img), h, w, c, fx, fy, _p(out)) == 0
    return out


def host_table(lib, resample, n_in, in0, in1, n_out):
    """-> (bounds [n_out, 2], weights [n_out, ksize])"""
    ksize = lib.vrg_pil_filter_ksize(resample, in0, in1, n_out)
    assert ksize >= 1
    bounds, weights = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ksize), np.int32)
    assert lib.vrg_pil_filter_table(resample, n_in, in0, in1, n_out, _p(bounds), _p(weights)) == 0
    return bounds, weights


def apply_table(img, bounds, weights, axis):
    """one byte pass of a resize along `axis` of an [h, w, c] uint8 array"""
    img = np.moveaxis(img, axis, 0)
    out = np.empty((len(bounds),) + img.shape[1:], dtype=np.uint8)
    for xx, (x0, n) in enumerate(bounds):
        acc = np.tensordot(weights[xx, :n].astype(np.int64), img[x0:x0 + n].astype(np.int64), axes=(0, 0)) + (1 << 21)
        out[xx] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def host_box_resize(lib, img, size, resample, box_w, box_h):
    """Image.resize(size, resample, box=(0, 0, box_w, box_h)): the horizontal pass first, a pass skipped where nothing changes"""
    h, w = img.shape[:2]
    if size[0] != w or np.float32(box_w) != w:
        img = apply_table(img, *host_table(lib, resample, w, 0.0, box_w, size[0]), axis=1)
    if size[1] != h or np.float32(box_h) != h:
        img = apply_table(img, *host_table(lib, resample, h, 0.0, box_h, size[1]), axis=0)
    return np.ascontiguousarray(img)


def host_plan(lib, shapes, requests, resample=BICUBIC, gap=2.0, columns=1, pair=False):
    """vrg_thumb_plan over pictures of `shapes` [(h, w)] -> (status, entries, (cols, rows, cell_w, cell_h, tmp_bytes))"""
    from comfyui_vrgamedevgirl_amd import far_face_repair as ffr
    entries = np.zeros(len(shapes), dtype=ffr._THUMB_ENTRY)
    for e, (h, w) in zip(entries, shapes):
        e["left_h"], e["left_w"], e["right_offset"] = h, w, 0 if pair else -1
    req = np.asarray(requests, dtype=np.float64).reshape(len(shapes), 2)
    sheet = np.zeros(5, dtype=np.int64)
    rc = lib.vrg_thumb_plan(_p(entries), len(shapes), _p(req), resample, 0.0 if gap is None else gap, columns, _p(sheet))
    return rc, entries, tuple(int(v) for v in sheet)


def host_thumbnail(lib, img, request, resample=BICUBIC, gap=2.0):
    """Image.thumbnail(request, resample, gap) from the library's plan, reduce and tables"""
    h, w = img.shape[:2]
    rc, entries, _ = host_plan(lib, [(h, w)], [request], resample, gap)
    assert rc == 0
    e = entries[0]
    fx, fy = int(e["fx"]), int(e["fy"])
    red = host_reduce(lib, img, fx, fy) if (fx, fy) != (1, 1) else img
    assert red.shape[:2] == (e["red_h"], e["red_w"])
    return host_box_resize(lib, red, (int(e["out_w"]), int(e["out_h"])), resample, w / fx, h / fy), (fx, fy)


def make_pair(original, fixed):
    """Image.new('RGB', (2 w, h), black) with the original at (0, 0) and the fixed frame at (w, 0), clipped"""
    h, w = original.shape[:2]
    pair = np.zeros((h, 2 * w, 3), dtype=np.uint8)
    pair[:, :w] = original
    f = original if fixed is None else fixed
    fh, fw = min(h, f.shape[0]), min(w, f.shape[1])
    pair[:fh, w:w + fw] = f[:fh, :fw]
    return pair


def host_sheet(lib, originals, fixed, limit, columns, thumb_width):
    """the whole sheet from the library's host entry points -> (sheet, [(fx, fy)])"""
    originals, fixed = originals[:limit], fixed[:limit]
    thumbs, factors = [], []
    for o, f in zip(originals, fixed):
        pair = make_pair(o, f)
        t, fac = host_thumbnail(lib, pair, (thumb_width, int(thumb_width * pair.shape[0] / pair.shape[1])))
        thumbs.append(t)
        factors.append(fac)
    cols = max(1, columns)
    rows = -(-len(thumbs) // cols)
    cell_w, cell_h = max(t.shape[1] for t in thumbs), max(t.shape[0] for t in thumbs)
    sheet = np.empty((rows * cell_h, cols * cell_w, 3), dtype=np.uint8)
    sheet[:] = CANVAS
    for i, t in enumerate(thumbs):
        x, y = (i % cols) * cell_w, (i // cols) * cell_h
        sheet[y:y + t.shape[0], x:x + t.shape[1]] = t
    return sheet, factors


def pillow_sheet(originals, fixed, limit, columns, thumb_width):
    """the same with the installed Pillow, statement for statement as the backend's contact_sheet works on its opened images"""
    import math
    from PIL import Image
    thumbs = []
    for o, f in list(zip(originals, fixed))[:limit]:
        original = Image.fromarray(o, "RGB")
        fixed_img = original if f is None else Image.fromarray(f, "RGB")
        pair = Image.new("RGB", (original.width * 2, original.height), (0, 0, 0))
        pair.paste(original, (0, 0))
        pair.paste(fixed_img, (original.width, 0))
        pair.thumbnail((int(thumb_width), int(thumb_width * pair.height / pair.width)))
        thumbs.append(pair.copy())
    cols = max(1, int(columns))
    rows = math.ceil(len(thumbs) / cols)
    cell_w, cell_h = max(t.width for t in thumbs), max(t.height for t in thumbs)
    sheet = Image.new("RGB", (cols * cell_w, rows * cell_h), CANVAS)
    for index, thumb in enumerate(thumbs):
        sheet.paste(thumb, ((index % cols) * cell_w, (index // cols) * cell_h))
    return np.asarray(sheet)

"""The byte movers on the GPU (k_pil_paste of csrc/vrg_farface.hip, k_ff_composite of csrc/vrg_facefix.hip) over the geometry sweep of
far_face_support.MOVER_CASES -- frame seams inside a 16-byte piece, pieces that span rows, box edges at every offset within a piece, the
batch's tail, batches off the 16-byte grid -- and the five entry points that launch their records in chunks of 32768, with 32768 + 3
records each.  Every comparison is byte for byte against the numpy restatements of far_face_support / facefix_builder_support, which
tests/test_byte_movers_host.py pins to the headers on the host and to Pillow at these sizes."""
import functools

import numpy as np
import pytest
import torch

import facefix_builder_support as FS
import far_face_support as S
import lanczos_support as LS

pytestmark = pytest.mark.gpu

CASES = sorted(S.MOVER_CASES)
RECORDS = 32768 + 3                      # one full chunk of blockIdx.y and three records of the next
GUARD = 0x5A


@pytest.fixture(scope="module")
def ffr(pkg):
    from comfyui_vrgamedevgirl_amd import far_face_repair
    return far_face_repair


@pytest.fixture(scope="module")
def ff(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix
    return VRGDG_FaceFix


@pytest.fixture(scope="module")
def hip(pkg):
    from comfyui_vrgamedevgirl_amd import _hip
    return _hip


def view_at(batch, offset):
    """-> (buffer, a contiguous view of `batch` that starts `offset` bytes into it); the rest of the buffer holds GUARD"""
    raw = torch.full((batch.size + offset + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    raw[offset:offset + batch.size] = torch.from_numpy(batch).cuda().reshape(-1)
    return raw, raw[offset:offset + batch.size].view(batch.shape)


def guards_intact(raw, offset, size):
    return bool((raw[:offset] == GUARD).all()) and bool((raw[offset + size:] == GUARD).all())


def assert_same(got, want, what):
    n, first = S.first_difference(got, want)
    assert n == 0, f"{what}: {n} bytes differ, the first at (frame, y, x, c) = {first}"


def check_batch(got, want, originals, untouched, raw, x, offset, what):
    """the bytes, the frames that must come back as they were, the input and the buffer around it"""
    assert got.is_cuda and got.shape == x.shape and got.data_ptr() != x.data_ptr()
    out = got.cpu().numpy()
    assert_same(out, want, what)
    for f in untouched:
        assert np.array_equal(out[f], originals[f]), (what, f)
    assert np.array_equal(x.cpu().numpy(), originals), what
    assert guards_intact(raw, offset, originals.size), what


# ------------------------------------------------------------------------------------------------
# the far-face paste
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def far_want(name, cm, other_sizes=False, feather=-1):
    originals, repaired, masks, boxes = S.mover_inputs(name, other_sizes)
    return S.composite(originals, repaired, boxes, feather, cm, masks if feather < 0 else None)


@pytest.mark.parametrize("offset", S.MOVER_OFFSETS)
@pytest.mark.parametrize("name", CASES)
def test_far_face_paste_over_the_sweep(ffr, name, offset):
    originals, repaired, masks, boxes = S.mover_inputs(name)
    untouched = [f for f, b in enumerate(boxes) if b is None]
    for cm in (False, True):
        raw, x = view_at(originals, offset)
        assert x.data_ptr() % 16 == offset
        got = ffr.composite_frames(x, repaired, boxes, feather=-1, color_match=cm, masks=masks)
        check_batch(got, far_want(name, cm), originals, untouched, raw, x, offset, f"{name} at +{offset}, colour match {cm}")


@pytest.mark.parametrize("offset", S.MOVER_OFFSETS)
@pytest.mark.parametrize("variant", ("other_sizes", "feather2"))
def test_far_face_paste_under_resized_and_fresh_masks(ffr, variant, offset):
    """case d once with crops and saved masks of sizes unlike their boxes (both LANCZOS-resized) and once under a fresh ellipse, feather 2"""
    name, other, feather = "d_left4", variant == "other_sizes", -1 if variant == "other_sizes" else 2
    originals, repaired, masks, boxes = S.mover_inputs(name, other)
    for cm in (False, True):
        raw, x = view_at(originals, offset)
        got = ffr.composite_frames(x, repaired, boxes, feather=feather, color_match=cm, masks=masks if feather < 0 else None)
        check_batch(got, far_want(name, cm, other, feather), originals, [], raw, x, offset, f"{name} {variant} at +{offset}, colour match {cm}")


@pytest.mark.parametrize("offsets", ((0, 16), (0, 1), (4, 16)))
@pytest.mark.parametrize("name", CASES)
def test_far_face_paste_writes_its_batch_and_nothing_else(ffr, name, offsets):
    """the output as a view into a larger buffer (on the grid at +16, off it at +1): the bytes before and after it are never written"""
    originals, repaired, masks, boxes = S.mover_inputs(name)
    F, H, W = originals.shape[:3]
    raw, x = view_at(originals, offsets[0])
    plan = ffr.CompositePlan(x, ffr._boxes(boxes, F, H, W), repaired, -1, True, masks)
    plan.run_resize()
    plan.run_masks()
    plan.run_means()
    big = torch.full((originals.size + offsets[1] + 64,), GUARD, dtype=torch.uint8, device="cuda")
    plan.out = big[offsets[1]:offsets[1] + originals.size].view(x.shape)
    got = plan.run_paste()
    assert_same(got.cpu().numpy(), far_want(name, True), f"{name}, in at +{offsets[0]}, out at +{offsets[1]}")
    assert guards_intact(big, offsets[1], originals.size) and guards_intact(raw, offsets[0], originals.size)


# ------------------------------------------------------------------------------------------------
# the Builder composite
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def builder_want(name, feather, cm):
    originals, enhanced, boxes, strengths = FS.mover_inputs(name)
    return FS.composite(originals, enhanced, boxes, strengths, feather, cm)


@pytest.mark.parametrize("offset", S.MOVER_OFFSETS)
@pytest.mark.parametrize("name", CASES)
def test_builder_composite_over_the_sweep(ff, name, offset):
    originals, enhanced, boxes, strengths = FS.mover_inputs(name)
    untouched = [f for f, b in enumerate(boxes) if b is None or strengths[f] <= 0]
    e = torch.from_numpy(enhanced).cuda()
    for feather, cm in FS.MOVER_SETTINGS:
        raw, x = view_at(originals, offset)
        assert x.data_ptr() % 16 == offset
        got = ff.composite_frames(x, e, boxes, strengths, feather, cm)
        check_batch(got, builder_want(name, feather, cm), originals, untouched, raw, x, offset,
                    f"{name} at +{offset}, feather {feather}, colour match {cm}")


@pytest.mark.parametrize("offsets", ((0, 16), (0, 1), (4, 16)))
@pytest.mark.parametrize("name", CASES)
def test_builder_composite_writes_its_batch_and_nothing_else(ff, name, offsets):
    originals, enhanced, boxes, strengths = FS.mover_inputs(name)
    F, H, W = originals.shape[:3]
    raw, x = view_at(originals, offsets[0])
    plan = ff.CompositePlan(x, torch.from_numpy(enhanced).cuda(), ff._boxes(boxes, F, H, W), ff._strengths(strengths, F), True, 1, 0.65)
    plan.run_masks()
    plan.run_resize_stats()
    big = torch.full((originals.size + offsets[1] + 64,), GUARD, dtype=torch.uint8, device="cuda")
    plan.out = big[offsets[1]:offsets[1] + originals.size].view(x.shape)
    got = plan.run_composite()
    assert_same(got.cpu().numpy(), builder_want(name, 1, 0.65), f"{name}, in at +{offsets[0]}, out at +{offsets[1]}")
    assert guards_intact(big, offsets[1], originals.size) and guards_intact(raw, offsets[0], originals.size)


# ------------------------------------------------------------------------------------------------
# more records than one launch takes: every record's bytes depend on its index, and all of them are compared
# ------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _spans_3x2(n):
    """[n, 2, 2] int32: the inclusive span of each of the two rows of n masks of 3 x 2, by index (some rows empty: first > last)"""
    i = np.arange(n)
    first = np.stack([i % 3, (i // 5) % 3], axis=1)
    last = np.stack([np.minimum(2, first[:, 0] + (i // 3) % 3), 2 - (i // 7) % 2], axis=1)
    last[i % 11 == 0, 0] = first[i % 11 == 0, 0] - 1
    return np.stack([first, last], axis=2).astype(np.int32)


def _planes_3x2(spans):
    x = np.arange(3)[None, None, :]
    return (x >= spans[:, :, :1]) & (x <= spans[:, :, 1:])


def test_resize_records_past_one_launch(ffr):
    """vrg_pil_resize_u8, L images: 1 x 1 -> 2 x 2 (even records) and 2 x 1 -> 1 x 2 (odd records: both passes, through `tmp`)"""
    n = RECORDS
    odd = np.arange(n) % 2 == 1
    lengths = np.where(odd, 2, 1)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    src = _rng(9001).integers(0, 256, size=int(lengths.sum()), dtype=np.uint8)
    sizes = [(2, 1, 1, 2) if o else (1, 1, 2, 2) for o in odd]
    device = torch.device("cuda", torch.cuda.current_device())
    plan = ffr.ResizePlan(torch.from_numpy(src).to(device), [int(o) for o in offsets], sizes, 1, device)
    got = plan.run()[:plan.dst_bytes].cpu().numpy()
    at = np.asarray(plan.offsets)
    even_src = src[offsets[~odd]][None, None, :]                             # [h = 1, w = 1, records]
    odd_src = np.stack([src[offsets[odd]], src[offsets[odd] + 1]])[None]     # [h = 1, w = 2, records]
    want = np.zeros_like(got)
    want[at[~odd][:, None] + np.arange(4)] = S.resize(even_src, (2, 2)).reshape(4, -1).T
    want[at[odd][:, None] + np.arange(2)] = S.resize(odd_src, (1, 2)).reshape(2, -1).T
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, int(np.searchsorted(at, bad[0], side="right") - 1))
    assert len(np.unique(S.resize(odd_src, (1, 2)))) > 100                   # the odd records are not all alike


def test_far_face_masks_past_one_launch(ffr, hip):
    """vrg_pil_mask_u8, 3 x 2 masks: no blur, feather 1 and feather 2 in turn"""
    n = RECORDS
    spans = _spans_3x2(n)
    kind = np.arange(n) % 3
    desc = np.zeros(n, dtype=ffr._MASK_DESC)
    desc["width"], desc["height"], desc["radius"] = 3, 2, -1
    for k, feather in ((1, 1), (2, 2)):
        r, ww, fw = ffr.box_parameters(feather)
        assert (r, ww, fw) == S.box_parameters(feather)
        desc["radius"][kind == k], desc["ww"][kind == k], desc["fw"][kind == k] = r, ww, fw
    desc["span_offset"], desc["mask_offset"] = 2 * np.arange(n), 6 * np.arange(n)
    device = torch.device("cuda", torch.cuda.current_device())
    dev_spans, dev_desc = ffr._upload(spans, device), ffr._upload(desc, device)
    masks = torch.full((6 * n + 64,), GUARD, dtype=torch.uint8, device=device)
    scratch = torch.zeros(6 * n, dtype=torch.uint8, device=device)
    hip.check(hip.lib().vrg_pil_mask_u8(hip.ptr(dev_spans), 2 * n, hip.ptr(dev_desc), n, 3, 2, hip.ptr(scratch), hip.ptr(masks), 6 * n,
                                        hip.current_stream()), "vrg_pil_mask_u8")
    got = masks.cpu().numpy()
    want = (_planes_3x2(spans) * 255).astype(np.uint8)
    for k, feather in ((1, 1), (2, 2)):
        x = want[kind == k]
        box = S.box_parameters(float(feather))
        for _ in range(3):
            x = S._box_lines_prefix(x, *box)
        x = np.ascontiguousarray(np.swapaxes(x, 1, 2))
        for _ in range(3):
            x = S._box_lines_prefix(x, *box)
        want[kind == k] = np.swapaxes(x, 1, 2)
    bad = np.argwhere(got[:6 * n].reshape(n, 2, 3) != want)
    assert len(bad) == 0, (len(bad), tuple(bad[0]))
    assert (got[6 * n:] == GUARD).all()
    assert np.array_equal(want[1], S.gaussian_blur((_planes_3x2(spans[1:2])[0] * 255).astype(np.uint8), 1.0))     # the batched blur is the blur


def test_builder_crops_past_one_launch(ff, hip):
    """vrg_lanczos4_boxes_u8: 2 x 2 crops of boxes of 2 x 2 (a copy) and 3 x 3 anywhere in one 8 x 8 frame"""
    n = RECORDS
    frames = FS.make_frames("random", (1, 8, 8, 3), 9002)
    combos = [(left, top, s) for s in (2, 3) for top in range(6) for left in range(6)]
    which = (np.arange(n) * 5 + np.arange(n) // 72) % len(combos)
    assert (which[:3] != which[32768:]).all()
    table, tap_offsets = ff._tap_tables([(2, 2), (3, 3)], lambda s: s, lambda s: (2, 2))
    desc = np.zeros(n, dtype=ff._BOX_DESC)
    per = np.array([(0, left, top, s, s, 0, tap_offsets[(s, s)]) for left, top, s in combos], dtype=ff._BOX_DESC)
    desc[:] = per[which]
    device = torch.device("cuda", torch.cuda.current_device())
    x = torch.from_numpy(frames).to(device)
    out = torch.full((n * 12 + 64,), GUARD, dtype=torch.uint8, device=device)
    taps, dev_desc = ff._upload(table, device), ff._upload(desc, device)
    hip.check(hip.lib().vrg_lanczos4_boxes_u8(hip.ptr(x), 1, 8, 8, hip.ptr(out), hip.ptr(dev_desc), n, 2, 2, hip.ptr(taps), len(table),
                                              hip.current_stream()), "vrg_lanczos4_boxes_u8")
    crops = np.stack([FS.crops(frames, [(left, top, left + s, top + s)], 2)[0] for left, top, s in combos])
    got = out.cpu().numpy()
    bad = np.argwhere(got[:n * 12].reshape(n, 2, 2, 3) != crops[which])
    assert len(bad) == 0, (len(bad), tuple(bad[0]))
    assert (got[n * 12:] == GUARD).all()


@pytest.mark.parametrize("feather", (0, 1))
def test_builder_masks_past_one_launch(ff, hip, feather):
    """vrg_ff_masks_f32, 3 x 2 masks: the spans alone (no coefficients) and blurred with feather 1"""
    n = RECORDS
    spans = _spans_3x2(n)
    desc = np.zeros(n, dtype=ff._MASK_DESC)
    desc["width"], desc["height"], desc["span_offset"], desc["mask_offset"] = 3, 2, 2 * np.arange(n), 6 * np.arange(n)
    device = torch.device("cuda", torch.cuda.current_device())
    got = ff._run_masks(spans.reshape(-1, 2), desc, 6 * n, 6, feather, device).cpu().numpy().reshape(n, 2, 3)
    want = _planes_3x2(spans).astype(np.float32)
    if feather:
        want = FS.blur(want, FS.gauss_coeffs(FS.gauss_taps(feather), max(0.1, feather))).clip(0.0, 1.0)
        assert np.array_equal(want[1], FS.blur(_planes_3x2(spans[1:2])[0], FS.gauss_coeffs(5, 1.0)).clip(0.0, 1.0))
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), tuple(bad[0]))


def test_builder_resize_statistics_and_composite_past_one_launch(ff, hip):
    """vrg_ff_resize_stats_u8 and the composite over its result: 4 x 4 frames, a 2 x 2 box placed by the frame's index, 3 x 3 repaired
    frames, strengths 1.0 and 0.65 in turn; the resized bytes, the seven sums of every frame and the output batch"""
    n = RECORDS
    originals = FS.make_frames("random", (n, 4, 4, 3), 9003)
    enhanced = FS.make_frames("random", (n, 3, 3, 3), 9004)
    i = np.arange(n)
    left, top = (i + i // 32768) % 3, (i // 3) % 3
    strengths = np.where(i % 2 == 0, 1.0, 0.65)
    boxes = [(int(l), int(t), 2, 2) for l, t in zip(left, top)]
    x, e = torch.from_numpy(originals).cuda(), torch.from_numpy(enhanced).cuda()
    plan = ff.CompositePlan(x, e, boxes, [float(s) for s in strengths], True, 1, 0.65)
    plan.run_masks()
    plan.run_resize_stats()
    face = plan.face.cpu().numpy().reshape(n, 2, 2, 3)
    stats = plan.stats.cpu().numpy().reshape(n, hip.FACEFIX_STATS_WORDS)
    got = plan.run_composite().cpu().numpy()

    resized = np.asarray(LS.restated(enhanced, 2, 2))
    bad = np.argwhere(face != resized)
    assert len(bad) == 0, ("resized bytes", len(bad), tuple(bad[0]))
    mask = FS.soft_ellipse_mask(2, 2, 1)
    rows, cols = top[:, None, None] + np.arange(2)[None, :, None], left[:, None, None] + np.arange(2)[None, None, :]
    target = originals[i[:, None, None], rows, cols]                          # [n, 2, 2, 3]
    sel = mask > np.float32(0.35)
    sums = np.concatenate([np.full((n, 1), int(sel.sum())), resized[:, sel].astype(np.int64).sum(axis=1), target[:, sel].astype(np.int64).sum(axis=1)], axis=1)
    assert sel.sum() < 16 and np.array_equal(sums[0], FS.color_match(resized[0], target[0], mask, 0.65)[1])
    bad = np.argwhere(stats[:, :7] != sums)
    assert len(bad) == 0, ("sums", len(bad), tuple(bad[0]))
    assert not stats[:, 7:].any()                                           # four pixels: never matched, no shift
    a = (mask[None] * strengths.astype(np.float32)[:, None, None])[..., None]
    blended = np.clip(target.astype(np.float32) * (np.float32(1.0) - a) + resized.astype(np.float32) * a, 0, 255).astype(np.uint8)
    assert np.array_equal(blended[1], FS.blend(target[1], resized[1], mask, 0.65))
    want = originals.copy()
    want[i[:, None, None], rows, cols] = blended
    assert_same(got, want, "the composite of 32771 frames")
    assert np.array_equal(x.cpu().numpy(), originals)


@pytest.mark.parametrize("color_match", (False, True))
def test_far_face_composite_past_one_launch(ffr, color_match):
    """composite_frames over 32771 frames of 4 x 4: a 2 x 2 box placed by the frame's index, crops and saved masks resized from 1 x 1
    (even frames) or copied from 2 x 2 (odd frames); four pixels are never colour matched"""
    n = RECORDS
    originals = S.random_image(9005, n * 4, 4).reshape(n, 4, 4, 3)
    i = np.arange(n)
    left, top = (i + i // 32768) % 3, (i // 3) % 3
    crops = S.random_image(9006, n * 2, 2).reshape(n, 2, 2, 3)
    masks = S.random_image(9007, n * 2, 2, 0).reshape(n, 2, 2)
    crops[::2], masks[::2] = crops[::2, :1, :1].copy(), masks[::2, :1, :1].copy()          # what a 1 x 1 source resizes to: its one value everywhere
    repaired = [c[:1, :1] if k % 2 == 0 else c for k, c in enumerate(crops)]
    saved = [m[:1, :1] if k % 2 == 0 else m for k, m in enumerate(masks)]
    assert np.array_equal(S.resize(repaired[0], (2, 2)), crops[0]) and np.array_equal(S.resize(saved[0], (2, 2)), masks[0])
    boxes = [(int(l), int(t), int(l) + 2, int(t) + 2) for l, t in zip(left, top)]
    x = torch.from_numpy(originals).cuda()
    got = ffr.composite_frames(x, repaired, boxes, feather=-1, color_match=color_match, masks=saved).cpu().numpy()
    rows, cols = top[:, None, None] + np.arange(2)[None, :, None], left[:, None, None] + np.arange(2)[None, None, :]
    target = originals[i[:, None, None], rows, cols]
    m = masks.astype(np.int64)[..., None]
    t = target.astype(np.int64) * (255 - m) + crops.astype(np.int64) * m + 128
    pasted = (((t >> 8) + t) >> 8).astype(np.uint8)
    assert np.array_equal(pasted[1], S.paste(target[1], crops[1], masks[1]))
    want = originals.copy()
    want[i[:, None, None], rows, cols] = pasted
    assert np.array_equal(want[:2], S.composite(originals[:2], repaired[:2], boxes[:2], -1, color_match, saved[:2]))
    assert_same(got, want, "the composite of 32771 frames")
    assert np.array_equal(x.cpu().numpy(), originals)

"""The packed far-face repair composite on the GPU (far_face_repair.composite_boxes_packed / composite_frames_packed,
csrc/vrg_farface_packed.hip): frames on the host, only the boxes cross the bus.  Every comparison is byte for byte: against the recorded
bytes of tests/golden/far_face.{json,npz} where they exist, against the numpy restatement of tests/far_face_support.py elsewhere, and
against the unchanged whole-frame ``composite_frames`` on the same inputs."""
import ctypes as C
import functools
import hashlib
import json

import numpy as np
import pytest
import torch

import far_face_support as S
import stream_support

pytestmark = pytest.mark.gpu

TILE = 256
GUARD, GUARD_BYTE = 64, 0x5A


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def ffr(pkg):
    from comfyui_vrgamedevgirl_amd import far_face_repair
    torch.cuda.set_device(0)
    return far_face_repair


@pytest.fixture(scope="module")
def hip(ffr):
    from comfyui_vrgamedevgirl_amd import _hip
    assert _hip.PIL_PACKED_TILE == TILE
    return _hip


@pytest.fixture(scope="module")
def golden():
    with open(S.FIXTURE_JSON) as fh:
        return json.load(fh), np.load(S.FIXTURE_NPZ)


@pytest.fixture(scope="module")
def composite_inputs():
    return S.composite_inputs()


def _cut(frames, boxes):
    return [np.asarray(frames[f])[b[1]:b[3], b[0]:b[2]] for f, b in enumerate(boxes) if b is not None]


def _same(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


# ---- the recorded variants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(S.COMPOSITE_VARIANTS)))
def test_recorded_variants_through_the_three_routes(ffr, golden, composite_inputs, index):
    originals, repaired, masks = composite_inputs
    feather, cm = S.COMPOSITE_VARIANTS[index]
    rec = golden[0]["composites"][index]
    boxes = S.COMPOSITE_BOXES
    plan = ffr.packed_plan(*originals.shape[:3], boxes)
    tensor = torch.from_numpy(originals.copy())
    # 1. the boxes alone
    blocks = ffr.composite_boxes_packed(tensor, repaired, boxes, feather, cm, masks)
    moved = ffr.last_transfer()
    assert moved["bytes_up"] == moved["bytes_down"] == plan.bytes_up < originals.nbytes
    assert moved["repaired_up"] == sum(r.size for r in repaired) + (sum(m.size for m in masks) if feather < 0 else 0) and moved["tables_up"] > 0
    assert [b.shape for b in blocks] == [(h, w, 3) for _, _, w, h in plan.boxes]
    for f in rec["stored_boxes"]:
        assert np.array_equal(blocks[plan.frames.index(f)], golden[1][f"composite.{index}.{f}"]), f
    # 2. a CPU tensor in, a CPU tensor out; repaired and masks one entry per frame
    out = ffr.composite_frames_packed(tensor, repaired + [None], boxes, feather, cm, masks + [None])
    assert isinstance(out, torch.Tensor) and not out.is_cuda and out.shape == tensor.shape and out.data_ptr() != tensor.data_ptr()
    assert [sha(f) for f in out.numpy()] == rec["frame_sha256"]
    assert _same(blocks, _cut(out.numpy(), boxes))
    assert np.array_equal(tensor.numpy(), originals)                         # inputs never written
    # 3. a list, in place: the caller's own list and frames
    listed = [f.copy() for f in originals]
    back = ffr.composite_frames_packed(listed, [torch.from_numpy(r) for r in repaired], boxes, feather, cm, masks, inplace=True)
    assert back is listed and [sha(f) for f in listed] == rec["frame_sha256"]
    copies = ffr.composite_frames_packed([f for f in originals], repaired, boxes, feather, cm, masks)
    assert isinstance(copies, list) and [sha(f) for f in copies] == rec["frame_sha256"] and np.array_equal(tensor.numpy(), originals)
    # the unchanged whole-frame route on the same inputs
    whole = ffr.composite_frames(tensor.cuda(), repaired, boxes, feather, cm, masks).cpu().numpy()
    assert np.array_equal(whole, out.numpy())
    fresh = S.composite_inputs()
    assert all(np.array_equal(a, b) for a, b in zip(repaired, fresh[1])) and all(np.array_equal(a, b) for a, b in zip(masks, fresh[2]))


# ---- the geometry sweep -------------------------------------------------------------------------------------------------------------------
SWEEP_H, SWEEP_W = 40, 700
SWEEP_BOXES = [None,
               (0, 0, 1, 1), (699, 0, 700, 1), (0, 39, 1, 40), (699, 39, 700, 40),          # 1 x 1 in the four corners
               (10, 3, 11, 10), (20, 5, 27, 6),                                             # 1 x 7 and 7 x 1
               (100, 10, 116, 26),                                                          # 16 x 16: exactly one tile, and matched
               (200, 7, 457, 8),                                                            # 257 x 1: a tile plus one pixel
               (300, 4, 364, 36),                                                           # 64 x 32 = 2048: one chunk of the means
               (5, 20, 688, 23),                                                            # 683 x 3 = 2049: a chunk plus one
               (0, 0, 700, 40),                                                             # the whole frame
               (50, 30, 53, 33),                                                            # 3 x 3: fewer than 16 pixels, never matched
               (117, 11, 133, 27),                                                          # 16 x 16 beside it
               (400, 10, 430, 30),                                                          # its repaired crop has its size already
               None]
SWEEP_OWN_SIZE = 14
SWEEP_VARIANTS = [(f, cm) for f in (0, 1, 18, -1) for cm in (False, True)]


@functools.lru_cache(maxsize=None)
def sweep_inputs():
    originals = np.stack([S.random_image(9400 + f, SWEEP_H, SWEEP_W) for f in range(len(SWEEP_BOXES))])
    repaired, masks = [], []
    for f, b in enumerate(SWEEP_BOXES):
        if b is None:
            continue
        w, h = b[2] - b[0], b[3] - b[1]
        cw, ch = (w, h) if f == SWEEP_OWN_SIZE else (w + 3 + f, max(1, h - 2) if h > 3 else h + 2)
        repaired.append(S.random_image(9500 + f, ch, cw, 3, 0, 200))
        m = S.random_image(9600 + f, ch + 1, cw + 2, 0, 0, 256)               # saved masks of other sizes again
        masks.append(np.maximum(m, 128) if f in (7, 13) else m)              # the two 16 x 16 boxes: every pixel selected
    return originals, repaired, masks


@functools.lru_cache(maxsize=None)
def sweep_want(feather, cm):
    originals, repaired, masks = sweep_inputs()
    return S.composite(originals, repaired, SWEEP_BOXES, feather, cm, masks)


def test_sweep_is_what_it_says(ffr):
    originals, repaired, masks = sweep_inputs()
    assert len(SWEEP_BOXES) == 16 and SWEEP_BOXES[0] is None and SWEEP_BOXES[-1] is None
    plan = ffr.packed_plan(16, SWEEP_H, SWEEP_W, SWEEP_BOXES)
    px = [w * h for _, _, w, h in plan.boxes]
    assert px == [1, 1, 1, 1, 7, 7, TILE, TILE + 1, 2048, 2049, 28000, 9, 256, 600]
    assert [int(b - a) for a, b in zip(plan.tile_prefix, plan.tile_prefix[1:])] == [1, 1, 1, 1, 1, 1, 1, 2, 8, 9, 110, 1, 1, 3]
    assert plan.tiles == 141 and (257, 1) == plan.boxes[7][2:] and (64, 32) == plan.boxes[8][2:] and (683, 3) == plan.boxes[9][2:]
    assert any(o % 4 for o in plan.offsets) and any(o % 16 for o in plan.offsets)
    for k, ((_, _, w, h), r) in enumerate(zip(plan.boxes, repaired)):
        assert (r.shape[:2] == (h, w)) == (plan.frames[k] == SWEEP_OWN_SIZE)
    # the 15 / 16 facts: a 3 x 3 box never has 16 selected pixels; the 16 x 16 boxes have them under the saved masks and the sharp ellipses
    for k in (6, 12):
        for feather in (0, 1):
            assert int((S.soft_face_mask((16, 16), feather) >= 64).sum()) >= 16
        assert int((S.resize(masks[k], (16, 16)) >= 64).sum()) >= 16
    assert plan.boxes[11][2:] == (3, 3)


@pytest.mark.parametrize("feather,cm", SWEEP_VARIANTS, ids=[f"feather{f}-{'match' if cm else 'plain'}" for f, cm in SWEEP_VARIANTS])
def test_geometry_sweep(ffr, feather, cm):
    originals, repaired, masks = sweep_inputs()
    want = sweep_want(feather, cm)
    frames = [f.copy() for f in originals]
    blocks = ffr.composite_boxes_packed(frames, repaired, SWEEP_BOXES, feather, cm, masks)
    wanted = _cut(want, SWEEP_BOXES)
    for k, (g, w) in enumerate(zip(blocks, wanted)):
        assert g.shape == w.shape and np.array_equal(g, w), (k, int((g != w).sum()))
    assert len(blocks) == len(wanted) and all(np.array_equal(a, b) for a, b in zip(frames, originals))
    out = ffr.composite_frames_packed(torch.from_numpy(originals), repaired, SWEEP_BOXES, feather, cm, masks)
    assert np.array_equal(out.numpy(), want)
    whole = ffr.composite_frames(torch.from_numpy(originals).cuda(), repaired, SWEEP_BOXES, feather, cm, masks).cpu().numpy()
    assert np.array_equal(whole, want)
    if cm and feather in (0, 1, -1):                                         # the colour match moved the matched box and not the 3 x 3 one
        plain = sweep_want(feather, False)
        assert not np.array_equal(want[13], plain[13]) and np.array_equal(want[12], plain[12])


# ---- the tile map's seams in one call ------------------------------------------------------------------------------------------------------
#: boxes at which the shared tile map (csrc/vrg_packed_tiles.hpp) can go wrong, one per frame of 32 x 300: a single pixel, 255 pixels (one
#: short of a tile), 256 (exactly one), 257 x 1 (a tile plus one pixel), and a frame without a box -- five frames, since a frame has one box.
#: This route admits all four sizes.
SEAM_H, SEAM_W = 32, 300
SEAM_BOXES = [(7, 5, 8, 6), (20, 3, 35, 20), None, (100, 10, 116, 26), (30, 31, 287, 32)]


@pytest.mark.parametrize("cm", (False, True), ids=("plain", "match"))
def test_tile_seams_equal_the_whole_frame_route(ffr, cm):
    plan = ffr.packed_plan(len(SEAM_BOXES), SEAM_H, SEAM_W, SEAM_BOXES)
    assert [w * h for _, _, w, h in plan.boxes] == [1, 255, 256, 257] and list(plan.tile_prefix) == [0, 1, 2, 3, 5] and plan.frames == [0, 1, 3, 4]
    originals = np.stack([S.random_image(9700 + f, SEAM_H, SEAM_W) for f in range(len(SEAM_BOXES))])
    repaired = [S.random_image(9710 + k, h + 2, w + 3, 3, 0, 200) for k, (_, _, w, h) in enumerate(plan.boxes)]
    got = ffr.composite_frames_packed(torch.from_numpy(originals), repaired, SEAM_BOXES, 1, cm)
    whole = ffr.composite_frames(torch.from_numpy(originals).cuda(), repaired, SEAM_BOXES, 1, cm)
    assert np.array_equal(got.numpy(), whole.cpu().numpy())
    assert np.array_equal(got[2].numpy(), originals[2]) and not np.array_equal(got.numpy(), originals)
    for f, (left, top, w, h) in zip(plan.frames, plan.boxes):                # nothing outside a box was written
        outside = np.ones((SEAM_H, SEAM_W), dtype=bool)
        outside[top:top + h, left:left + w] = False
        assert np.array_equal(got[f].numpy()[outside], originals[f][outside]), f


# ---- the means: 15 / 16 selected pixels, sums beyond 2^24 ------------------------------------------------------------------------------------
def test_the_selection_boundary_on_saved_masks(ffr):
    frames, repaired, masks, boxes = [], [], [], []
    for f, key in enumerate(("sel15", "sel16", "sel15", "sel16")):
        o, r, m = S.means_inputs(key)
        frame = S.random_image(9700 + f, 11, 13)
        left, top = 1 + 2 * f, f
        frame[top:top + 6, left:left + 6] = o
        frames.append(frame)
        repaired.append(r)
        masks.append(m)
        boxes.append((left, top, left + 6, top + 6))
    originals = np.stack(frames)
    want = S.composite(originals, repaired, boxes, -1, True, masks)
    plain = S.composite(originals, repaired, boxes, -1, False, masks)
    assert np.array_equal(want[0], plain[0]) and not np.array_equal(want[1], plain[1])       # 15: no shift; 16: shifted
    got = ffr.composite_frames_packed(torch.from_numpy(originals), repaired, boxes, -1, True, masks)
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(ffr.composite_frames(torch.from_numpy(originals).cuda(), repaired, boxes, -1, True, masks).cpu().numpy(), want)


def test_steered_case_matches_the_recorded_bytes(ffr, golden):
    """fp32 sums beyond 2^24: an implementation with exact means moves every byte of the box by a level (exact_route_sha256)"""
    rec = golden[0]["steered"]
    frames, rep, masks = S.steered_inputs(rec["k"])
    got = ffr.composite_frames_packed(torch.from_numpy(frames), rep, [S.STEERED_BOX], -1, True, masks).numpy()
    assert sha(got) == rec["sha256"] and sha(got) != rec["exact_route_sha256"]
    assert ffr.last_transfer()["bytes_up"] == 400 * 400 * 3 < frames.nbytes


def test_many_small_boxes(ffr):
    """700 records of one tile each: the prefix search runs over 700 equal steps"""
    n = 700
    originals = S.random_image(9800, n * 6, 6).reshape(n, 6, 6, 3)
    boxes = [(1, 2, 3, 4) if f % 2 == 0 else (3, 0, 6, 3) for f in range(n)]
    crops = [S.random_image(9801, 5, 4), S.random_image(9802, 2, 7), S.random_image(9803, 3, 3)]
    repaired = [crops[f % 3] for f in range(n)]
    plan = ffr.packed_plan(n, 6, 6, boxes)
    assert list(plan.tile_prefix) == list(range(n + 1))
    want = S.composite(originals, repaired, boxes, 1, True)
    got = ffr.composite_frames_packed(torch.from_numpy(originals), repaired, boxes, 1, True)
    assert np.array_equal(got.numpy(), want)
    assert ffr.last_transfer()["bytes_up"] == sum(w * h * 3 for _, _, w, h in plan.boxes)


# ---- through the C ABI by hand ---------------------------------------------------------------------------------------------------------------
ABI_BOXES = [(5, 7), (16, 16), (1, 1), (300, 2), (64, 33), (7, 5)]           # (w, h)


def _guarded(nbytes, device):
    t = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=device)
    return t, t[GUARD:GUARD + nbytes]


def _guards_intact(t, nbytes):
    host = t.cpu().numpy()
    return bool((host[:GUARD] == GUARD_BYTE).all() and (host[GUARD + nbytes:] == GUARD_BYTE).all())


def test_through_the_c_abi_by_hand(ffr, hip):
    device = torch.device("cuda", 0)
    lib = hip.lib()
    blocks = [(S.random_image(9900 + k, h, w), S.random_image(9910 + k, h, w, 3, 0, 180), S.random_image(9920 + k, h, w, 0, 0, 256))
              for k, (w, h) in enumerate(ABI_BOXES)]
    n = len(blocks)
    desc = np.zeros(n, dtype=hip.record_dtype(hip.PilPackedDesc))
    at = at_mask = 0
    for k, (w, h) in enumerate(ABI_BOXES):
        desc[k] = (at, at, w, h, 1, 0, at_mask, at)
        at, at_mask = at + w * h * 3, at_mask + w * h
    total, mask_total = at, at_mask
    prefix = np.concatenate([[0], np.cumsum([-(-(w * h) // TILE) for w, h in ABI_BOXES])]).astype(np.int64)
    tiles = int(prefix[-1])
    src_host = np.concatenate([b[0].reshape(-1) for b in blocks])
    src = torch.from_numpy(src_host).to(device)
    rep = torch.from_numpy(np.concatenate([b[1].reshape(-1) for b in blocks])).to(device)
    masks = torch.from_numpy(np.concatenate([b[2].reshape(-1) for b in blocks])).to(device)
    stream = torch.cuda.current_stream().cuda_stream

    def run(table, grid):
        """-> (stats [n, 12] uint32, out bytes) of the two launches on `table`, every written buffer between guards"""
        assert table.nbytes % 8 == 0
        dev_desc = hip.upload_records(table, device, trailing=(prefix,))
        stats_all, stats = _guarded(n * 12 * 4, device)
        out_all, out = _guarded(total, device)
        args = (hip.ptr(src), total, hip.ptr(rep), total, hip.ptr(masks), mask_total, hip.ptr(dev_desc))
        assert lib.vrg_np_packed_masked_means_f32(*args, hip.ptr(stats), n, 0.65, stream) == 0
        assert lib.vrg_pil_packed_paste_u8(*args, C.c_void_p(dev_desc.data_ptr() + table.nbytes), n, grid, hip.ptr(stats), hip.ptr(out), total,
                                           stream) == 0
        torch.cuda.synchronize()
        assert _guards_intact(stats_all, n * 48) and _guards_intact(out_all, total)
        assert np.array_equal(src.cpu().numpy(), src_host)                   # the packed originals are never written
        return stats.cpu().numpy().view(np.uint32).reshape(n, 12), out.cpu().numpy()

    def check(table):
        return hip.host_library().vrg_pil_packed_check(C.c_void_p(table.ctypes.data), n, C.c_void_p(prefix.ctypes.data), total, total, mask_total,
                                                       total)

    want_stats, want_out = [], []
    for o, r, m in blocks:
        adjusted, count, om, rm, shift = S.color_match(o, r, m)
        want_stats.append([count] + S.bits(om) + S.bits(rm) + S.bits(shift) + [int(count >= 16), 0])
        want_out.append(S.paste(o, adjusted, m).reshape(-1))
    want_stats = np.array(want_stats, dtype=np.uint32)
    assert {bool(s[10]) for s in want_stats} == {True, False}                # a matched and an unmatched record
    assert check(desc) == 0
    stats, out = run(desc, tiles)
    assert np.array_equal(stats, want_stats)
    assert np.array_equal(out, np.concatenate(want_out))
    stats3, out3 = run(desc, tiles + 3)                                      # a grid longer than the table
    assert np.array_equal(stats3, stats) and np.array_equal(out3, out)

    plain = desc.copy()
    plain["color_match"] = 0                                                  # no colour match: zero records, the crops pasted as they are
    stats0, out0 = run(plain, tiles)
    assert not stats0.any()
    assert np.array_equal(out0, np.concatenate([S.paste(o, r, m).reshape(-1) for o, r, m in blocks]))

    bad = desc.copy()
    bad[1]["rep_offset"] = total - 5                                          # the crop leaves its buffer: a copy of the original block
    bad[2]["src_offset"] = -1                                                 # nowhere to read: the output is left alone
    bad[3]["box_w"] = 0                                                       # no box: the output is left alone
    bad[5]["mask_offset"] = -1                                                # the mask leaves its buffer: a copy
    assert check(bad) == 1
    for k in (1, 2, 3, 5):
        one = desc.copy()
        one[k] = bad[k]
        assert check(one) == 1, k
    stats_b, out_b = run(bad, tiles)
    sizes = [w * h * 3 for w, h in ABI_BOXES]
    for k, (size, offset) in enumerate(zip(sizes, desc["src_offset"])):
        got = out_b[offset:offset + size]
        if k in (1, 5):
            assert np.array_equal(got, src_host[offset:offset + size]) and not stats_b[k].any(), k
        elif k in (2, 3):
            assert (got == GUARD_BYTE).all() and not stats_b[k].any(), k
        else:                                                                 # the neighbours are unchanged
            assert np.array_equal(got, out[offset:offset + size]) and np.array_equal(stats_b[k], want_stats[k]), k


# ---- refusals and empty calls ---------------------------------------------------------------------------------------------------------------
def test_gpu_resident_inputs_are_refused_by_name(ffr, composite_inputs):
    from comfyui_vrgamedevgirl_amd.VRGDG_StandaloneVideoEnhancerNodes import DecodedFrames
    originals, repaired, masks = composite_inputs
    tensor = torch.from_numpy(originals)
    for call in (ffr.composite_boxes_packed, ffr.composite_frames_packed):
        with pytest.raises(TypeError, match="use composite_frames"):
            call(tensor.cuda(), repaired, S.COMPOSITE_BOXES)
        with pytest.raises(TypeError, match="use composite_frames"):
            call(DecodedFrames(tensor.cuda()), repaired, S.COMPOSITE_BOXES)
        with pytest.raises(TypeError, match="use composite_frames"):
            call(tensor, [torch.from_numpy(r).cuda() for r in repaired], S.COMPOSITE_BOXES)
        with pytest.raises(TypeError, match="use composite_frames"):
            call(tensor, repaired, S.COMPOSITE_BOXES, -1, False, [torch.from_numpy(m).cuda() for m in masks])


def test_no_box_moves_nothing(ffr, composite_inputs):
    originals = composite_inputs[0]
    ffr.composite_boxes_packed(torch.from_numpy(originals), composite_inputs[1], S.COMPOSITE_BOXES)
    assert ffr.last_transfer()["bytes_up"] > 0
    none = [None] * len(originals)
    assert ffr.composite_boxes_packed(torch.from_numpy(originals), [], none) == []
    assert ffr.last_transfer() == {"bytes_up": 0, "bytes_down": 0, "repaired_up": 0, "tables_up": 0}
    out = ffr.composite_frames_packed(torch.from_numpy(originals), [], none, 18, True)
    assert np.array_equal(out.numpy(), originals) and ffr.last_transfer()["bytes_down"] == 0


# ---- stream order ---------------------------------------------------------------------------------------------------------------------------
def _packed_case(ops, dev):
    """frames on the host: only the boxes cross the bus, in and out (no device input to poison: the outputs and the flags are probed)"""
    from comfyui_vrgamedevgirl_amd import far_face_repair as FR
    originals = stream_support._bytes((3, 90, 120, 3), 95)
    crops = [stream_support._bytes((48, 40, 3), 96).numpy(), stream_support._bytes((100, 130, 3), 97).numpy()]
    masks = [stream_support._bytes((33, 29), 98).numpy(), stream_support._bytes((20, 20), 99).numpy()]

    def call(inp, out):
        fresh = FR.composite_boxes_packed(originals, crops, stream_support.FF_BOXES, 6, True)              # fresh soft ellipses, colour match
        saved = FR.composite_boxes_packed(originals, crops, stream_support.FF_BOXES, -1, True, masks)      # the saved masks, resized
        return tuple(torch.from_numpy(np.concatenate([b.reshape(-1) for b in boxes])) for boxes in (fresh, saved))
    return [], call


def test_launches_go_to_the_callers_stream(ffr):
    """The call waits on the host for its download (and its record uploads), so it is armed against the default stream only, like
    facefix_builder_packed of tests/stream_support.py."""
    from comfyui_vrgamedevgirl_amd import ops
    case = stream_support.Case("far_face_packed", _packed_case, ("far_face_repair.ResizePlan.run", "far_face_repair.MaskPlan.run",
                                                                 "far_face_repair.CompositePlan.run_means", "far_face_repair.CompositePlan.run_paste"))
    spin = stream_support.Spin()
    inputs, call = case.build(ops, torch.device("cuda", 0))
    torch.cuda.synchronize()
    r = stream_support.probe(ops, case, inputs, call, spin)
    print(f"\n[stream order] {case.name}: host {r['host_ms']:.3f} ms, spins {r['early_ms']:.1f} / {r['late_ms']:.1f} ms, "
          f"armed early {r['armed_early']} late {r['armed_late']}")
    assert r["armed_late"], f"the spin on the default stream had ended when the call returned (host {r['host_ms']:.3f} ms)"
    assert r["outputs"] and all(r["outputs"]), f"outputs differ from the default-stream run: {r['outputs']}"

"""The byte movers without a GPU (k_pil_paste of csrc/vrg_farface.hip, k_ff_composite of csrc/vrg_facefix.hip): the geometry sweep of
far_face_support.MOVER_CASES really reaches every class of 16-byte piece the kernels distinguish (a model of the geometry, no kernel is
called), and the expected bytes of the sweep are right at these sizes: every box through the headers compiled for the host, the numpy
restatements and, where Pillow is importable, Image.paste itself.  The host side of what the two kernels share (csrc/vrg_byte_mover.hpp,
csrc/vrg_common.hpp) is called here through tests/host_math/farface_check.cpp: the hit test against far_face_support.piece_hits, span_fits
at its edges and the chunked launcher.  tests/test_gpu_byte_movers.py runs the sweep on the GPU."""
import numpy as np
import pytest

import facefix_builder_support as FS
import far_face_support as S
import lanczos_support as LS


@pytest.fixture(scope="module")
def pieces():
    return [p for name in S.MOVER_CASES for p in S.classify_pieces(name)]


@pytest.fixture(scope="module")
def hm_far(tmp_path_factory):
    return S.build_host_lib(tmp_path_factory.mktemp("farface_check"))


@pytest.fixture(scope="module")
def hm_ff(tmp_path_factory):
    return FS.build_host_lib(tmp_path_factory.mktemp("facefix_check"))


def test_the_list_holds_the_stated_cases():
    C = S.MOVER_CASES
    assert C["a_1x1"][:3] == (5, 1, 1) and [b is not None for b in C["a_1x1"][3]] == [True, False, True, False, True]
    assert C["b_7x5"][:3] == (3, 7, 5) and C["b_7x5"][3] == [(0, 0, 5, 7), (4, 6, 5, 7), None] and (3 * 7 * 5 * 3) % 16 == 11
    assert C["c_corners"][:3] == C["c_lines"][:3] == (3, 9, 11)
    corners = C["c_corners"][3] + C["c_lines"][3][:1]
    assert sorted((b[0] == 0, b[1] == 0, b[2] == 11, b[3] == 9) for b in corners) == \
        sorted([(True, True, False, False), (False, True, True, False), (True, False, False, True), (False, False, True, True)])
    assert (10, 0, 11, 9) in C["c_lines"][3] and (0, 8, 11, 9) in C["c_lines"][3]
    lefts = []
    for k in (0, 4, 8, 12):
        F, H, W, boxes = C[f"d_left{k}"]
        assert (F, H, W) == (4, 33, 37) and all((b[2] - b[0], b[3] - b[1]) == (6, 5) and b[1] > 0 and b[3] < H and b[2] < W for b in boxes)
        lefts += [b[0] for b in boxes]
    assert sorted(lefts) == list(range(16))
    F, H, W, boxes = C["d_47x45"]
    sizes = [(b[2] - b[0], b[3] - b[1]) for b in boxes if b is not None]
    assert (F, H, W) == (3, 64, 48) and sizes == [(47, 45), (1, 40)] and 47 * 45 > 2048 and (47 * 45) % 2048 != 0
    assert C["e_96x128"][:3] == (2, 96, 128) and (96 * 128 * 3) % 16 == 0 and (128 * 3) % 16 == 0
    for F, H, W, boxes in C.values():
        assert len(boxes) == F and all(b is None or (0 <= b[0] < b[2] <= W and 0 <= b[1] < b[3] <= H) for b in boxes)


def test_every_class_of_piece_is_reached(pieces):
    def some(rule):
        return sum(1 for p in pieces if rule(p))

    counts = {
        "crosses one seam": some(lambda p: p["seams"] == 1),
        "crosses several seams": some(lambda p: p["seams"] > 1),
        "the batch's tail": some(lambda p: p["tail"]),
        "a tail that is no seam": some(lambda p: p["tail"] and p["seams"] == 0),
        "enters a frame whose box it touches": some(lambda p: p["seams"] and p["later_box_touched"]),
        "enters a frame without a box": some(lambda p: p["seams"] and p["later_frame_without_box"]),
        "enters a frame whose box it misses": some(lambda p: p["seams"] and not p["later_box_touched"] and not p["later_frame_without_box"]),
        "in one row, hits": some(lambda p: p["rows"] == 1 and p["asked"] is True),
        "in one row, misses": some(lambda p: p["rows"] == 1 and p["asked"] is False),
        "in several rows, hits": some(lambda p: (p["rows"] or 0) > 1 and p["asked"] is True and p["touches"]),
        "in several rows, above the box": some(lambda p: (p["rows"] or 0) > 1 and p["asked"] is False and
                                               p["y1"] < S.MOVER_CASES[p["case"]][3][p["frame"]][1]),
        "in several rows, below the box": some(lambda p: (p["rows"] or 0) > 1 and p["asked"] is False and
                                               p["y0"] >= S.MOVER_CASES[p["case"]][3][p["frame"]][3]),
        "in a frame without a box": some(lambda p: not p["walk"] and p["asked"] is None),
        "ends one byte before the box": some(lambda p: p["ends_before"]),
        "starts one byte after the box": some(lambda p: p["starts_after"]),
        "touches the first column": some(lambda p: p["first_col"]),
        "touches the last column": some(lambda p: p["last_col"]),
        "touches the first column only": some(lambda p: p["first_col"] and not p["last_col"]),
        "touches the last column only": some(lambda p: p["last_col"] and not p["first_col"]),
        "rebuilt although no byte is in the box": some(lambda p: p["asked"] is True and not p["touches"]),
    }
    print(counts)
    assert all(counts.values()), [k for k, v in counts.items() if not v]
    # a piece one byte short of / one byte past the box is not rebuilt, and no piece with a byte in the box is ever passed over
    assert all(p["asked"] is False for p in pieces if p["ends_before"] or p["starts_after"])
    assert not any(p["touches"] and p["asked"] is False for p in pieces)
    offsets = sorted({o for name in S.MOVER_CASES for o in S.box_first_byte_offsets(name)})
    assert offsets == list(range(16))
    # the control has none of it: that is why the older tests saw none of it
    control = S.classify_pieces("e_96x128")
    assert not any(p["walk"] or p["tail"] or p["seams"] or (p["rows"] or 1) > 1 for p in control)


def test_the_sweep_has_boxes_on_both_sides_of_the_colour_match_threshold():
    """16 selected pixels: below it a box comes back unmatched, from it on matched -- both kernels meet both in the sweep"""
    far = [int((m >= 64).sum()) for name in S.MOVER_CASES for m in S.mover_inputs(name)[2]]
    builder = [int((FS.soft_ellipse_mask(b[2] - b[0], b[3] - b[1], feather) > np.float32(0.35)).sum())
               for name in S.MOVER_CASES for b in S.MOVER_CASES[name][3] if b is not None for feather in (0, 1)]
    for counts in (far, builder):
        assert min(counts) < 16 <= max(counts) and sum(c >= 16 for c in counts) >= 2, counts


@pytest.mark.parametrize("name", sorted(S.MOVER_CASES))
def test_far_face_boxes_on_the_host_equal_the_restatement_and_pillow(hm_far, name):
    originals, repaired, masks, boxes = S.mover_inputs(name)
    want_off = S.composite(originals, repaired, boxes, -1, False, masks)
    want_on = S.composite(originals, repaired, boxes, -1, True, masks)
    k = 0
    for f, box in enumerate(boxes):
        if box is None:
            assert np.array_equal(want_off[f], originals[f]) and np.array_equal(want_on[f], originals[f])
            continue
        left, top, right, bottom = box
        target = np.ascontiguousarray(originals[f, top:bottom, left:right])
        rep, mask, k = repaired[k], masks[k], k + 1
        assert np.array_equal(S.host_paste(hm_far, target, rep, mask), want_off[f, top:bottom, left:right]), (name, f)
        stats = S.host_means(hm_far, target, rep, mask, 1)
        count = int((mask >= 64).sum())
        assert int(stats[0]) == count and int(stats[10]) == (1 if count >= 16 else 0)
        assert np.array_equal(S.host_paste(hm_far, target, rep, mask, stats), want_on[f, top:bottom, left:right]), (name, f)
        if count < 16:                                                      # too few selected: the colour match leaves the crop alone
            assert np.array_equal(want_on[f], want_off[f])
        outside = np.ones(originals[f].shape[:2], bool)
        outside[top:bottom, left:right] = False
        assert np.array_equal(want_on[f][outside], originals[f][outside])
        try:
            from PIL import Image
        except ImportError:
            continue
        frame = Image.fromarray(originals[f])
        frame.paste(Image.fromarray(rep), (left, top), Image.fromarray(mask))
        assert np.array_equal(np.asarray(frame), want_off[f]), (name, f)


@pytest.mark.parametrize("name", sorted(S.MOVER_CASES))
def test_builder_boxes_on_the_host_equal_the_restatement(hm_ff, name):
    originals, enhanced, boxes, strengths = FS.mover_inputs(name)
    for feather, cm in FS.MOVER_SETTINGS:
        want = FS.composite(originals, enhanced, boxes, strengths, feather, cm)
        k = 0
        for f, box in enumerate(boxes):
            if box is None:
                assert np.array_equal(want[f], originals[f])
                continue
            e, k = enhanced[k], k + 1
            if strengths[f] <= 0:
                assert np.array_equal(want[f], originals[f])
                continue
            left, top, right, bottom = box
            w, h = right - left, bottom - top
            mask = FS.soft_ellipse_mask(w, h, feather)
            assert np.array_equal(FS.host_mask(hm_ff, w, h, feather).view(np.uint32), mask.view(np.uint32)), (name, f, feather)
            resized = np.asarray(LS.restated(e[None], w, h))[0]
            target = np.ascontiguousarray(originals[f, top:bottom, left:right])
            got, _ = FS.host_composite(hm_ff, target, resized, mask, cm, strengths[f])
            assert np.array_equal(got, want[f, top:bottom, left:right]), (name, f, feather, cm)


def test_the_header_hit_test_equals_the_restatement(hm_far, pieces):
    """byte_piece_hits of csrc/vrg_byte_mover.hpp == far_face_support.piece_hits: every r that classify_pieces visits in a frame with a box,
    and every r in 0 .. frame_bytes - 16 of the cases of at most 37 pixels of width"""
    asked = narrow = 0
    for p in pieces:
        if p["asked"] is None:
            continue
        F, H, W, boxes = S.MOVER_CASES[p["case"]]
        left, top, right, bottom = boxes[p["frame"]]
        r = p["b0"] - p["frame"] * H * W * 3
        assert bool(hm_far.hm_byte_piece_hits(left, top, right - left, bottom - top, W, r)) == p["asked"] == \
            S.piece_hits(boxes[p["frame"]], W, r), (p["case"], p["frame"], r)
        asked += 1
    for name, (F, H, W, boxes) in S.MOVER_CASES.items():
        if W > 37:
            continue
        for box in boxes:
            if box is None:
                continue
            left, top, right, bottom = box
            for r in range(H * W * 3 - 15):
                assert bool(hm_far.hm_byte_piece_hits(left, top, right - left, bottom - top, W, r)) == S.piece_hits(box, W, r), (name, box, r)
                narrow += 1
    assert asked and narrow
    assert sorted(n for n, c in S.MOVER_CASES.items() if c[2] <= 37) == ["a_1x1", "b_7x5", "c_corners", "c_lines", "d_left0", "d_left12", "d_left4", "d_left8"]


@pytest.mark.parametrize("n", [0, 1, 32767, 32768, 32769, 32771])
def test_the_launch_chunks_tile_the_records_in_order(hm_far, n):
    chunks, calls = np.full((4, 2), -1, np.int64), np.zeros(1, np.int32)
    assert hm_far.hm_launch_chunks(n, 0, 0, chunks, 4, calls) == 0
    k = int(calls[0])
    assert k == (n + 32767) // 32768
    first, count = chunks[:k, 0], chunks[:k, 1]
    assert (count >= 1).all() and (count <= 32768).all() and int(count.sum()) == n
    assert list(first) == [int(count[:i].sum()) for i in range(k)]             # each chunk starts where the one before it ended, from 0


def test_a_failing_launch_stops_the_chunks_and_returns_its_code(hm_far):
    chunks, calls = np.full((4, 2), -1, np.int64), np.zeros(1, np.int32)
    assert hm_far.hm_launch_chunks(3 * 32768 + 5, 2, 3, chunks, 4, calls) == 3
    assert int(calls[0]) == 2 and chunks.tolist() == [[0, 32768], [32768, 32768], [-1, -1], [-1, -1]]
    assert hm_far.hm_launch_chunks(32771, 1, 2, chunks, 4, calls) == 2 and int(calls[0]) == 1


@pytest.mark.parametrize("align", [1, 2, 3, 5, 7, 32768])
def test_the_aligned_launch_chunks_tile_the_records_and_start_on_the_alignment(hm_far, align):
    """Records that share state in groups of `align` (f % ref_frames, the frames of one Philox chunk): every launch starts on a group."""
    for n in (0, 1, align, 32768, 32769, 3 * 32768 + 5):
        chunks, calls = np.full((8, 2), -1, np.int64), np.zeros(1, np.int32)
        assert hm_far.hm_launch_chunks_aligned(n, align, chunks, 8, calls) == 0, n
        k = int(calls[0])
        step = 32768 - 32768 % align
        assert k == (0 if n == 0 else 1 if n <= 32768 else -(-n // step)) and k <= 8, n
        first, count = chunks[:k, 0], chunks[:k, 1]
        assert (count >= 1).all() and (count <= 32768).all() and int(count.sum()) == n, n
        assert list(first) == [int(count[:i].sum()) for i in range(k)], n           # in order, from 0, nothing left out or done twice
        assert not (first % align).any(), n
        assert (chunks[k:] == -1).all(), n


def test_an_alignment_no_launch_can_hold_is_refused_past_one_launch(hm_far):
    chunks, calls = np.full((4, 2), -1, np.int64), np.zeros(1, np.int32)
    for n in (32769, 32771, 2 * 32769):
        assert hm_far.hm_launch_chunks_aligned(n, 32769, chunks, 4, calls) == 2 and int(calls[0]) == 0, n      # VRG_ERR_UNSUPPORTED, nothing launched
    for n in (1, 32767, 32768):
        assert hm_far.hm_launch_chunks_aligned(n, 32769, chunks, 4, calls) == 0 and int(calls[0]) == 1, n
        assert chunks[0].tolist() == [0, n]
    assert hm_far.hm_launch_chunks_aligned(0, 32769, chunks, 4, calls) == 0 and int(calls[0]) == 0
    assert hm_far.hm_launch_chunks_aligned(5, 0, chunks, 4, calls) == 1 and int(calls[0]) == 0                  # VRG_ERR_BAD_ARG


def test_the_alignment_of_two_is_their_least_common_multiple(hm_far):
    import math
    for a in (1, 2, 3, 4, 6, 7, 32768, 2**31 - 1):
        for b in (1, 2, 3, 5, 6, 9, 32767, 2**31 - 1):
            assert hm_far.hm_chunk_lcm(a, b) == math.lcm(a, b), (a, b)


def test_span_fits_at_its_edges(hm_far):
    fits = lambda offset, need, size: bool(hm_far.hm_span_fits(offset, need, size))
    size = 100
    assert fits(size, 0, size)                                                  # an empty span may start at the end
    assert not fits(size, 1, size)
    for offset in (0, 1, 37, size - 1):
        assert fits(offset, size - offset, size) and not fits(offset, size - offset + 1, size)
    assert not fits(-1, 0, size) and not fits(-1, 1, size)
    assert not fits(size + 1, 0, size) and not fits(size + 1, -1, size)         # past the end, whatever the need
    assert fits(0, 0, 0) and not fits(0, 1, 0)
    big = 2 ** 63 - 1
    assert fits(0, big, big) and not fits(1, big, big) and not fits(-big, 1, big)

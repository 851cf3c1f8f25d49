"""The shot-aware cut score on the MI355X: vrg_cut_thumbs_f32, vrg_cut_hist_u8 and vrg_cut_pair_sums against the numpy restatement of
tests/cut_support.py (itself equal to the host-compiled header, tests/test_cut_host.py) bit for bit -- device-resident and host-fed
frames, three and four channels, offset base pointers, batches cut into pieces -- and shot_cut_scores / shot_boundaries against the host
arithmetic and the reference's recorded flags (tests/golden/cut_score.json)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import cut_support as CS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def FF(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes
    return VRGDG_StandaloneFaceFixNodes


@pytest.fixture(scope="module")
def golden():
    with open(CS.golden_path()) as fh:
        return json.load(fh)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def device_sums(ops, xd):
    t = ops.cut_thumbnails(xd)
    h = ops.cut_histograms(t)
    s = ops.cut_pair_sums(t, h)
    assert t.dtype == torch.uint8 and h.dtype == torch.int32 and s.dtype == torch.int64
    return t.cpu().numpy(), h.cpu().numpy(), s.cpu().numpy()


def report(name, got, want):
    worst, share = CS.differences(got[0], want[0])
    bins, sums = int((got[1] != want[1]).sum()), int((got[2] != want[2]).sum())
    print(f"{name}: thumbnails: largest difference {worst} levels, {share:.4%} of the bytes differ; {bins} histogram bins and {sums} sums differ")
    return worst == 0 and bins == 0 and sums == 0 and all(g.shape == w.shape for g, w in zip(got, want))


@pytest.mark.parametrize("kind", ("uniform", "smooth", "special"))
@pytest.mark.parametrize("size", CS.SIZES + CS.SEGMENTED_SIZES)
def test_device_frames_equal_the_restatement(ops, size, kind):
    h, w, c = size
    assert (CS.cells_per_segment(w, c) < 64) == (size in CS.SEGMENTED_SIZES)           # the segmented sizes, and they alone, take that path
    n = 1 if size in CS.SEGMENTED_SIZES else (3 if h * w <= 1500 * 2500 else 2)
    x = CS.FRAME_KINDS[kind]((n, h, w, c), 500 + h + w)
    xd = torch.from_numpy(x).to(dev())
    got = device_sums(ops, xd)
    assert report(f"{size} {kind}", got, CS.restated_sums(x))
    assert np.array_equal(xd.cpu().numpy(), x)


@pytest.mark.parametrize("size", ((480, 854, 3), (65, 67, 3), (96, 130, 4), (128, 128, 3), (720, 1280, 3)))
def test_host_fed_frames_equal_the_restatement(ops, FF, size, monkeypatch):
    from comfyui_vrgamedevgirl_amd import _devices
    h, w, c = size
    x = CS.smooth_frames((7, h, w, c), 600 + h)
    cpu = torch.from_numpy(x.copy())
    want = CS.restated_sums(x)
    monkeypatch.setattr(_devices, "PIPE_BYTES", 2 * h * w * c * 4)                     # pieces of two frames: 2 + 2 + 2 + 1
    for frames in (cpu, cpu.pin_memory()):
        t = ops.cut_thumbnails_host(frames)
        assert t.is_cuda and tuple(t.shape) == (7, 64, 64, 3)
        h_ = ops.cut_histograms(t)
        got = (t.cpu().numpy(), h_.cpu().numpy(), ops.cut_pair_sums(t, h_).cpu().numpy())
        assert report(f"{size} host-fed", got, want)
        assert np.array_equal(frames.numpy(), x)
    scores = FF.shot_cut_scores(cpu)
    assert scores.dtype == np.float64 and np.array_equal(scores, FF.cut_scores_from_sums(want[2])) and np.array_equal(cpu.numpy(), x)


@pytest.mark.parametrize("channels", (3, 4))
@pytest.mark.parametrize("offset_floats", (1, 2, 3))
def test_offset_base_pointers(ops, pkg, channels, offset_floats):
    """frames that start 4, 8 and 12 bytes off the 16-byte grid, thumbnails that start 3 bytes off the dword grid: same bytes"""
    from comfyui_vrgamedevgirl_amd import _hip
    x = CS.uniform_frames((2, 70, 131, channels), 40 + offset_floats)
    want = CS.thumbnails(x)
    src = torch.zeros(x.size + 8, dtype=torch.float32, device=dev())
    src[offset_floats:offset_floats + x.size] = torch.from_numpy(x.reshape(-1)).to(dev())
    dst = torch.full((want.size + 8,), 0xAB, dtype=torch.uint8, device=dev())
    taps = torch.from_numpy(ops.area_taps(70, 131).view(np.uint8).copy()).to(dev())
    st = _hip.lib().vrg_cut_thumbs_f32(C.c_void_p(src.data_ptr() + 4 * offset_floats), C.c_void_p(dst.data_ptr() + 3), 2, 70, 131, channels, _hip.ptr(taps),
                                       _hip.current_stream())
    assert st == _hip.VRG_OK
    out = dst.cpu().numpy()
    worst, share = CS.differences(out[3:3 + want.size].reshape(want.shape), want)
    print(f"C = {channels}, {offset_floats} floats off: largest difference {worst} levels, {share:.4%} of the bytes differ")
    assert worst == 0 and (out[:3] == 0xAB).all() and (out[3 + want.size:] == 0xAB).all()
    assert np.array_equal(src.cpu().numpy()[offset_floats:offset_floats + x.size], x.reshape(-1))
    # a view into a larger batch: frames 1 .. 2 of three
    y = CS.smooth_frames((3, 64, 200, channels), 9)
    yd = torch.from_numpy(y).to(dev())
    assert np.array_equal(ops.cut_thumbnails(yd[1:]).cpu().numpy(), CS.thumbnails(y[1:]))


def test_scores_equal_the_host_scores_and_flags_match_the_golden_cases(ops, FF, golden):
    for case in golden["cases"]:
        x = CS.make_video(case["kind"], case["shape"], case["seed"])
        want = FF.cut_scores_from_sums(np.asarray(case["sums"], dtype=np.int64).reshape(-1, 4))
        for frames in (torch.from_numpy(x.copy()).to(dev()), torch.from_numpy(x.copy())):
            scores = FF.shot_cut_scores(frames)
            worst = float(np.abs(scores - np.asarray(case["scores"])).max())
            print(f"{case['key']} ({frames.device.type}): |score - reference| <= {worst:.3e}")
            assert scores.dtype == np.float64 and scores[0] == 0.0 and np.array_equal(scores, want), case["key"]
            assert worst <= golden["bound"]
            for t in case["thresholds"]:
                assert FF.shot_boundaries(frames, t["cut_sensitivity"]) == (t["hard_cut"], t["shot_id"]), (case["key"], t["cut_sensitivity"])
            assert np.array_equal(frames.cpu().numpy(), x)


def test_a_batch_in_pieces_gives_the_same_integers(ops, FF):
    """48 frames of 1080p whole, and the same frames fed in pieces of 5: thumbnails per piece, the pair pass over all of them"""
    scenes = [CS.smooth_frames((1, 1080, 1920, 3), 70 + k)[0] for k in range(4)]
    rng = np.random.Generator(np.random.PCG64(5))
    x = np.stack([np.roll(scenes[f // 12], 7 * f, axis=1) + rng.normal(0.0, 0.01, (1080, 1920, 3)).astype(np.float32) for f in range(48)])
    xd = torch.from_numpy(x).to(dev())
    keep = xd.clone()
    whole = device_sums(ops, xd)
    pieces = torch.cat([ops.cut_thumbnails(xd[s:s + 5]) for s in range(0, 48, 5)])
    hist = ops.cut_histograms(pieces)
    in_pieces = (pieces.cpu().numpy(), hist.cpu().numpy(), ops.cut_pair_sums(pieces, hist).cpu().numpy())
    assert report("48 x 1080p, whole against pieces of 5", in_pieces, whole)
    assert torch.equal(xd, keep)                                                       # video_frames is unchanged
    scores = FF.shot_cut_scores(xd)
    assert np.array_equal(scores, FF.cut_scores_from_sums(whole[2])) and torch.equal(xd, keep)
    want = CS.restated_sums(x)
    assert report("48 x 1080p against the restatement", whole, want)
    for sensitivity in (0.28, 0.05):
        assert FF.shot_boundaries(xd, sensitivity) == FF.boundaries_from_scores(FF.cut_scores_from_sums(want[2]), sensitivity)
    print("scores at the scene changes:", [round(float(scores[i]), 4) for i in (12, 24, 36)], "largest elsewhere:",
          round(float(np.delete(scores, [12, 24, 36]).max()), 4))
    assert torch.equal(xd, keep)


def test_degenerate_batches(ops, FF):
    one = torch.from_numpy(CS.uniform_frames((1, 64, 64, 3), 1)).to(dev())
    assert FF.shot_cut_scores(one).tolist() == [0.0] and FF.shot_boundaries(one, 0.28) == ([False], [0])
    assert tuple(ops.cut_pair_sums(ops.cut_thumbnails(one)).shape) == (0, 4)
    assert tuple(ops.cut_thumbnails(one[:0]).shape) == (0, 64, 64, 3)
    with pytest.raises(ValueError, match="below 64 px"):
        ops.cut_thumbnails(torch.zeros(1, 63, 64, 3, device=dev()))
    with pytest.raises(ValueError):
        ops.cut_thumbnails(torch.zeros(1, 64, 64, 3, device=dev(), dtype=torch.float16))
    half = torch.from_numpy(CS.uniform_frames((3, 64, 96, 3), 2)).to(dev())
    assert np.array_equal(FF.shot_cut_scores(half.half()), FF.shot_cut_scores(half.half().float()))     # other dtypes are converted, as .float() would

"""The Video Compare Slider's byte hand-off on the MI355X: vrg_rgb24_frames_u8 byte for byte against numpy running the reference's
expression on the downloaded input (NaN as 0), every geometry at which the flat run of 16-byte pieces takes another path, the overlap
and stream contracts, and ops.stream_rgb24 from a CUDA batch, a CPU batch and a pending result of one of the pack's nodes.  The launch
is never chunked (one grid takes about 2^43 bytes), so there is no chunk seam to cross.  Nothing here provokes a fault: the raising sink
is a Python exception on the host."""
import importlib
import os

import numpy as np
import pytest
import torch

import compare_support as S
import overlap_support as O
import stream_support as T
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

GUARD_U8 = 0x5A
GEOMETRY = ((1, 1, 1, 3), (1, 1, 5, 3), (1, 2, 8, 3), (5, 1, 3, 3), (2, 3, 7, 3), (3, 5, 11, 4))
STREAMED = (7, 6, 10, 3)
PIECE_BYTES = 3 * 6 * 10 * 3 + 17                  # three frames of 180 bytes and a bit: 3 + 3 + 1


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def streamed():
    """the seven frames of the hand-off tests and their bytes: computed once, never changed"""
    x = S.batch(STREAMED, 70)
    want = S.expected(x)
    for a in (x, want):
        a.setflags(write=False)
    return x, want


def _run(ops, dev, x, shift_in=0, shift_out=0):
    """x through ops.rgb24_frames with the input `shift_in` floats and the output `shift_out` bytes off the 16-byte grid, into a guarded out"""
    raw_in = torch.zeros(x.size + 8, dtype=torch.float32, device=dev)
    src = raw_in[shift_in:shift_in + x.size].view(x.shape)
    src.copy_(torch.from_numpy(x))
    count = x.size // x.shape[3] * 3
    raw = torch.full((count + 64,), GUARD_U8, dtype=torch.uint8, device=dev)
    out = raw[16 + shift_out:16 + shift_out + count].view(*x.shape[:3], 3)
    assert src.data_ptr() % 16 == 4 * (shift_in % 4) and out.data_ptr() % 16 == shift_out % 16
    assert ops.rgb24_frames(src, out=out) is out
    assert bool((raw[:16 + shift_out] == GUARD_U8).all()) and bool((raw[16 + shift_out + count:] == GUARD_U8).all())
    assert torch.equal(src.cpu(), torch.from_numpy(x)) or np.isnan(x).any()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", (3, 4))
def test_the_sweep_and_a_poisoned_alpha(ops, dev, channels):
    """every k / 255 with its neighbours, the ties, the clip's ends, -0.0, a subnormal, the infinities and NaN, as [1, 16, 64, C]; with four
    channels the alpha is NaN everywhere and must not leak"""
    x = S.sweep_batch(channels)
    assert x.shape == (1, 16, 64, channels) and np.isnan(x[..., :3]).any() and np.isinf(x).any()
    want = S.expected(x)
    got = ops.rgb24_frames(torch.from_numpy(x).to(dev))
    assert got.dtype == torch.uint8 and got.device == dev and tuple(got.shape) == (1, 16, 64, 3)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), [(float(v), int(g), int(w)) for v, g, w in zip(x[..., :3].ravel(), got.ravel(), want.ravel()) if g != w][:8]
    for shift_in, shift_out in ((1, 7), (2, 0)):
        assert np.array_equal(_run(ops, dev, x, shift_in, shift_out), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GEOMETRY, ids=["x".join(map(str, s)) for s in GEOMETRY])
def test_geometry_at_every_output_offset(ops, dev, shape):
    """3 bytes; 15, one short of a piece; exactly 48; 9-byte frames (seams inside pieces); ragged tails with three and four channels --
    with `out` a byte view whose first byte lies at each of the 16 offsets within a 16-byte piece, and the source on and off the grid"""
    x = S.batch(shape, sum(shape))
    want = S.expected(x)
    assert want.size == int(np.prod(shape[:3])) * 3
    for shift_out in range(16):
        assert np.array_equal(_run(ops, dev, x, shift_out % 4, shift_out), want), shift_out
    fresh = ops.rgb24_frames(torch.from_numpy(x).to(dev))
    assert np.array_equal(fresh.cpu().numpy(), want)
    if shape[0] == 1:                                                                   # [H, W, C]: one frame
        assert np.array_equal(ops.rgb24_frames(torch.from_numpy(x[0]).to(dev)).cpu().numpy(), want)


@pytest.mark.parametrize("channels", (3, 5))
def test_frame_slices_off_the_source_grid(ops, dev, channels):
    """frames of 9 (C = 3) or 15 (C = 5) floats, 36 or 60 bytes: the slice from frame i on begins 4, 8 and 12 bytes off the 16-byte
    grid (with four channels a frame is whole 16-byte pieces; such a source goes off the grid in the tests above)"""
    shape = (5, 1, 3, channels)
    x = S.batch(shape, 40 + channels)
    whole = torch.from_numpy(x).to(dev)
    assert whole.data_ptr() % 16 == 0
    seen = set()
    for first in range(1, 5):
        piece = whole[first:]
        seen.add(piece.data_ptr() % 16)
        assert piece.is_contiguous() and np.array_equal(ops.rgb24_frames(piece).cpu().numpy(), S.expected(x[first:])), first
    assert {4, 8, 12} <= seen


# ---------------------------------------------------------------------------------------------------------------------------------
# contracts
# ---------------------------------------------------------------------------------------------------------------------------------
def test_out_overlapping_the_input_is_refused_and_touching_is_not(ops, dev):
    """the arrangements of tests/overlap_support.py: refused before anything is launched (every byte unchanged), accepted back to back"""
    x = S.batch((2, 9, 11, 4), 33)
    want = S.expected(x)
    r_shape, w_shape = x.shape, want.shape
    r_bytes, w_bytes = O.nbytes_of(r_shape, torch.float32), O.nbytes_of(w_shape, torch.uint8)
    tried = set()
    for arrangement, (refused, what) in O.ARRANGEMENTS.items():
        offset = O.placement(arrangement, w_bytes, 1, r_bytes)
        if offset is None:
            continue
        base = O.GUARD + (w_bytes + 15) // 16 * 16
        buffer = O.sentinel(base + r_bytes + w_bytes + O.GUARD + 16, dev)
        images, out = O.carve(buffer, base, r_shape, torch.float32), O.carve(buffer, base + offset, w_shape, torch.uint8)
        assert O.overlap_truth(offset, w_bytes, r_bytes) == refused
        if refused:
            torch.cuda.synchronize()
            before = buffer.clone()
            with pytest.raises(ValueError, match=r"^rgb24_frames: out must not alias images"):
                ops.rgb24_frames(images, out=out)
            torch.cuda.synchronize()
            assert torch.equal(buffer, before), what
        else:
            images.copy_(torch.from_numpy(x))
            guards = buffer.clone()
            assert np.array_equal(ops.rgb24_frames(images, out=out).cpu().numpy(), want), what
            assert torch.equal(images.cpu(), torch.from_numpy(x))
            lo, hi = min(base, base + offset), max(base + r_bytes, base + offset + w_bytes)
            assert torch.equal(buffer[:lo], guards[:lo]) and torch.equal(buffer[hi:], guards[hi:])
        tried.add(arrangement)
    assert {"a", "b", "c", "d", "f", "g"} <= tried
    with pytest.raises(ValueError):
        ops.rgb24_frames(torch.zeros((1, 4, 4, 3), device=dev), out=torch.zeros((1, 4, 4, 4), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        ops.rgb24_frames(torch.zeros((1, 4, 4, 3), device=dev), out=torch.zeros((1, 4, 4, 3), dtype=torch.float32, device=dev))


def test_the_launch_goes_to_the_callers_stream(ops, dev):
    """the probe of tests/stream_support.py: poisoned inputs made valid behind a spin on the caller's stream, a spin on the default one"""
    torch.cuda.set_device(dev)
    spin = T.Spin()
    case = T.Case("rgb24_frames", None, ("rgb24_frames",), out=True)
    inputs = [T._rand((2, 37, 53, 4), 75, -0.1, 1.1).to(dev)]
    torch.cuda.synchronize()
    r = T.probe(ops, case, inputs, lambda inp, out: ops.rgb24_frames(inp[0], out=out), spin)
    print(f"\n[stream order] rgb24_frames: host {r['host_ms']:.3f} ms, armed early {r['armed_early']} late {r['armed_late']}")
    assert r["armed_late"] and r["armed_early"], r
    assert r["outputs"] and all(r["outputs"]) and all(r["inputs_kept"]), r


# ---------------------------------------------------------------------------------------------------------------------------------
# the hand-off
# ---------------------------------------------------------------------------------------------------------------------------------
def _collector():
    chunks = []

    def sink(view):
        assert isinstance(view, memoryview) and view.format == "B" and view.ndim == 1
        chunks.append(bytes(view))                     # the memory is the sink's only until it returns
    return chunks, sink


def _check_pieces(chunks, want):
    assert [len(c) for c in chunks] == [540, 540, 180]
    assert b"".join(chunks) == want.tobytes()


@pytest.mark.parametrize("where", ("cuda", "cpu", "cpu-pageable-buffers"))
def test_stream_rgb24_hands_over_the_one_launch_result_in_order(ops, dev, streamed, monkeypatch, where):
    x, want = streamed
    if where == "cpu-pageable-buffers":                # a host that refuses to page-lock
        monkeypatch.setattr(ops.Rgb24Handoff, "_host_buffer", staticmethod(lambda nbytes: torch.empty((nbytes,), dtype=torch.uint8)))
    images = torch.from_numpy(x.copy())
    images = images.to(dev) if where == "cuda" else images
    assert np.array_equal(ops.rgb24_frames(torch.from_numpy(x.copy()).to(dev)).cpu().numpy(), want)
    chunks, sink = _collector()
    assert ops.stream_rgb24(images, sink, piece_bytes=PIECE_BYTES) == 7
    _check_pieces(chunks, want)
    assert torch.equal(images.cpu(), torch.from_numpy(x.copy()))
    chunks, sink = _collector()
    assert ops.stream_rgb24(images, sink, piece_bytes=1 << 20) == 7 and [len(c) for c in chunks] == [1260]
    chunks, sink = _collector()
    assert ops.stream_rgb24(images[2], sink, piece_bytes=PIECE_BYTES) == 1 and b"".join(chunks) == want[2].tobytes()     # [H, W, C]


def test_stream_rgb24_reads_a_pending_result_in_hbm(ops, dev, monkeypatch):
    """a pending LazyFrames made by one of the pack's own nodes: the bytes of its frames, which never come to the host as fp32"""
    from comfyui_vrgamedevgirl_amd import nodes, _devices as D
    monkeypatch.setattr(D, "LAZY_SECONDS", 60.0)
    monkeypatch.setattr(D, "DEFER_GRAPH", True)
    monkeypatch.setattr(D, "LAZY_DOWNLOAD", True)
    D._DEVICE_COPIES.clear()
    try:
        x = torch.from_numpy(S.batch(STREAMED, 71)).clamp(0, 1)
        t = nodes.FastUnsharpSharpen().apply_unsharp(x, 0.6, False)[0]
        assert isinstance(t, D.LazyFrames) and D.pending_of(t) is not None and t.device.type == "cpu"
        skipped = D._LAZY.downloads_skipped
        chunks, sink = _collector()
        assert ops.stream_rgb24(t, sink, piece_bytes=PIECE_BYTES) == 7
        assert D.pending_of(t) is not None and D._LAZY.downloads_skipped > skipped
        want = S.expected(t.numpy())                   # the first host use: downloaded now
        assert D.pending_of(t) is None and not np.array_equal(want, S.expected(x.numpy()))
        _check_pieces(chunks, want)
    finally:
        torch.cuda.synchronize()
        D._DEVICE_COPIES.clear()


@pytest.mark.parametrize("where", ("cuda", "cpu"))
def test_a_sink_that_raises_stops_the_hand_off(ops, dev, streamed, where):
    x, want = streamed
    images = torch.from_numpy(x.copy())
    images = images.to(dev) if where == "cuda" else images
    boom, calls = KeyError("the pipe is gone"), []

    def sink(view):
        calls.append(bytes(view))
        if len(calls) == 2:
            raise boom
    with pytest.raises(KeyError) as caught:
        ops.stream_rgb24(images, sink, piece_bytes=PIECE_BYTES)
    assert caught.value is boom and len(calls) == 2 and b"".join(calls) == want[:6].tobytes()
    assert np.array_equal(ops.rgb24_frames(torch.from_numpy(x.copy()).to(dev)).cpu().numpy(), want)      # the stream is as usable as before
    chunks, sink = _collector()
    assert ops.stream_rgb24(images, sink, piece_bytes=PIECE_BYTES) == 7
    _check_pieces(chunks, want)


def test_the_node_end_to_end_over_a_collecting_writer(ops, dev, streamed, tmp_path, monkeypatch):
    """compare() with a device-resident *after* batch and a CPU *before* batch: each writer receives its batch's bytes"""
    node = importlib.import_module(PKG_NAME + ".VRGDG_VideoCompareNode")
    x, want = streamed
    written = []

    class Writer:
        def __init__(self, path, width, height, fps):
            self.path, self.args, self.chunks = path, (width, height, fps), []
            written.append(self)

        def write(self, buffer):
            self.chunks.append(bytes(buffer))

        def close(self):
            pass

    monkeypatch.setattr(node, "folder_paths", lambda: S.Folders(tmp_path))
    monkeypatch.setattr(node, "video_writer", Writer)
    before, after = torch.from_numpy(x[:3].copy()), torch.from_numpy(x.copy()).to(dev)
    got = node.VRGDG_VideoCompareSlider().compare(0.5, "Before", "After", True, True, True, 5.0, before_images=before, after_images=after)
    assert [w.args for w in written] == [(10, 6, 24.0), (10, 6, 24.0)]
    assert b"".join(written[0].chunks) == want[:3].tobytes() and b"".join(written[1].chunks) == want.tobytes()
    assert got["result"] == ((True, [written[0].path]), (True, [written[1].path])) and os.path.isdir(os.path.join(str(tmp_path), "temp"))

"""The anchor round trip on the MI355X: vrg_anchor_frames_f32 bit for bit against live Pillow + numpy, vrg_anchor_store_u8 byte for byte
against live numpy, and the five nodes end to end over a temporary folder against the fixture recorded from the reference's classes.
Small shapes: every route of the kernels (copy, width only, height only, both, several LDS chunks, ragged tiles, both store orders, the
16-byte grid and off it), a record count past one launch chunk, frame seams inside 16-byte pieces.  Nothing here provokes a fault: bad
records are refused on the host (tests/test_anchor_host.py)."""
import importlib
import os

import numpy as np
import pytest
import torch

import anchor_support as S
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

GUARD, GUARD_U8 = 7.25, 0x5A


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def geometry():
    """the pictures of the issue's geometry list and what live Pillow + numpy make of them: computed once, never changed"""
    pictures = S.load_pictures(S.FIRST, 1 + len(S.OTHERS), seed=3)
    want = S.load_expected(pictures)
    want.setflags(write=False)
    return pictures, want


def test_load_geometry_host_fed_and_device_resident(ops, dev, geometry):
    pictures, want = geometry
    got = ops.anchor_frames(pictures)
    assert got.device == dev and got.dtype == torch.float32 and S.same_bits(got.cpu().numpy(), want) == 0
    on_device = [torch.from_numpy(p).to(dev) for p in pictures]
    keep = [p.clone() for p in on_device]
    assert S.same_bits(ops.anchor_frames(on_device).cpu().numpy(), want) == 0
    assert all(torch.equal(a, b) for a, b in zip(on_device, keep))
    mixed = [p if i % 2 else torch.from_numpy(p).to(dev) for i, p in enumerate(pictures)]
    assert S.same_bits(ops.anchor_frames(mixed).cpu().numpy(), want) == 0


@pytest.mark.parametrize("first", S.FIRSTS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("n", S.BATCHES)
def test_load_first_pictures_batches_and_float_offsets(ops, dev, first, n):
    """first pictures of 1 x 1, 13 x 5 (rows off the 16-byte grid), 64 x 64 and 70 x 20; N of 1, 2 and 7; `out` at each of the four float
    offsets within a 16-byte piece, the floats around it untouched"""
    pictures = S.load_pictures(first, n, seed=n)
    want = S.load_expected(pictures)
    values = want.size
    for shift in range(4):
        raw = torch.full((values + 8,), GUARD, dtype=torch.float32, device=dev)
        out = raw[shift:shift + values].view(want.shape)
        assert out.data_ptr() % 16 == 4 * shift
        assert ops.anchor_frames(pictures, out=out) is out
        assert S.same_bits(out.cpu().numpy(), want) == 0, shift
        assert bool((raw[:shift] == GUARD).all()) and bool((raw[shift + values:] == GUARD).all())


def test_load_past_one_launch(ops, dev):
    """32768 + 3 records of 1 x 1 pictures: the second launch takes its records and its frames where the first stopped"""
    n = S.LAUNCH_RECORDS + 3
    values = np.random.default_rng(12).integers(0, 256, (n, 1, 1, 3), dtype=np.uint8)          # no period: record 32768 is not record 0
    got = ops.anchor_frames(list(torch.from_numpy(values).to(dev)))
    want = values.astype(np.float32) / 255.0
    assert tuple(got.shape) == (n, 1, 1, 3) and S.same_bits(got.cpu().numpy(), want) == 0
    assert not np.array_equal(want[S.LAUNCH_RECORDS:], want[:3])


def test_load_a_given_size_and_several_chunks(ops, dev):
    pictures = [S.picture(4, (7, 333)), S.picture(5, (97, 61))]
    assert S.same_bits(ops.anchor_frames(pictures, size=S.FIRST).cpu().numpy(), S.load_expected(pictures, S.FIRST)) == 0


def test_load_refuses_on_the_host(ops, dev):
    with pytest.raises(ValueError):
        ops.anchor_frames([])
    with pytest.raises(ValueError):
        ops.anchor_frames([np.zeros((4, 4, 4), dtype=np.uint8)])
    with pytest.raises(ValueError):
        ops.anchor_frames([S.picture(1, (4, 4))], out=torch.empty((1, 4, 4, 3), dtype=torch.float16, device=dev))
    desc, tables, src_bytes, (h, w) = ops.anchor_plan([(24, 40), (61, 97)])
    with pytest.raises(ValueError):
        ops.anchor_check(desc, tables, src_bytes - 1, h, w)


def _store(ops, dev, x, bgr, shift_in, shift_out):
    """x through ops.anchor_store_bytes with input and output `shift` elements off the 16-byte grid, into a guarded `out`"""
    raw_in = torch.zeros(x.size + 8, dtype=torch.float32, device=dev)
    src = raw_in[shift_in:shift_in + x.size].view(x.shape)
    src.copy_(torch.from_numpy(x))
    count = x.size // x.shape[3] * 3
    raw = torch.full((count + 64,), GUARD_U8, dtype=torch.uint8, device=dev)
    out = raw[16 + shift_out:16 + shift_out + count].view(*x.shape[:3], 3)
    assert src.data_ptr() % 16 == 4 * (shift_in % 4) and out.data_ptr() % 16 == shift_out % 16
    assert ops.anchor_store_bytes(src, bgr=bgr, out=out) is out
    assert bool((raw[:16 + shift_out] == GUARD_U8).all()) and bool((raw[16 + shift_out + count:] == GUARD_U8).all())
    return out.cpu().numpy()


@pytest.mark.parametrize("channels", S.STORE_CHANNELS)
@pytest.mark.parametrize("bgr", (False, True), ids=("rgb", "bgr"))
def test_store_geometry(ops, dev, channels, bgr):
    """C of 3 and 4, H x W of 1 x 1, 5 x 13 and 24 x 40, N of 1 and 5 (195 and 2880 bytes a frame: seams inside 16-byte pieces for
    5 x 13), both orders, on the grid and off it on both sides"""
    for hw in S.STORE_SHAPES:
        for n in S.STORE_FRAMES:
            x = S.store_batch(n, hw, channels, seed=n + hw[1])
            want = S.store_expected(x, bgr)
            for shift_in, shift_out in ((0, 0), (1, 5), (3, 15), (2, 0), (0, 9)):
                assert np.array_equal(_store(ops, dev, x, bgr, shift_in, shift_out), want), (hw, n, shift_in, shift_out)
            fresh = ops.anchor_store_bytes(torch.from_numpy(x).to(dev), bgr=bgr)
            assert fresh.dtype == torch.uint8 and np.array_equal(fresh.cpu().numpy(), want)


@pytest.mark.parametrize("channels", S.STORE_CHANNELS)
@pytest.mark.parametrize("bgr", (False, True), ids=("rgb", "bgr"))
def test_store_ties_and_specials_across_a_seam(ops, dev, channels, bgr):
    x = S.seam_batch(channels)
    assert (x.shape[1] * x.shape[2] * 3) % 16 != 0 and np.isnan(x).any() and np.isinf(x).any()
    want = S.store_expected(x, bgr)
    for shift_in, shift_out in ((0, 0), (1, 7)):
        assert np.array_equal(_store(ops, dev, x, bgr, shift_in, shift_out), want)


def test_store_refuses_on_the_host(ops, dev):
    with pytest.raises(ValueError):
        ops.anchor_store_bytes(torch.zeros((0, 4, 4, 3), device=dev))
    with pytest.raises(ValueError):
        ops.anchor_store_bytes(torch.zeros((1, 4, 4, 2), device=dev))
    with pytest.raises(ValueError):
        ops.anchor_store_bytes(torch.zeros((1, 4, 4, 3), device=dev), out=torch.zeros((1, 4, 4, 4), dtype=torch.uint8, device=dev))


def test_the_five_nodes_end_to_end(ops, dev, tmp_path, monkeypatch):
    """Load (both pipelines, every recorded schedule) -> Store (both) -> Collect over a temporary folder: tensors, states, files and
    bytes equal the fixture.  Fails on the parent commit: the classes are not there."""
    from PIL import Image
    ve = importlib.import_module(PKG_NAME + ".VRGDG_VideoEnhanceNodes")
    ff = importlib.import_module(PKG_NAME + ".VRGDG_StandaloneFaceFixNodes")
    monkeypatch.setattr(ve, "_log", lambda message: None)
    monkeypatch.setattr(ff, "_log", lambda message: None)
    sources = S.write_sources(str(tmp_path / "anchor_sources"))
    context = {"anchor_sources_folder": sources, "job_id": "job_a"}
    for which, node in (("video_enhance", ve.VRGDGVideoEnhanceLoadAnchorsMetaBatch()), ("face_fix", ff.VRGDGFaceFixLoadAnchorsMetaBatch())):
        for schedule in S.FIXTURE["load"][which]["schedules"]:
            S.run_schedule(node, context, schedule, S.ARRAYS["frames"], lambda t: t.cpu().numpy())
    images, _, _, _ = ve.VRGDGVideoEnhanceLoadAnchorsMetaBatch().load(context, S.MetaBatch(7, 100), "device")
    assert images.is_cuda

    x = torch.from_numpy(S.ARRAYS["store.input"].copy())
    rec = S.FIXTURE["store"]["video_enhance"]
    job = str(tmp_path / "jobs" / "job_a")
    os.makedirs(os.path.join(job, rec["folder"]))
    for name in rec["stale"]:
        open(os.path.join(job, rec["folder"], name), "wb").close()
    ctx_in = {k: (job if k == "job_folder" else rec["context_in"][k]) for k in rec["context_keys"] if k != "enhanced_anchor_folder"}
    for batch in (x, x.to(dev)):
        folder, joined, count, ctx = ve.VRGDGVideoEnhanceStoreAnchors().store(batch, ctx_in)
        assert sorted(os.listdir(folder)) == rec["files_after"] and (joined, count) == (rec["indices"], rec["count"])
        got = np.stack([np.asarray(Image.open(os.path.join(folder, n)).convert("RGB")) for n in rec["files_after"] if n.endswith(".png")])
        assert np.array_equal(got, S.ARRAYS["store.video_enhance.png"])
    assert list(ctx) == rec["context_keys"] and ctx["enhanced_anchor_folder"] == folder

    rec = S.FIXTURE["store"]["face_fix"]
    out_dir = tmp_path / "output"
    os.makedirs(out_dir / rec["folder"])
    for name in rec["stale"]:
        open(out_dir / rec["folder"] / name, "wb").close()
    written = []
    real = ff.png_writer
    monkeypatch.setattr(ff, "png_writer", lambda path, data: (written.append((os.path.basename(path), np.array(data))), real(path, data)))
    with S.output_directory(monkeypatch, out_dir):
        folder, joined, count, ctx = ff.VRGDGFaceFixStoreAnchors().store(x, dict(rec["context_in"]))
    assert sorted(os.listdir(folder)) == rec["files_after"] and [n for n, _ in written] == rec["written"]
    assert np.array_equal(np.stack([d for _, d in written]), S.ARRAYS["store.face_fix.bgr"])
    decoded = np.stack([np.asarray(Image.open(os.path.join(folder, n)).convert("RGB")) for n in rec["written"]])
    assert np.array_equal(decoded, S.ARRAYS["store.face_fix.bgr"][..., ::-1])

    video = str(tmp_path / "ltx_working_video.mp4")
    open(video, "wb").close()
    prepared = {"job_id": "job_a", "ltx_video_path": video, "frame_count": 40, "ltx_width": 960, "ltx_height": 544}
    stored = ve.VRGDGVideoEnhanceStoreAnchors().store(x.to(dev), ctx_in)[3]
    out = ve.VRGDGVideoEnhanceCollectLTXInputs().collect(prepared, stored)
    assert out[:6] == (video, stored["enhanced_anchor_folder"], "0,8,15", 3, 960, 544) and out[6]["anchor_indices"] == [0, 8, 15]

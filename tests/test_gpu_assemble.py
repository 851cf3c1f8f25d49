"""The music-video assembly on the GPU (csrc/vrg_assemble.hip through ops.assemble_frames, ops.assemble_labelled_bytes and the nodes):
every output bit for bit against the reference restated in numpy (assemble_support).  Copies, one correctly rounded division and
truncations only, so there is no tolerance.  Nothing reads a reference checkout."""
import importlib
import os

import numpy as np
import pytest
import torch

import assemble_support as S
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
IDS = [c["name"] for c in S.CASES]


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture()
def node(pkg):
    return importlib.import_module(PKG_NAME + ".VRGDG_VideoAssembly")


def _case(name):
    return next(c for c in S.CASES if c["name"] == name)


def _plan(ops, case):
    return ops.assemble_plan(case["mode"], [None if n is None else (n, *case["hwc"]) for n in case["lengths"]], **case["kw"])


def _cuda(clips):
    return [None if c is None else torch.from_numpy(c).cuda() for c in clips]


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=IDS)
def test_clean_join_is_bit_exact(ops, i):
    """uint32 views equal numpy's concatenation on frames that hold NaN (two payloads), +-Inf, -0.0 and 1e-40"""
    case = S.CASES[i]
    clips = S.case_clips(case, "special")
    want = S.expected_join(case, clips)
    got = ops.assemble_frames(_cuda(clips), _plan(ops, case))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert S.same_bits(got.cpu().numpy(), want) == 0
    words = want.view(np.uint32)
    assert (words == 0xffa5a5a5).any() and (words == 0x80000000).any() and (want == np.float32(1e-40)).any() and np.isinf(want).any()


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=IDS)
def test_bytes_sources_give_byte_over_255(ops, i):
    case = S.CASES[i]
    data = S.case_clips(case, "bytes")
    want = S.expected_join(case, [None if b is None else b.astype(np.float32) / 255.0 for b in data])
    got = ops.assemble_frames(_cuda(data), _plan(ops, case))
    assert got.dtype == torch.float32 and S.same_bits(got.cpu().numpy(), want) == 0


@pytest.mark.parametrize("with_overlays", (False, True), ids=("black-bar", "overlays"))
@pytest.mark.parametrize("i", [k for k, c in enumerate(S.CASES) if c["hwc"][2] == 3], ids=[n for n, c in zip(IDS, S.CASES) if c["hwc"][2] == 3])
def test_labelled_bytes_and_their_clean_batch(ops, i, with_overlays):
    """the writer's bytes equal the restatement byte for byte inside the contract range (k / 255 and its two neighbours included); the
    clean fp32 batch of the same launch is vrg_assemble_f32's"""
    case = S.CASES[i]
    clips = S.case_clips(case, "contract")
    want = S.expected_labelled(case, clips, with_overlays)
    dev, plan = _cuda(clips), _plan(ops, case)
    data, clean = ops.assemble_labelled_bytes(dev, plan, S.overlays_for(case) if with_overlays else None, clean_out=True)
    assert data.is_cuda and data.dtype == torch.uint8 and tuple(data.shape) == want.shape
    assert S.same_bits(data.cpu().numpy(), want) == 0
    assert torch.equal(clean.view(torch.int32), ops.assemble_frames(dev, plan).view(torch.int32))
    alone, none = ops.assemble_labelled_bytes(dev, plan, S.overlays_for(case) if with_overlays else None)
    assert none is None and torch.equal(alone, data)


def test_all_levels_on_the_device(ops):
    """every byte level and its neighbours through the device's chain, fp32 and byte sources, and the out-of-range rule"""
    unit = np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0
    x = np.concatenate([unit, np.nextafter(unit, np.float32(2.0)), np.nextafter(unit, np.float32(-1.0))[1:], np.zeros(1, np.float32)])
    assert x.size == 768
    clip = np.ascontiguousarray(x.reshape(1, 16, 16, 3))
    want = S.label_bar_bytes(clip)
    got, _ = ops.assemble_labelled_bytes([torch.from_numpy(clip).cuda()], [(0, 0)])
    assert S.same_bits(got.cpu().numpy(), want) == 0
    levels = np.arange(768, dtype=np.int64).astype(np.uint8).reshape(1, 16, 16, 3)
    got, clean = ops.assemble_labelled_bytes([torch.from_numpy(levels).cuda()], [(0, 0)], clean_out=True)
    assert S.same_bits(got.cpu().numpy(), S.label_bar_bytes(levels.astype(np.float32) / 255.0)) == 0
    assert S.same_bits(clean.cpu().numpy(), levels.astype(np.float32) / 255.0) == 0
    wild = np.zeros((1, 2, 2, 3), np.float32)
    wild.reshape(-1)[:10] = [np.nan, -np.inf, -3.0, -1e-3, -0.0, 256.0 / 255.0, 1.01, 7.0, 1e30, np.inf]
    got, _ = ops.assemble_labelled_bytes([torch.from_numpy(wild).cuda()], [(0, 0)])
    image = got.cpu().numpy()[0, :2][:, :, ::-1].reshape(-1)
    assert image[:10].tolist() == [0, 0, 0, 0, 0, 255, 255, 255, 255, 255]


@pytest.mark.parametrize("hwc", ((33, 37, 3), (32, 36, 3)), ids=("dword", "vector"))
def test_workgroups_stride_over_tiles(ops, hwc):
    """more output frames than the launch has workgroups to give each tile one (8192): a workgroup then walks several tiles of its frame.
    8200 frames of two 1024-pixel tiles leave one x workgroup per frame in the labelled launch and in the join"""
    clip = S.contract_clip((3, *hwc), 5)
    idx = np.arange(8200) % 3
    plan = [(0, int(f)) for f in idx]
    dev = [torch.from_numpy(clip).cuda()]
    data, clean = ops.assemble_labelled_bytes(dev, plan, [S.pattern_bar(1, hwc[1])], clean_out=True)
    assert S.same_bits(clean.cpu().numpy(), clip[idx]) == 0
    assert S.same_bits(data.cpu().numpy(), S.label_bar_bytes(clip, S.pattern_bar(1, hwc[1]))[idx]) == 0
    assert torch.equal(ops.assemble_frames(dev, plan), clean)


@pytest.mark.parametrize("hwc", ((5, 7, 3), (4, 4, 3)), ids=("dword", "vector"))
def test_more_frames_than_one_launch_takes(ops, hwc):
    """blockIdx.y takes 32768 frames a launch: 33000 output frames are two launches over one table"""
    clip = S.contract_clip((3, *hwc), 6)
    idx = (np.arange(33000) * 7) % 3
    plan = np.stack([np.zeros_like(idx), idx], axis=1)
    data, clean = ops.assemble_labelled_bytes([torch.from_numpy(clip).cuda()], plan, clean_out=True)
    assert S.same_bits(clean.cpu().numpy(), clip[idx]) == 0 and S.same_bits(data.cpu().numpy(), S.label_bar_bytes(clip)[idx]) == 0
    assert torch.equal(ops.assemble_frames([torch.from_numpy(clip).cuda()], plan), clean)


def test_off_grid_source_and_out_slice(ops):
    """a source that is batch[1:] of 105-float frames (an off-grid base) and out= a slice of a larger buffer whose surroundings stay"""
    case = _case("v3-dword-5x7")
    clips = S.case_clips(case, "special")
    want = S.expected_join(case, clips)
    dev = []
    for c in clips:
        if c is None:
            dev.append(None)
            continue
        batch = torch.from_numpy(np.concatenate([np.full((1, *c.shape[1:]), 3.5, np.float32), c])).cuda()
        dev.append(batch[1:])
        assert dev[-1].data_ptr() % 16 != 0
    big = torch.full((want.shape[0] + 3, *want.shape[1:]), 7.25, dtype=torch.float32, device="cuda")
    out = big[1:1 + want.shape[0]]
    got = ops.assemble_frames(dev, _plan(ops, case), out=out)
    assert got.data_ptr() == out.data_ptr()
    host = big.cpu().numpy()
    assert S.same_bits(host[1:1 + want.shape[0]], want) == 0
    assert (host[0] == 7.25).all() and (host[1 + want.shape[0]:] == 7.25).all()
    # the same through the vector route: 4 x 4 x 3 frames, everything on the grid
    case = _case("v3-vector-4x4")
    clips = S.case_clips(case, "special")
    want = S.expected_join(case, clips)
    big = torch.full((want.shape[0] + 2, *want.shape[1:]), 7.25, dtype=torch.float32, device="cuda")
    out = big[1:1 + want.shape[0]]
    assert out.data_ptr() % 16 == 0
    ops.assemble_frames(_cuda(clips), _plan(ops, case), out=out)
    host = big.cpu().numpy()
    assert S.same_bits(host[1:-1], want) == 0 and (host[0] == 7.25).all() and (host[-1] == 7.25).all()
    with pytest.raises(ValueError):
        ops.assemble_frames(_cuda(clips), _plan(ops, case), out=big[:want.shape[0], :, :, :2])
    with pytest.raises(ValueError):                                                      # out overlapping a source
        src = torch.zeros(6, 4, 4, 3, device="cuda")
        ops.assemble_frames([src[:3]], [(0, 0), (0, 1)], out=src[2:4])


def test_cpu_in_cpu_out_uploads_only_the_kept_frames(ops, monkeypatch):
    """CPU clips: the batch comes back on the CPU, inputs are not written, and a trimmed tail poisoned with NaN is neither uploaded
    nor read"""
    case = _case("v5-sixteen")
    clips = S.case_clips(case, "contract")
    plan = _plan(ops, case)
    want = S.expected_join(case, clips)
    kept = {s: max(f for t, f in plan if t == s) + 1 for s in {s for s, _ in plan}}
    assert any(kept[s] < clips[s].shape[0] for s in kept)
    poisoned = [c.copy() for c in clips]
    for s, c in enumerate(poisoned):
        c[kept.get(s, 0):] = np.nan
    before = [c.copy() for c in poisoned]
    uploaded = []
    real_to = torch.Tensor.to

    def spy(self, *args, **kw):
        if not self.is_cuda and self.dtype == torch.float32 and self.ndim == 4:
            uploaded.append(self)
        return real_to(self, *args, **kw)

    monkeypatch.setattr(torch.Tensor, "to", spy)
    got = ops.assemble_frames([torch.from_numpy(c) for c in poisoned], plan)
    data, clean = ops.assemble_labelled_bytes([torch.from_numpy(c) for c in poisoned], plan, clean_out=True)
    monkeypatch.undo()
    assert not got.is_cuda and not data.is_cuda and not clean.is_cuda
    assert S.same_bits(got.numpy(), want) == 0 and S.same_bits(clean.numpy(), want) == 0
    assert S.same_bits(data.numpy(), S.expected_labelled(case, clips, False)) == 0
    assert uploaded and not any(bool(torch.isnan(t).any()) for t in uploaded)
    assert sum(int(t.shape[0]) for t in uploaded) == 2 * sum(kept.values())
    assert all(S.same_bits(a, b) == 0 for a, b in zip(poisoned, before))
    # one clip on the device, the others on the CPU: the batch stays on the device
    mixed = [torch.from_numpy(c) for c in clips]
    mixed[0] = mixed[0].cuda()
    got = ops.assemble_frames(mixed, plan)
    assert got.is_cuda and S.same_bits(got.cpu().numpy(), want) == 0
    # other float types are widened by torch first
    half = [torch.from_numpy(c).cuda().half() for c in clips]
    assert torch.equal(ops.assemble_frames(half, plan), torch.cat([half[s][f:f + 1].float() for s, f in plan]))


def test_refusals(ops):
    a, b = torch.zeros(2, 4, 4, 3, device="cuda"), torch.zeros(2, 4, 5, 3, device="cuda")
    with pytest.raises(ValueError):
        ops.assemble_frames([a, b], [(0, 0), (1, 0)])                                    # shapes differ
    with pytest.raises(ValueError):
        ops.assemble_frames([a], [(0, 2)])                                               # a frame outside its clip
    with pytest.raises(ValueError):
        ops.assemble_frames([a] * 17, [(i, 0) for i in range(17)])                       # more than 16 sources
    with pytest.raises(ValueError):
        ops.assemble_frames([a, a.to(torch.uint8)], [(0, 0), (1, 0)])
    with pytest.raises(ValueError):
        ops.assemble_labelled_bytes([torch.zeros(2, 4, 4, 4, device="cuda")], [(0, 0)])  # labelled, C != 3
    with pytest.raises(ValueError):
        ops.assemble_labelled_bytes([a], [(0, 0)], [np.zeros((60, 5, 3), np.uint8)])
    assert tuple(ops.assemble_frames([a] * 16, [(i, 1) for i in range(16)]).shape) == (16, 4, 4, 3)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the nodes, seams injected
# ---------------------------------------------------------------------------------------------------------------------------------------
def _kwargs(clips):
    return {f"video_{i + 1}": torch.from_numpy(c).cuda() for i, c in enumerate(clips) if c is not None}


def test_v2_and_v3_nodes(ops, node):
    case = _case("v2-pad")
    clips = S.case_clips(case, "special")
    out, = node.VRGDG_CombinevideosV2().blend_videos(case["kw"]["fps"], case["kw"]["audio_meta"], **_kwargs(clips))
    assert out.is_cuda and S.same_bits(out.cpu().numpy(), S.expected_join(case, clips)) == 0
    case = _case("v3-dword-5x7")
    clips = S.case_clips(case, "special")
    out, = node.VRGDG_CombinevideosV3().blend_videos(25.0, 4.0, case["kw"]["audio_meta"], 0, 1, 16, **_kwargs(clips))
    assert S.same_bits(out.cpu().numpy(), S.expected_join(case, clips)) == 0
    with pytest.raises(RuntimeError):                                                    # groups_in_last_set = 0: nothing to join
        node.VRGDG_CombinevideosV3().blend_videos(25.0, 4.0, case["kw"]["audio_meta"], 0, 1, 0, **_kwargs(clips))


@pytest.mark.parametrize("name", ("v5-last-run", "v5-sixteen"))
def test_v5_node_hands_the_writer_the_bytes(ops, node, monkeypatch, tmp_path, name):
    case = _case(name)
    clips = S.case_clips(case, "contract")
    calls, labels = [], []

    def renderer(text, width):
        labels.append(text)
        return S.pattern_bar(int(text.rsplit(" ", 1)[1]), width)

    monkeypatch.setattr(node, "label_renderer", renderer)
    monkeypatch.setattr(node, "video_writer", lambda frames, path, fps: calls.append((np.array(frames), path, fps)))
    kw = case["kw"]
    index = kw.get("index", 0)
    out, = node.VRGDG_CombinevideosV5().blend_videos(kw["fps"], 4.0, kw["audio_meta"], index, kw.get("total_sets", 1),
                                                     kw.get("groups_in_last_set", 16), str(tmp_path), True, **_kwargs(clips))
    assert out.is_cuda and S.same_bits(out.cpu().numpy(), S.expected_join(case, clips)) == 0
    (frames, path, fps), = calls
    assert path == os.path.join(str(tmp_path), "WithLabels", f"set{index + 1}_combined.mp4") and fps == kw["fps"]
    assert os.path.isdir(os.path.dirname(path))
    assert frames.dtype == np.uint8 and S.same_bits(frames, S.expected_labelled(case, clips, True)) == 0
    slots = sorted({s + 1 for s, _ in _plan(ops, case)})
    assert labels == [f"set {index + 1} - group {s}" for s in slots]
    calls.clear()
    out, = node.VRGDG_CombinevideosV5().blend_videos(kw["fps"], 4.0, kw["audio_meta"], index, kw.get("total_sets", 1),
                                                     kw.get("groups_in_last_set", 16), str(tmp_path), False, **_kwargs(clips))
    assert not calls and S.same_bits(out.cpu().numpy(), S.expected_join(case, clips)) == 0


def test_pad_and_load_nodes(ops, node, monkeypatch, tmp_path):
    for name in ("pad-front", "pad-tail"):
        case = _case(name)
        clip = S.case_clips(case, "special")[0]
        out, = node.VRGDG_PadVideoWithLastFrame().pad_video(torch.from_numpy(clip).cuda(), **case["kw"])
        assert out.is_cuda and S.same_bits(out.cpu().numpy(), S.pad_video(clip, **case["kw"])) == 0
        out, = node.VRGDG_PadVideoWithLastFrame().pad_video(torch.from_numpy(clip), **case["kw"])
        assert not out.is_cuda and S.same_bits(out.numpy(), S.pad_video(clip, **case["kw"])) == 0
    files = {"b.mp4": S.bytes_clip((2, 5, 7, 3), 1), "a.MOV": S.bytes_clip((3, 5, 7, 3), 2), "c.mkv": None, "d.avi": S.bytes_clip((1, 5, 7, 3), 3),
             "notes.txt": None}
    for name in files:
        (tmp_path / name).write_bytes(b"")
    seen = []

    def decoder(path):
        seen.append(os.path.basename(path))
        return files[os.path.basename(path)]

    monkeypatch.setattr(node, "video_decoder", decoder)
    out, = node.VRGDG_LoadVideos().load_videos(None, str(tmp_path), 3)
    assert seen == ["a.MOV", "b.mp4", "c.mkv"]
    want = np.concatenate([files["a.MOV"], files["b.mp4"]]).astype(np.float32) / 255.0
    assert not out.is_cuda and out.dtype == torch.float32 and S.same_bits(out.numpy(), want) == 0

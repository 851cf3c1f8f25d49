"""Video Enhance Prepare on the MI355X (csrc/vrg_prepare.hip through ops.prepare_frames and the node): the fp32 frames equal the shipped
resize kernel's bit for bit, the bytes are numpy's rounding of those frames, both equal the recorded run of the reference
(tests/golden/prepare.npz), and the node gives the same results from host and device frames, in one piece or in several.

Bounds.  Test 1 and 2 are equalities.  Test 3 compares with the recording by resize_support.mismatches, the helper (and the rule: no
differing element) of tests/test_gpu_resize.py::test_resize_fixtures_bit_equal -- the recording was made by torch's plain CPU kernels,
which csrc/vrg_resize_math.hpp restates; the bytes then differ by no level at all, which the one-level bound of the issue contains."""
import os
import re

import numpy as np
import pytest
import torch

import prepare_support as PS
import resize_support as RS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def vep(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_VideoEnhancePrepare
    return VRGDG_VideoEnhancePrepare


@pytest.fixture(scope="module")
def golden():
    return PS.arrays()


def dev():
    return torch.device("cuda", torch.cuda.current_device())


FRAMES = 18
INDEX_LISTS = (None, [0], [FRAMES - 1, 0, 0, 3], PS.anchor_list(18, 8))
_INPUTS = {}


def source_frames(source):
    """the 18 seeded frames of a source of the sweep, made once and shared by the tests"""
    if source not in _INPUTS:
        _INPUTS[source] = PS.special_frames((FRAMES, *source), 40 + PS.SOURCES.index(source)).to(dev())
    return _INPUTS[source]


@pytest.mark.parametrize("method", PS.METHODS)
@pytest.mark.parametrize("source", PS.SOURCES, ids=["x".join(map(str, s)) for s in PS.SOURCES])
def test_f32_equals_the_shipped_resize_and_bytes_its_rounding(ops, source, method):
    """tests 1 and 2 of the sweep: torch.equal with ops.resize_geometry_frames(x[idx]) -- the shipped kernel is the yardstick -- and
    out_u8 == np.round(out_f32 * 255).astype(uint8); letterbox bars are 0; either output alone equals itself beside the other"""
    x = source_frames(source)
    checked = 0
    for gi, g in enumerate(PS.geometries(ops, source)):
        for li, idx in enumerate(INDEX_LISTS):
            picked = x if idx is None else x[torch.tensor(idx, device=x.device)]
            want = ops.resize_geometry_frames(picked, g, method)
            f32, u8 = ops.prepare_frames(x, g, method, idx)
            assert f32.dtype == torch.float32 and u8.dtype == torch.uint8 and f32.shape == u8.shape == want.shape
            assert torch.equal(f32, want), (g, idx, int((f32 != want).sum()))
            host = f32.cpu().numpy()
            assert np.array_equal(u8.cpu().numpy(), np.round(host * np.float32(255)).astype(np.uint8)), (g, idx)
            if g.dst[0] > 0 or g.dst[1] > 0:                                   # letterbox bars
                bars = torch.ones(g.out_h, g.out_w, dtype=torch.bool)
                bars[max(0, g.dst[1]):g.dst[1] + g.dst[3], max(0, g.dst[0]):g.dst[0] + g.dst[2]] = False
                assert bars.any() and int(u8.cpu()[:, bars].max()) == 0 and float(f32.cpu()[:, bars].abs().max()) == 0.0
            only_f32, none = ops.prepare_frames(x, g, method, idx, want_u8=False)
            assert none is None and torch.equal(only_f32, f32)
            none, only_u8 = ops.prepare_frames(x, g, method, idx, want_f32=False)
            assert none is None and torch.equal(only_u8, u8)
            checked += 1
    assert checked >= 12 * len(INDEX_LISTS)


def test_special_values_reach_the_bytes(ops):
    """a 1:1 nearest copy hands every sprinkled value (0, 1, k / 255, the ties and their neighbours, out-of-range) to the byte rule"""
    x = PS.special_frames((2, 16, 259, 3), 77)
    g = ops.resize_geometry(16, 259, 259, 16, PS.STRETCH)
    f32, u8 = ops.prepare_frames(x.to(dev()), g, PS.NEAREST)
    assert torch.equal(f32.cpu(), x.clamp(0, 1))
    assert np.array_equal(u8.cpu().numpy(), PS.quantise(x.clamp(0, 1).numpy()))
    ties = ((np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255)).astype(np.float32)
    assert np.isin(ties[:255], x.numpy()).all()


def test_against_the_reference_recording(ops, golden):
    """test 3: fp32 by resize_support.mismatches (no differing element), bytes within one level of the recorded PNG bytes, and the share of
    differing bytes -- printed -- no larger than that of quantise(ops.resize_frames(...)), the parent path, on the same case"""
    for case in PS.META["cases"]:
        x = PS.seeded_frames(case["seed"], case["shape"]).to(dev())
        a = case["args"]
        for which, idx in (("ltx", None), ("anchors", case["anchor_indices"])):
            width, height = (case["resolved"][("ltx_" if which == "ltx" else "anchor_") + k] for k in ("width", "height"))
            g = ops.resize_geometry(x.shape[1], x.shape[2], width, height, a["fit_mode"])
            f32, u8 = ops.prepare_frames(x, g, a["resize_method"], idx)
            want, want_png = golden[f"{case['key']}.{which}"], golden[f"{case['key']}.{which}_png"]
            assert RS.mismatches(f32.cpu().numpy(), want) == 0, (case["key"], which)
            got = u8.cpu().numpy().astype(np.int16)
            assert got.shape == want_png.shape and int(np.abs(got - want_png).max()) <= 1
            picked = x if idx is None else x[torch.tensor(idx, device=x.device)]
            parent = PS.quantise(ops.resize_frames(picked, width, height, a["fit_mode"], a["resize_method"]).cpu().numpy())
            share, parent_share = float((got != want_png).mean()), float((parent != want_png).mean())
            print(f"{case['key']}.{which}: {100 * share:.4f} % of the bytes differ from the recording (parent path: {100 * parent_share:.4f} %)")
            assert share <= parent_share


def _run_node(vep, tmp_path, name, frames, case, encodes):
    out_dir = tmp_path / name
    out_dir.mkdir()
    with PS.stub_folder_paths(out_dir):
        out = vep.VRGDGVideoEnhancePrepare().prepare(frames, **case["args"])
    assert len(encodes) >= 1
    return out


@pytest.mark.parametrize("ci", [0, 1, 4])
def test_node_end_to_end(vep, golden, tmp_path, monkeypatch, ci):
    """test 4: host frames, device frames and host frames in forced small pieces give equal tuples; the PNG files decode to the recorded
    bytes; names, layout, context and the ffmpeg hand-off are the recording's; the input is unmodified and handed on as it is"""
    from PIL import Image
    from comfyui_vrgamedevgirl_amd import _devices
    case = PS.META["cases"][ci]
    encodes = []
    monkeypatch.setattr(vep, "_encode_mp4", lambda folder, count, fps, path: encodes.append((folder, count, fps, path)))
    monkeypatch.setattr(vep, "_log", lambda message: None)
    x = PS.seeded_frames(case["seed"], case["shape"])
    keep = x.clone()
    frame_bytes = x[0].numel() * 4
    xd = x.to(dev())
    results = {"host": _run_node(vep, tmp_path, "host", x, case, encodes)}
    results["device"] = _run_node(vep, tmp_path, "device", xd, case, encodes)
    monkeypatch.setattr(_devices, "PIPE_BYTES", 5 * frame_bytes)              # pieces of five frames: anchors 0, 8, 16, 17 fall into four of them
    results["pieces"] = _run_node(vep, tmp_path, "pieces", x, case, encodes)
    assert torch.equal(x, keep) and torch.equal(xd.cpu(), keep)
    for name, out in results.items():
        ctx = out[8]
        assert len(out) == 9 and ctx["original_frames"] is (xd if name == "device" else x)
        assert out[0].is_cuda == out[1].is_cuda == (name == "device")
        assert RS.mismatches(out[0].cpu().numpy(), golden[f"{case['key']}.ltx"]) == 0, name
        assert RS.mismatches(out[1].cpu().numpy(), golden[f"{case['key']}.anchors"]) == 0, name
        assert [out[2], out[3], out[5], out[6], out[7]] == case["returns"]
        assert list(ctx) == case["context_keys"] and {k: ctx[k] for k in case["context"]} == case["context"]
        assert ctx["anchor_indices"] == case["anchor_indices"] and {k: ctx[k] for k in case["resolved"]} == case["resolved"]
        assert re.fullmatch(case["job_id_pattern"], ctx["job_id"])
        job = os.path.join(str(tmp_path / name), *case["layout"]["job_folder"].replace("{job_id}", ctx["job_id"]).split("/"))
        assert ctx["job_folder"] == job and ctx["anchor_sources_folder"] == os.path.join(job, case["layout"]["anchor_sources_folder"])
        assert out[4] == ctx["ltx_video_path"] == os.path.join(job, case["layout"]["ltx_video_path"])
        frames_folder = os.path.join(job, case["layout"]["ltx_working_frames"])
        assert sorted(os.listdir(frames_folder)) == case["frame_files"] and sorted(os.listdir(ctx["anchor_sources_folder"])) == case["anchor_files"]
        for folder, files, key in ((frames_folder, case["frame_files"], "ltx"), (ctx["anchor_sources_folder"], case["anchor_files"], "anchors")):
            decoded = np.stack([np.asarray(Image.open(os.path.join(folder, n))) for n in files])
            assert np.array_equal(decoded, golden[f"{case['key']}.{key}_png"]), (name, key)
            assert np.array_equal(decoded, PS.quantise(out[0 if key == "ltx" else 1].cpu().numpy()))
    assert len(encodes) == 3
    for (folder, count, fps, path), out in zip(encodes, results.values()):
        assert folder == os.path.join(out[8]["job_folder"], "ltx_working_frames") and path == out[4]
        assert (count, fps) == (case["encode"]["frame_count"], case["encode"]["fps"])


def test_an_index_outside_the_batch_raises_and_launches_nothing(ops, monkeypatch):
    from comfyui_vrgamedevgirl_amd import _hip
    x = source_frames(PS.SOURCES[0])
    g = ops.resize_geometry(5, 7, 4, 4, PS.STRETCH)
    launched = []
    monkeypatch.setattr(_hip, "lib", lambda: launched.append(1) or (_ for _ in ()).throw(AssertionError("launched")))
    for bad in ([FRAMES], [0, -1], [3, 2 ** 31]):
        with pytest.raises(ValueError, match="outside the batch"):
            ops.prepare_frames(x, g, PS.BICUBIC, bad)
    assert not launched
    monkeypatch.undo()
    f32, u8 = ops.prepare_frames(x, g, PS.BICUBIC, [])
    assert f32.shape == u8.shape == (0, 4, 4, 3)

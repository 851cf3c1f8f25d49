"""The landmark-aligned Face Fix composite on the MI355X: vrg_warp_affine_u8 and vrg_face_bytes_u8 against the numpy restatement of
tests/warp_support.py byte for byte, and VRGDGFaceFixCompositeLandmarkAligned against every recorded case of the reference
(tests/golden/landmark.*) bit for bit -- image and mask digests and samples, the count and the log line with its `aligned` number --
with device-resident and with host-fed originals, under torch.inference_mode(), with the inputs unchanged.  Reads only tests/golden/."""
import numpy as np
import pytest
import torch

import warp_support as WS
from test_warp_host import CASES as WARP_CASES, IDS as WARP_IDS

pytestmark = pytest.mark.gpu
CASES = WS.meta()["cases"]


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def FF(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes
    return VRGDG_StandaloneFaceFixNodes


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().numpy()


@pytest.mark.parametrize("src,dst,transform,kind", WARP_CASES, ids=WARP_IDS)
def test_warp_equals_the_restatement(ops, src, dst, transform, kind):
    frames = np.stack([WS.frames_of(src, kind, 200 + k) for k in range(3)])
    x = torch.from_numpy(frames).to(dev())
    got = bits(ops.warp_affine_u8(x, [transform, None, transform], dst[1], dst[0]))
    assert np.array_equal(got[0], WS.restated(frames[0], transform, dst[1], dst[0]))
    assert not got[1].any() and np.array_equal(got[2], WS.restated(frames[2], transform, dst[1], dst[0]))
    assert np.array_equal(bits(x), frames)


def test_warp_of_a_large_frame_equals_the_restatement(ops):
    frame = WS.frames_of((270, 480), "smooth", 17)
    t = WS.similarity(1.04, -6.0, 3.3, -2.7, (240, 135))
    got = bits(ops.warp_affine_u8(torch.from_numpy(frame[None]).to(dev()), [t], 480, 270))[0]
    assert np.array_equal(got, WS.restated(frame, t, 480, 270))


def test_face_bytes_equal_the_restatement(ops):
    """generated = quantise(clamp(bicubic)) where the bicubic face is what the opaque composite blends with alpha 1 (feather 0, centre of
    the box); source = quantise(original under the box) everywhere"""
    rng = np.random.Generator(np.random.PCG64(5))
    originals = torch.from_numpy((rng.random((3, 50, 70, 4), dtype=np.float32) * 1.3 - 0.15)).to(dev())
    originals[0, 20, 30, 1] = float("nan")
    work = torch.from_numpy(rng.random((4, 24, 20, 3), dtype=np.float32) * 1.2 - 0.1).to(dev())
    rows = [{"original": 0, "crop": 1, "box": (10, 5, 51, 38)}, {"original": 1, "crop": 0, "box": None}, {"original": 2, "crop": 3, "box": (0, 0, 70, 50)}]
    faces = ops.face_bytes(work, rows, 50, 70, originals=originals)
    only = ops.face_bytes(work, rows, 50, 70)
    assert faces.offsets[1] == -1 and faces.sizes[1] is None and only.source is None
    assert torch.equal(only.generated, faces.generated)
    gen, src = bits(faces.generated), bits(faces.source)
    out, mask = ops.composite_frames(originals, work, rows, ops.CompositeRule("opaque", feather=0), 0.0)
    for f in (0, 2):
        l, t, r, b = rows[f]["box"]
        want_source = WS.quantise(bits(originals[f, t:b, l:r, :3]))
        assert np.array_equal(faces.image(src, f), want_source)
        inside = bits(mask[f, t:b, l:r]) == 1.0
        assert inside.sum() > 0.7 * inside.size
        face = bits(out[f, t:b, l:r, :3])                                  # alpha 1: target * 0 + face * 1 = the clamped bicubic face
        finite = inside & np.isfinite(bits(originals[f, t:b, l:r, :3])).all(axis=2)
        assert np.array_equal(faces.image(gen, f)[finite], WS.quantise(face)[finite])
    assert faces.image(src, 0)[15, 20, 1] == 0                              # the NaN became byte 0


def run_case(FF, case, where):
    originals_np, work_np = WS.case_inputs(case)
    originals, work = torch.from_numpy(originals_np.copy()), torch.from_numpy(work_np.copy())
    if where != "cpu":
        originals, work = originals.to(dev()), work.to(dev())
    ctx = {"original_frames": originals, "entries": WS.case_entries(case), "ltx_frame_offset": case["offset"]}
    estimator = None

    class Node(FF.VRGDGFaceFixCompositeLandmarkAligned):
        pass

    if case["detector"]:                                                    # call k of the estimator = the k-th usable frame with a box
        usable = min(len(case["entries"]), max(0, case["work_shape"][0] - case["offset"]))
        estimator = WS.ScriptedEstimator([case["script"][i] for i in range(usable) if FF._has_area(ctx["entries"][i])])
        Node.estimator = staticmethod(estimator)
    res = Node().composite(work, ctx, case["feather_pixels"], case["transform_smoothing"])
    assert torch.equal(originals.cpu(), torch.from_numpy(originals_np)) and torch.equal(work.cpu(), torch.from_numpy(work_np))   # inputs unchanged
    return res, estimator, originals_np


@pytest.mark.parametrize("where", ["cpu", "device", "inference_mode"])
@pytest.mark.parametrize("case", CASES, ids=[c["key"] for c in CASES])
def test_node_on_the_fixture(FF, golden_dir, capsys, monkeypatch, case, where):
    golden = WS.arrays()
    if where == "cpu":                                                      # several pieces through the staging pipeline
        from comfyui_vrgamedevgirl_amd import _devices
        shape = case["originals_shape"]
        monkeypatch.setattr(_devices, "PIPE_BYTES", 2 * shape[1] * shape[2] * shape[3] * 4)
    capsys.readouterr()
    if where == "inference_mode":
        with torch.inference_mode():
            (image, mask, repaired), estimator, originals_np = run_case(FF, case, where)
    else:
        (image, mask, repaired), estimator, originals_np = run_case(FF, case, where)
    logged = capsys.readouterr().out
    assert image.is_cuda == (where != "cpu") and mask.is_cuda == (where != "cpu")
    assert repaired == case["repaired"] and logged == f"[VRGDG Face Fix] {case['log']}\n"
    assert f"aligned={case['aligned']}," in logged
    img, msk = bits(image), bits(mask)
    pos = WS.sample_positions(img.size, case["seed"])
    bad = int((img.reshape(-1)[pos].view(np.uint32) != golden[case["key"] + ".out_samples"].view(np.uint32)).sum())
    pos_m = WS.sample_positions(msk.size, case["seed"])
    bad_m = int((msk.reshape(-1)[pos_m].view(np.uint32) != golden[case["key"] + ".mask_samples"].view(np.uint32)).sum())
    print(f"{case['key']} [{where}]: {bad} of {pos.size} image samples and {bad_m} of {pos_m.size} mask samples differ")
    assert bad == 0 and bad_m == 0
    assert WS.sha(msk) == case["mask_sha256"] and WS.sha(img) == case["out_sha256"]
    if estimator is not None:                                               # what the estimator saw: the reference's two byte images
        assert estimator.calls == len(estimator.script)
        entries = WS.case_entries(case)
        boxed = [i for i in range(len(entries)) if FF._has_area(entries[i])][:estimator.calls]
        for i, (source, generated) in zip(boxed, estimator.seen):
            l, t, r, b = entries[i]["box"]
            assert source.dtype == np.uint8 and generated.dtype == np.uint8 and source.shape == generated.shape == (b - t, r - l, 3)
            assert np.array_equal(source, WS.quantise(originals_np[i, t:b, l:r, :3]))


@pytest.mark.parametrize("where", ["cpu", "device"])
def test_without_an_estimator_the_node_is_the_opaque_composite(FF, where, capsys):
    case = next(c for c in CASES if c["key"] == "resets")
    originals_np, work_np = WS.case_inputs(case)
    originals, work = torch.from_numpy(originals_np), torch.from_numpy(work_np)
    if where == "device":
        originals, work = originals.to(dev()), work.to(dev())
    ctx = {"original_frames": originals, "entries": WS.case_entries(case), "ltx_frame_offset": case["offset"]}
    assert FF.VRGDGFaceFixCompositeLandmarkAligned.estimator is None
    got = FF.VRGDGFaceFixCompositeLandmarkAligned().composite(work, ctx, 6, 0.75)
    assert "aligned=0, fallback=7," in capsys.readouterr().out
    want = FF.VRGDGFaceFixCompositeOpaque().composite(work, ctx, 6)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2] == 7


def test_ops_fallback_and_mixed_frames(ops):
    """no transform at all = composite_frames' bits; a transform on one frame leaves the other frames' bits alone; the identity transform
    blends the byte face (face quantised to n / 255), not the float one"""
    rng = np.random.Generator(np.random.PCG64(9))
    originals = torch.from_numpy(rng.random((3, 90, 120, 3), dtype=np.float32)).to(dev())
    work = torch.from_numpy(rng.random((3, 32, 32, 3), dtype=np.float32)).to(dev())
    rows = [{"original": i, "crop": i, "box": (10 + i, 8, 90 + i, 80)} for i in range(3)]
    want = ops.composite_frames(originals, work, rows, ops.CompositeRule("opaque", feather=5), 0.0)
    none = ops.aligned_composite_frames(originals, work, rows, 5, [None] * 3)
    assert torch.equal(none[0], want[0]) and torch.equal(none[1], want[1])
    ident = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32)
    got = ops.aligned_composite_frames(originals, work, rows, 5, [None, ident, None])
    assert torch.equal(got[1], want[1]) and torch.equal(got[0][0], want[0][0]) and torch.equal(got[0][2], want[0][2])
    assert not torch.equal(got[0][1], want[0][1])
    faces = ops.face_bytes(work, rows, 90, 120)
    face = faces.image(bits(faces.generated), 1).astype(np.float32) / np.float32(255.0)
    alpha = bits(want[1][1, 8:80, 11:91])[..., None]
    target = bits(originals[1, 8:80, 11:91])
    expect = np.clip(target * (np.float32(1) - alpha) + face * alpha, 0, 1).astype(np.float32)
    assert np.array_equal(bits(got[0][1, 8:80, 11:91]), expect)
    with pytest.raises(ValueError):
        ops.aligned_composite_frames(originals, work, rows, 5, [None, np.full((2, 3), np.nan, dtype=np.float32), None])

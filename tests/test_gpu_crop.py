"""The Face Fix crop sequence on the MI355X: csrc/vrg_crop.hip through VRGDG_StandaloneFaceFixNodes.face_crop_sequence against the
recorded results of the reference's two Prepare nodes (tests/golden/crop.json: digests; the inputs are rebuilt from their seeds) and, on
shapes too large for a fixture, against the same arithmetic compiled for the host (tests/host_math/crop_check.cpp, itself checked against
the fixture by tests/test_crop_host.py).  Everything is compared bit for bit."""
import numpy as np
import pytest
import torch

import crop_support as CS

pytestmark = pytest.mark.gpu
META = CS.meta()
CASES = META["cases"]
KEYS = [c["key"] for c in CASES]


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return CS.build_host_lib(tmp_path_factory.mktemp("crop_check"))


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
    return CS.arrays()


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().numpy()


@pytest.mark.parametrize("where", ("device", "host"))
@pytest.mark.parametrize("key", KEYS)
def test_fixture_cases_through_the_public_call(FF, golden, key, where):
    """(a) every fixture case, device-resident and CPU frames: batch, every frame and the anchors have the reference's digests; the
    prefix length is the reference's; the input is not written"""
    case = CASES[KEYS.index(key)]
    x = torch.from_numpy(CS.make_frames(case["shape"], case["seed"]))
    frames = x.to(dev()) if where == "device" else x.clone()
    crop, anchors, offset = FF.face_crop_sequence(frames, CS.entries_of(case), per_shot=case["per_shot"], anchors=case["anchors"])
    assert crop.device.type == ("cuda" if where == "device" else "cpu") and anchors.device == crop.device
    assert torch.equal(frames.cpu(), x)
    got = bits(crop)
    assert offset == case["ltx_frame_offset"] and list(got.shape) == case["crop_shape"] and got.dtype == np.float32
    print(CS.describe_difference(case, got, golden[key + ".samples"]))
    assert CS.frame_shas(got) == case["frame_sha256"]
    assert CS.sha(got) == case["crop_sha256"]
    assert list(anchors.shape) == case["anchor_shape"] and CS.sha(bits(anchors)) == case["anchor_sha256"]
    none = FF.face_crop_sequence(frames, CS.entries_of(case), per_shot=case["per_shot"])
    assert none[1] is None and none[2] == offset and torch.equal(none[0], crop)


def _large_entries(n, height, width):
    """64 boxes from 37 px to the whole frame height, square and not, at seeded positions, with leading, inner and trailing holes"""
    rng = np.random.Generator(np.random.PCG64(4242))
    sides = [37, 2160, 1024, 300, 150, 513, 2049, 64, 1500, 777]
    entries = []
    for i in range(n):
        if i in (0, 1, 9, 10, 11, 30, n - 2, n - 1):
            entries.append({"index": i, "box": None, "strength": 0.0, "shot_id": i // 16})
            continue
        bh = sides[i % len(sides)] if i % 7 else int(rng.integers(37, height + 1))
        bw = bh if i % 3 else min(width, int(bh * 1.5))
        left, top = int(rng.integers(0, width - bw + 1)), int(rng.integers(0, height - bh + 1))
        entries.append({"index": i, "box": (left, top, left + bw, top + bh), "strength": 1.0, "shot_id": i // 16})
    return entries


def test_4k_batch_against_the_host_arithmetic_and_host_fed_against_resident(hm, ops, FF):
    """(b) 64 4K frames, boxes from 37 px to 2160 px in one batch, holes and a prefix: device-resident == host arithmetic == host-fed"""
    n, height, width = 64, 2160, 3840
    x = CS.make_frames((n, height, width, 3), 99)
    entries = _large_entries(n, height, width)
    plan = ops.crop_sequence_plan(entries, n, height, width)
    heights = [b - t for _, (l, t, r, b) in plan.sources]
    assert min(heights) == 37 and max(heights) == 2160 and plan.ltx_offset == 1 and plan.count == 65
    want = CS.host_crop(hm, x, CS.plan_records(plan, 3))
    cpu = torch.from_numpy(x)
    resident = cpu.to(dev())
    got, _, offset = FF.face_crop_sequence(resident, entries)
    assert offset == 1 and tuple(got.shape) == (65, 512, 512, 3)
    bad = CS.mismatches(bits(got), want)
    print(f"4K batch: {bad} of {want.size} elements differ from the host arithmetic")
    assert bad == 0
    fed, _, _ = FF.face_crop_sequence(cpu, entries)
    assert fed.device.type == "cpu" and CS.mismatches(bits(fed), want) == 0
    assert ops.crop_host_bytes(plan) < x.nbytes // 4                       # only the boxes crossed
    shot = ops.crop_sequence_plan(entries, n, height, width, per_shot=True)
    assert shot.sources != plan.sources
    got_shot, _, _ = FF.face_crop_sequence(resident, entries, per_shot=True)
    assert CS.mismatches(bits(got_shot), CS.host_crop(hm, x, CS.plan_records(shot, 3))) == 0
    assert torch.equal(resident.cpu(), cpu)


def test_host_fed_in_pieces_equals_one_pack(ops, monkeypatch):
    """a pack limit smaller than the boxes: the pieces along the output-frame axis give the same batch"""
    from comfyui_vrgamedevgirl_amd import _devices
    x = torch.from_numpy(CS.make_frames((12, 96, 128, 4), 5))
    entries = [{"box": (i, 2 * i, i + 40 + i, 2 * i + 50)} if i % 4 else {"box": None} for i in range(12)]
    plan = ops.crop_sequence_plan(entries, 12, 96, 128)
    whole = ops.crop_frames_host(x, plan, size=(64, 48))
    resident = ops.crop_frames(x.to(dev()), plan, size=(64, 48))
    assert tuple(whole.shape) == (plan.count, 64, 48, 3) and torch.equal(whole, resident.cpu())
    monkeypatch.setattr(_devices, "PIN_LIMIT_BYTES", 70000)                # two or three boxes per piece
    assert torch.equal(ops.crop_frames_host(x, plan, size=(64, 48)), whole)
    monkeypatch.setattr(_devices, "PIN_LIMIT_BYTES", 1)                    # every box alone
    assert torch.equal(ops.crop_frames_host(x, plan, size=(64, 48)), whole)


def test_duplicated_records_give_identical_frames(ops):
    """(c) holes and the prefix re-read another frame's rectangle: equal bits"""
    x = torch.from_numpy(CS.make_frames((3, 70, 90, 3), 11)).to(dev())
    entries = [{"box": None}, {"box": (5, 7, 60, 66)}, {"box": None}]
    plan = ops.crop_sequence_plan(entries, 3, 70, 90)
    assert plan.ltx_offset == 6 and len(set(plan.sources)) == 1
    out = ops.crop_frames(x, plan)
    assert tuple(out.shape) == (9, 512, 512, 3)
    for k in range(1, 9):
        assert torch.equal(out[k], out[0]), k
    mine = torch.empty_like(out)
    assert ops.crop_frames(x, plan, out=mine) is mine and torch.equal(mine, out)


def test_records_outside_the_source_are_refused_before_any_launch(ops):
    """(d) a record that reaches past the source is a ValueError of ops; nothing is launched with it"""
    x = torch.zeros((2, 16, 16, 3), device=dev())
    fine = (0, 48, 3, 16, 16)
    assert tuple(ops.crop_resize(x, [fine], (8, 8)).shape) == (1, 8, 8, 3)
    for rec in ((x.numel() - 10, 48, 3, 4, 1), (0, 48, 3, 16, 33), (16 * 16 * 3, 48, 3, 17, 16), (-3, 48, 3, 4, 4), (0, 48, 2, 4, 4),
                (0, 48, 3, 0, 4), (0, -48, 3, 4, 4)):
        with pytest.raises(ValueError, match="refused"):
            ops.crop_resize(x, [fine, rec], (8, 8))
    last_pixel = (x.numel() - 3, 48, 3, 1, 1)                              # the last pixel of the source is still inside
    assert tuple(ops.crop_resize(x, [last_pixel], (8, 8)).shape) == (1, 8, 8, 3)
    with pytest.raises(ValueError, match="plan was made for"):
        ops.crop_frames(x, ops.crop_sequence_plan([{"box": (0, 0, 4, 4)}], 1, 16, 16))
    with pytest.raises(RuntimeError):
        ops.crop_frames(x.cpu(), ops.crop_sequence_plan([{"box": (0, 0, 4, 4)}] * 2, 2, 16, 16))


@pytest.mark.parametrize("key", ("holes_everywhere", "per_shot_fill", "rgba_source"))
def test_crop_batch_goes_through_the_opaque_composite(FF, key):
    """(e) plumbing: the crop batch, the fixture's entries and the context fields the reference builds are accepted unchanged by the
    composite node of this pack (shapes and the repaired count; no numeric claim)"""
    case = CASES[KEYS.index(key)]
    frames = torch.from_numpy(CS.make_frames(case["shape"], case["seed"])).to(dev())
    entries = CS.entries_of(case)
    crop, _, offset = FF.face_crop_sequence(frames, entries, per_shot=case["per_shot"])
    context = {"version": 1, "job_id": "test", "original_frames": frames, "entries": entries, "ltx_frame_offset": offset,
               "frame_count": int(crop.shape[0]), "original_frame_count": case["shape"][0]}
    out, masks, repaired = FF.VRGDGFaceFixCompositeOpaque().composite(crop, context, 0)
    assert tuple(out.shape) == tuple(frames.shape) and tuple(masks.shape) == tuple(frames.shape[:3])
    assert repaired == sum(1 for e in entries if e["box"])
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0

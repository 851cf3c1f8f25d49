"""The detector input on the MI355X: vrg_detect_blobs_f32 / _u8 and vrg_warp_linear_u8 against the numpy restatement of
tests/detect_support.py (itself equal to the host-compiled header, tests/test_detect_host.py) byte for byte -- blobs and rotated frames, every
frame kind, device-resident and host-fed frames, a non-zero storage offset, untouched inputs, zero blobs and the refusals -- and
detect_with_rotation with the fixture's recorded net against the reference's recorded candidates (tests/golden/detect_prep.json)."""
import json

import numpy as np
import pytest
import torch

import detect_support as D

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
def BF(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_FaceFix
    return VRGDG_FaceFix


@pytest.fixture(scope="module")
def restated():
    """(key, kind) -> (frames, blobs [F, A, R, 3, 300, 300], rotated [F, A, H, W, 3]) of the restatement, computed once and left unchanged"""
    cache = {}

    def get(key, kind="uniform"):
        if (key, kind) not in cache:
            _, _, mode, regions = D.CASES[key]
            x = D.case_frames(key, kind)
            cache[(key, kind)] = (x,) + D.restated_blobs(x, mode, regions)
        return cache[(key, kind)]

    return get


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def module_of(FF, BF, key):
    return BF if D.CASES[key][3] is not None else FF


def plan_of(FF, BF, key):
    shape, _, mode, regions = D.CASES[key]
    if regions is not None:
        return BF.detection_plan(shape[2], shape[1], mode, regions)
    return FF.detection_plan(shape[2], shape[1], mode)


def same(name, got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{name}: largest difference {diff.max() if diff.size else 0:g} levels, {float((diff != 0).mean()) if diff.size else 0:.4%} of the values differ")
    return bool((diff == 0).all())


@pytest.mark.parametrize("key", sorted(D.CASES))
def test_device_frames_equal_the_restatement(FF, BF, restated, key):
    x, blobs, rotated = restated(key)
    plan, M = plan_of(FF, BF, key), module_of(FF, BF, key)
    xd = torch.from_numpy(x).to(dev())
    assert same(f"{key} blobs", M.detector_blobs(xd, plan), blobs)
    assert same(f"{key} rotated frames", M.rotated_frames(xd, plan), rotated)
    assert np.array_equal(xd.cpu().numpy(), x, equal_nan=True)
    last = M.detector_blobs(xd, plan, frames=[x.shape[0] - 1])                          # a subset of the frames
    assert same(f"{key} last frame", last, blobs[-1:])


@pytest.mark.parametrize("kind", ("smooth", "special"))
@pytest.mark.parametrize("key", sorted(D.CASES))
def test_frame_kinds(FF, BF, restated, key, kind):
    x, blobs, rotated = restated(key, kind)
    plan, M = plan_of(FF, BF, key), module_of(FF, BF, key)
    xd = torch.from_numpy(x).to(dev())
    assert same(f"{key} {kind} blobs", M.detector_blobs(xd, plan), blobs)
    assert same(f"{key} {kind} rotated frames", M.rotated_frames(xd, plan), rotated)
    assert np.array_equal(xd.cpu().numpy(), x, equal_nan=True)


@pytest.mark.parametrize("key", ("light_640x420", "builder_u8"))
def test_storage_offset(FF, BF, restated, key):
    """frames that are a view into a larger buffer, starting 5 elements into it (fp32: 4 bytes off the 16-byte grid; bytes: odd)"""
    x, blobs, rotated = restated(key)
    plan, M = plan_of(FF, BF, key), module_of(FF, BF, key)
    buf = torch.zeros(x.size + 16, dtype=torch.from_numpy(x).dtype, device=dev())
    view = buf[5:5 + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x).to(dev()))
    assert view.storage_offset() == 5
    keep = buf.clone()
    assert same(f"{key} blobs at an offset", M.detector_blobs(view, plan), blobs)
    assert same(f"{key} rotated frames at an offset", M.rotated_frames(view, plan), rotated)
    assert torch.equal(buf, keep)


@pytest.mark.parametrize("key", ("light_640x420", "strong_97x61", "builder_u8"))
def test_host_fed_frames(FF, BF, restated, key, monkeypatch):
    from comfyui_vrgamedevgirl_amd import _devices
    x, blobs, rotated = restated(key)
    plan, M = plan_of(FF, BF, key), module_of(FF, BF, key)
    monkeypatch.setattr(_devices, "PIPE_BYTES", x[0].nbytes)                            # pieces of one frame
    for frames in (torch.from_numpy(x.copy()), torch.from_numpy(x.copy()).pin_memory()):
        got = M.detector_blobs(frames, plan)
        assert got.is_cuda and same(f"{key} host-fed blobs", got, blobs)
        assert same(f"{key} host-fed rotated frames", M.rotated_frames(frames, plan), rotated)
        assert np.array_equal(frames.numpy(), x)


def test_host_fed_calls_upload_only_the_frames_they_name(ops, FF, monkeypatch):
    """a CPU batch scanned in chunks, or for a subset of its frames, crosses PCIe once: every call hands the staging pipeline the frames
    its records name and no others"""
    from comfyui_vrgamedevgirl_amd import _devices
    x = D.make_frames("smooth", (7, 61, 97, 3), "f32", 12)
    cpu = torch.from_numpy(x.copy())
    want, rotated = D.restated_blobs(x, "Light: ±15°")
    plan = FF.detection_plan(97, 61, "Light: ±15°")
    handed, upload = [], _devices.upload_frames

    def counting(images, fn):
        handed.append(int(images.shape[0]))
        return upload(images, fn)

    monkeypatch.setattr(_devices, "upload_frames", counting)
    assert same("frames 2 .. 4", FF.detector_blobs(cpu, plan, frames=[2, 3, 4]), want[2:5]) and handed == [3]
    del handed[:]
    assert same("frames 6, 1, 1, 3", FF.detector_blobs(cpu, plan, frames=[6, 1, 1, 3]), want[[6, 1, 1, 3]]) and handed == [3]
    del handed[:]
    assert same("rotated frame 5", FF.rotated_frames(cpu, plan, frames=[5]), rotated[5:6]) and handed == [1]
    del handed[:]
    seen = []

    def forward(blobs):
        seen.append(blobs.cpu().numpy())
        return [np.zeros((k % 3, 7), dtype=np.float32) for k in range(blobs.shape[0])]      # ragged: 0, 1 or 2 rows per blob

    assert FF.detect_with_rotation(forward, cpu, 0.5, 4, "Light: ±15°", chunk_frames=3) == [[]] * 7
    assert handed == [3, 3, 1] and sum(handed) == 7                                          # 7 frames uploaded once, not once per chunk
    assert np.array_equal(np.concatenate(seen), want.reshape(-1, 3, 300, 300))
    assert np.array_equal(cpu.numpy(), x)


def test_records_in_any_order_and_other_float_types(ops, FF, restated):
    x, blobs, _ = restated("light_640x420")
    plan = FF.detection_plan(640, 420, "Light: ±15°")
    desc, _ = plan.descriptors([0, 1])
    order = np.random.Generator(np.random.PCG64(3)).permutation(desc.size)
    want = blobs.reshape(-1, 3, 300, 300)[order]
    assert same("shuffled records, device", ops.detect_blobs(torch.from_numpy(x).to(dev()), desc[order], plan.transforms), want)
    assert same("shuffled records, host-fed", ops.detect_blobs(torch.from_numpy(x.copy()), desc[order], plan.transforms), want)
    half = torch.from_numpy(x).to(dev()).half()
    assert torch.equal(ops.detect_blobs(half, desc, plan.transforms), ops.detect_blobs(half.float(), desc, plan.transforms))


def test_zero_blobs_and_refusals(ops, FF):
    x = torch.from_numpy(D.uniform_frames((1, 64, 96, 3), 1)).to(dev())
    assert tuple(ops.detect_blobs(x, [], None).shape) == (0, 3, 300, 300)
    assert tuple(ops.warp_linear_bytes(x, [], None).shape) == (0, 64, 96, 3)
    assert tuple(ops.detect_blobs(x[:0], [], None).shape) == (0, 3, 300, 300)
    plan = FF.detection_plan(96, 64, "Off (fastest)")
    assert tuple(FF.detector_blobs(x, plan, frames=[]).shape) == (0, 1, 1, 3, 300, 300)
    for bad in ((0, -1, 0, 0, 97, 64), (1, -1, 0, 0, 96, 64), (0, 0, 0, 0, 96, 64), (0, -1, 0, 0, 7, 64), (0, -1, 8, 8, 8, 64)):
        with pytest.raises(ValueError):
            ops.detect_blobs(x, [bad], None)
    with pytest.raises(ValueError):
        ops.detect_blobs(x[..., :2], [(0, -1, 0, 0, 96, 64)], None)
    with pytest.raises(ValueError):
        ops.warp_linear_bytes(x, [(1, -1)], None)
    with pytest.raises(ValueError):
        FF.detector_blobs(x, FF.detection_plan(64, 96, "Off (fastest)"))


def test_detect_with_rotation_reproduces_the_recorded_candidates(FF, BF):
    with open(D.golden_path()) as fh:
        golden = json.load(fh)
    ran = 0
    for case in golden["cases"]:
        if case["kind"] != "caffe":
            continue
        builder = case["module"] == "builder"
        dtype = "u8" if builder else "f32"
        x = D.make_frames("smooth", (2, case["height"], case["width"], 3), dtype, 11)
        plan = (BF.detection_plan(case["width"], case["height"], case["rotation_assist"], case["regions"]) if builder
                else FF.detection_plan(case["width"], case["height"], case["rotation_assist"]))
        rows = max(len(o) for per in case["outputs"] for o in per)
        recorded = np.zeros((len(plan.angles), plan.slots, rows, 7), dtype=np.float32)      # padding rows score 0: below every threshold
        for a, per in enumerate(case["outputs"]):
            for r, o in enumerate(per):
                if len(o):
                    recorded[a, r, :len(o)] = np.array(o, dtype=np.float32)
        small = case["width"] * case["height"] <= 640 * 420                                 # the restatement of the larger ones is slow
        if not small:
            want_blobs = None
        elif builder:
            mode = str(case["rotation_assist"] or "light").lower()
            want_blobs, _ = D.restated_blobs(x, mode if mode in D.ANGLES else "light", case["regions"] or D.regions_of(case["width"], case["height"], True))
        else:
            want_blobs, _ = D.restated_blobs(x, case["rotation_assist"] if case["rotation_assist"] in D.ANGLES else "Off (fastest)")
        seen = []

        def forward(blobs):
            seen.append(blobs)
            n = blobs.shape[0] // (len(plan.angles) * plan.slots)
            return torch.from_numpy(np.tile(recorded.reshape(-1, 1, rows, 7), (n, 1, 1, 1)))

        for frames in (torch.from_numpy(x).to(dev()), torch.from_numpy(x.copy())):
            if builder:
                got = BF.detect_with_rotation(forward, frames, case["confidence"], case["regions"], case["rotation_assist"])
            else:
                got = FF.detect_with_rotation(forward, frames, case["confidence"], case["minimum_pixels"], case["rotation_assist"])
            assert len(got) == 2
            for per_frame in got:
                assert [[float(v) for v in item] for item in per_frame] == case["candidates"], case["key"]
        assert len(seen) == 2 and tuple(seen[0].shape) == (2 * len(plan.angles) * plan.slots, 3, 300, 300)
        if small:
            assert same(f"{case['key']} blobs fed to the net", seen[0], want_blobs.reshape(-1, 3, 300, 300))
        ran += 1
    assert ran >= 6

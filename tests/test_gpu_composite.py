"""The feathered crop composite on the MI355X: csrc/vrg_composite.hip through the three nodes against the recorded reference results
(tests/golden/composite.npz) and, on shapes too large for a fixture, against the same arithmetic compiled for the host
(tests/host_math/composite_check.cpp, itself checked against the fixture by tests/test_composite_host.py).

What is asserted, for EVERY fixture case: the blend mask and the selected count equal the fixture bit for bit; where no statistic takes part
(strength 0, fewer than 16 selected pixels, the opaque node) the image does too; where one does, (1) the kernel's fp32 means equal the fp64
means of the fixture's own inputs rounded to fp32, (2) the image equals the host arithmetic given those means bit for bit, and (3) its
distance to the fixture d_gpu is at most the reference's own d_ref + 1 ulp(1.0).  Both distances are printed."""
import threading

import numpy as np
import pytest
import torch

import composite_support as CS

pytestmark = pytest.mark.gpu
CASES = CS.meta()["cases"]


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return CS.build_host_lib(tmp_path_factory.mktemp("composite_check"))


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def nodes(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_ImagePasteBack as PB
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes as FF
    return PB, FF


@pytest.fixture(scope="module")
def golden():
    return CS.arrays()


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def noisy(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 1.2 - 0.1).contiguous()


def bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().numpy()


def run_node(nodes, case, originals, crops, user_mask):
    PB, FF = nodes
    if case["node"] == "paste":
        crop_data = (tuple(case["crop_data"][0]), tuple(case["crop_data"][1]))
        return PB.VRGDG_ImagePasteBack().paste_back(originals, crops, crop_data, case["inset_padding"], case["feather_strength"],
                                                    case["blend_shape"], case["color_match"], mask=user_mask)
    ctx = {"original_frames": originals, "entries": case["entries"], "ltx_frame_offset": case["offset"], "job_id": "test"}
    if case["node"] == "facefix":
        res = FF.VRGDGFaceFixComposite().composite(crops, ctx, case["feather_pixels"], case["color_match"])
    else:
        res = FF.VRGDGFaceFixCompositeOpaque().composite(crops, ctx, case["feather_pixels"])
    assert res[2] == case["repaired"]
    return res


def device_stats(ops, call, entries_rule_match, user_mask):
    entries, rule, color_match = entries_rule_match
    rec = ops.composite_stats(torch.from_numpy(call.originals).to(dev()), torch.from_numpy(call.crops).to(dev()), entries, rule, color_match,
                              user_mask=None if user_mask is None else torch.from_numpy(user_mask).to(dev()))
    out = np.zeros((max(1, call.frames), CS.STATS_WORDS), dtype=np.uint32)
    f32 = out.view(np.float32)
    out[:call.frames, 0], out[:call.frames, 1] = bits(rec["count"]), bits(rec["matched"])
    f32[:call.frames, 2:6], f32[:call.frames, 6:10], f32[:call.frames, 10:14] = bits(rec["crop_mean"]), bits(rec["original_mean"]), bits(rec["shift"])
    return out


@pytest.mark.parametrize("where", ["cpu", "device", "inference_mode"])
@pytest.mark.parametrize("case", CASES, ids=[c["key"] for c in CASES])
def test_nodes_on_the_fixture(hm, ops, nodes, golden, case, where):
    key = case["key"]
    call = CS.case_call(hm, ops, case, golden)
    np_mask = golden[key + ".user_mask"] if case["user_mask"] else None
    originals, crops = torch.from_numpy(golden[key + ".originals"]), torch.from_numpy(golden[key + ".crops"])
    user_mask = None if np_mask is None else torch.from_numpy(np_mask)
    if where != "cpu":
        originals, crops, user_mask = originals.to(dev()), crops.to(dev()), None if user_mask is None else user_mask.to(dev())
    keep = [t.clone() for t in (originals, crops) + (() if user_mask is None else (user_mask,))]
    if where == "inference_mode":
        with torch.inference_mode():
            res = run_node(nodes, case, originals, crops, user_mask)
    else:
        res = run_node(nodes, case, originals, crops, user_mask)
    image, mask = res[0], res[1]
    assert image.is_cuda == (where != "cpu") and mask.is_cuda == (where != "cpu")
    for t, k in zip((originals, crops) + (() if user_mask is None else (user_mask,)), keep):
        assert torch.equal(t, k)                                                              # inputs unchanged
    assert CS.mismatches(bits(mask), golden[key + ".mask"]) == 0                              # the mask never depends on the statistic

    # condition 1: the statistic against the truth (fp64 means over the fixture's own selection, rounded to fp32)
    def selection(f):
        d = call.table[f]
        return golden[key + ".mask"][f, d.top:d.top + d.paste_h, d.left:d.left + d.paste_w] > np.float32(d.threshold)
    truth = call.truth_stats(selection)
    n_masks = 0 if np_mask is None else np_mask.shape[0]
    got = device_stats(ops, call, CS.case_entries(ops, case, call.originals.shape[0], call.crops.shape[0], n_masks), np_mask)
    assert [int(v) for v in got[:call.frames, 0]] == case["selected"]                        # the count is an integer and exact
    assert np.array_equal(got, truth)
    # condition 2: the pixels given the statistic
    expected, _ = call.apply(truth)
    assert CS.mismatches(bits(image), expected) == 0
    # condition 3: against the reference itself
    d_ref, d_gpu = CS.ulp_distance(golden[key + ".out"], expected), CS.ulp_distance(bits(image), expected)
    print(f"\n{key} [{where}]: d_ref = {d_ref} ulp(1.0), d_gpu = {d_gpu} ulp(1.0)")
    assert d_gpu <= d_ref + 1
    if not case["matched_frames"]:
        assert CS.mismatches(bits(image), golden[key + ".out"]) == 0                          # bit-equality wherever no statistic takes part


def large_cases():
    entries_4k = [{"original": 0, "crop": 0, "box": (1400, 500, 2424, 1524), "strength": 1.0}]
    return [
        ("4k_1024_box_from_512_crop_radial", (1, 2160, 3840, 3), (1, 512, 512, 3), None, entries_4k, ("radial", 18, 0), 0.65),
        ("4k_1024_box_opaque", (1, 2160, 3840, 3), (1, 512, 512, 3), None, entries_4k, ("opaque", 6, 0), 0.0),
        ("odd_widths_ellipse_masked_rgba", (2, 203, 331, 4), (2, 77, 91, 3), (1, 33, 29),
         [{"original": i, "crop": i, "mask": 0, "box": (37, 11, 37 + 251, 11 + 173)} for i in range(2)], ("ellipse", 24, 8), 0.65),
        ("box_touching_every_edge_rgba_crop", (1, 205, 333, 4), (1, 64, 96, 4), None,
         [{"original": 0, "crop": 0, "box": (0, 0, 333, 205)}], ("rectangle", 5, 3), 1.0),
        ("box_over_the_right_and_bottom_edge", (1, 201, 335, 3), (1, 300, 280, 3), None,
         [{"original": 0, "crop": 0, "box": (200, 120, 200 + 190, 120 + 140)}], ("ellipse", 0, 4), 0.65),
    ]


@pytest.mark.parametrize("name,o_shape,c_shape,m_shape,entries,rule,color_match", large_cases(), ids=[c[0] for c in large_cases()])
def test_large_shapes_equal_the_host_arithmetic(hm, ops, name, o_shape, c_shape, m_shape, entries, rule, color_match):
    originals, crops = noisy(o_shape, 31), noisy(c_shape, 32)
    user_mask = None if m_shape is None else (noisy(m_shape, 33) * 1.3).contiguous()
    rule = ops.CompositeRule(rule[0], feather=rule[1], inset=rule[2])
    call = CS.HostCall(hm, ops, originals.numpy(), crops.numpy(), entries, rule, color_match, None if user_mask is None else user_mask.numpy())
    truth = call.truth_stats()                                  # numpy fp64 means over the host arithmetic's resampled crop
    expected, expected_mask = call.apply(truth)
    o, c = originals.to(dev()), crops.to(dev())
    m = None if user_mask is None else user_mask.to(dev())
    image, mask = ops.composite_frames(o, c, entries, rule, color_match, user_mask=m)
    got = device_stats(ops, call, (entries, rule, color_match), None if user_mask is None else user_mask.numpy())
    assert np.array_equal(got[:, :2], truth[:, :2])
    assert np.array_equal(got, truth), (got.view(np.float32)[:, 2:14], truth.view(np.float32)[:, 2:14])
    assert CS.mismatches(bits(mask), expected_mask) == 0
    assert CS.mismatches(bits(image), expected) == 0
    assert torch.equal(o, originals.to(dev())) and torch.equal(c, crops.to(dev()))


def test_64_frames_with_their_own_boxes_equal_one_call_each(ops):
    frames, H, W = 64, 135, 241
    originals, work = noisy((frames, H, W, 3), 41).to(dev()), noisy((frames + 1, 48, 40, 3), 42).to(dev())
    rng = np.random.default_rng(7)
    entries = []
    for i in range(frames):
        w, h = int(rng.integers(1, 120)), int(rng.integers(1, 100))
        left, top = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        box = None if i % 9 == 4 else (left, top, left + w, top + h)
        entries.append({"original": i, "crop": i + 1, "box": box, "strength": (0.0, 0.5, 1.0, 1.0)[i % 4]})
    rule = ops.CompositeRule("radial", feather=7)
    image, mask = ops.composite_frames(originals, work, entries, rule, 0.65)
    stats = ops.composite_stats(originals, work, entries, rule, 0.65)
    assert int(stats["matched"].sum()) > 8
    for i in range(frames):
        one = [dict(entries[i], original=0)]
        image_i, mask_i = ops.composite_frames(originals[i:i + 1], work, one, rule, 0.65)
        assert torch.equal(image[i], image_i[0]) and torch.equal(mask[i], mask_i[0]), i
        stats_i = ops.composite_stats(originals[i:i + 1], work, one, rule, 0.65)
        for k in stats:
            assert torch.equal(stats[k][i], stats_i[k][0]), (i, k)


def test_stats_record_is_identical_over_three_calls(ops):
    originals, crops = noisy((3, 540, 960, 3), 51).to(dev()), noisy((3, 128, 128, 3), 52).to(dev())
    entries = [{"original": i, "crop": i, "box": (100 + 50 * i, 60, 100 + 50 * i + 400, 60 + 420), "strength": 1.0} for i in range(3)]
    rule = ops.CompositeRule("radial", feather=18)
    runs = [{k: v.clone() for k, v in ops.composite_stats(originals, crops, entries, rule, 0.65).items()} for _ in range(3)]
    assert int(runs[0]["matched"].sum()) == 3 and int(runs[0]["count"].min()) > 10000
    for other in runs[1:]:
        for k in runs[0]:
            assert torch.equal(runs[0][k].view(torch.int32), other[k].view(torch.int32)), k


def test_two_host_threads_at_once(nodes, golden):
    case = next(c for c in CASES if c["key"] == "facefix.offset_mixed")
    originals, crops = torch.from_numpy(golden[case["key"] + ".originals"]), torch.from_numpy(golden[case["key"] + ".crops"])
    results, errors = {}, []

    def run(k):
        try:
            for _ in range(4):
                results[k] = run_node(nodes, case, originals, crops, None)
        except Exception as exc:      # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert torch.equal(results[k][0], results[0][0]) and CS.mismatches(bits(results[k][1]), golden[case["key"] + ".mask"]) == 0


def test_paste_back_helpers_run_on_the_device(nodes, golden):
    PB, _ = nodes
    case = next(c for c in CASES if c["key"] == "paste.ellipse_up")
    box = case["crop_data"][1]
    alpha = PB._soft_blend_mask(box[3] - box[1], box[2] - box[0], case["inset_padding"], case["feather_strength"], "ellipse", dev(), torch.float32)
    want = golden[case["key"] + ".mask"][0, box[1]:box[3], box[0]:box[2]]
    assert alpha.is_cuda and CS.mismatches(bits(alpha), want) == 0
    source, target = noisy((40, 50, 3), 61).to(dev()), noisy((40, 50, 3), 62).to(dev())
    a = torch.rand((40, 50, 1), generator=torch.Generator().manual_seed(63)).to(dev())
    got = PB._match_color(source, target, a, 0.65)
    sel = (a[..., 0] > 0.25)
    shift = ((target[sel].double().mean(0).float() - source[sel].double().mean(0).float()) * 0.65)
    assert torch.equal(got, torch.clamp(source + shift, 0.0, 1.0))
    assert PB._match_color(source, target, a * 0.2, 0.65).equal(source) and PB._match_color(source, target, a, 0.0) is source


def test_host_fed_pieces_equal_the_device_result(nodes, pkg, monkeypatch, capsys):
    """CPU originals cut into several pieces by the staging pipeline (two frames each): an offset > 0, boxes that differ per frame, a
    no-face entry, and a preserved tail that begins inside a later piece -- frames, masks and count equal the device-tensor call, and
    the log lines are the reference's.  Paste Back with a batch of originals goes the same way."""
    PB, FF = nodes
    from comfyui_vrgamedevgirl_amd import _devices
    frames, H, W = 9, 120, 200
    originals, work = noisy((frames, H, W, 3), 71), noisy((8, 40, 36, 3), 72)
    entries = [{"box": (10 + 7 * i, 5 + 3 * i, 90 + 9 * i, 60 + 5 * i), "strength": (1.0, 0.5, 1.0)[i % 3]} for i in range(frames)]
    entries[3] = {"box": None, "strength": 1.0}
    entries[4] = {"box": (0, 0, 0, 0), "strength": 0.0}
    ctx = {"original_frames": originals, "entries": entries, "ltx_frame_offset": 3, "job_id": "pieces"}     # usable = 5: frames 5..8 are the tail
    monkeypatch.setattr(_devices, "PIPE_BYTES", 2 * H * W * 3 * 4)
    keep = originals.clone()
    for node, extra in ((FF.VRGDGFaceFixComposite(), (0.65,)), (FF.VRGDGFaceFixCompositeOpaque(), ())):
        if not extra:
            entries[4] = {"box": (3, 3, 3, 9)}
        capsys.readouterr()
        got = node.composite(work, ctx, 6, *extra)
        logged = capsys.readouterr().out
        want = node.composite(work.to(dev()), dict(ctx, original_frames=originals.to(dev())), 6, *extra)
        assert not got[0].is_cuda and not got[1].is_cuda and want[0].is_cuda
        assert torch.equal(got[0], want[0].cpu()) and torch.equal(got[1], want[1].cpu()) and got[2] == want[2] == 3
        assert torch.equal(got[0][5:], keep[5:].clamp(0, 1)) and not got[1][5:].any() and got[1][:3].any()
        assert torch.equal(originals, keep)
        if extra:
            assert logged == ("[VRGDG Face Fix] Composite started. Job=pieces; source_frames=9, LTX_frames=8, delta=4, feather=6, color_match=0.65.\n"
                              "[VRGDG Face Fix] Composite finished: repaired=3, unchanged=6, preserved_LTX_tail=4.\n")
        else:
            assert logged == "[VRGDG Face Fix] Opaque composite finished: repaired=3, unchanged=6, feather=6.\n"
    crops, user_mask = noisy((4, 30, 34, 3), 73), noisy((frames, 16, 18), 74)
    args = (((80, 70), (60, 30, 140, 100)), 4, 9, "ellipse", 0.65)
    got = PB.VRGDG_ImagePasteBack().paste_back(originals, crops, *args, mask=user_mask)
    want = PB.VRGDG_ImagePasteBack().paste_back(originals.to(dev()), crops.to(dev()), *args, mask=user_mask.to(dev()))
    assert not got[0].is_cuda and tuple(got[0].shape) == (frames, H, W, 3)
    assert torch.equal(got[0], want[0].cpu()) and torch.equal(got[1], want[1].cpu()) and torch.equal(originals, keep)

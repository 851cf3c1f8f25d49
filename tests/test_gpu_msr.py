"""The LTX MSR reference frames on the GPU (csrc/vrg_msr.hip): every value equals restated(...).astype(np.float32) / np.float32(255) of
tests/lanczos_support.py bit for bit, every repeat of it; the two nodes equal what the reference returned (tests/golden/msr_reference.npz).
Outputs start as NaN, so a float no store reached shows."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import lanczos_support as LS
import msr_support as M
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

#: (in_w, in_h, out_w, out_h, repeats of the picture): one source pixel; frames off the 16-byte grid (33 * 5 * 3 values); an enlargement
#: with a tile seam; a shrink above 3 (disjoint tap rows); a strong shrink along one axis; a picture that already has the size;
#: a source 8 wide: the one column position (s == 3) whose 24-byte window is the whole row, every other column gathers
GEOMETRIES = ((1, 1, 32, 32, 2), (7, 5, 33, 5, 3), (37, 53, 96, 64, 2), (301, 203, 64, 96, 2), (1024, 16, 32, 64, 1), (96, 64, 96, 64, 2),
              (8, 2, 16, 3, 1))
GUARD = 64                      # floats before and after the output inside the larger allocation


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def fixture():
    return np.load(M.FIXTURE)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    directory = tmp_path_factory.mktemp("msr_inputs")
    M.write_inputs(directory)
    return directory


@pytest.fixture()
def nodes(pkg, inputs):
    before = M.install_folder_paths(inputs)
    yield importlib.import_module(PKG_NAME + ".vrgdg_ltx_msr_reference_builder")
    M.restore_folder_paths(before)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def odd_copy(pic, dev):
    """the picture's bytes on the device at an odd byte address"""
    flat = torch.zeros(pic.size + 1, dtype=torch.uint8, device=dev)
    flat[1:] = torch.from_numpy(np.ascontiguousarray(pic).reshape(-1)).to(dev)
    assert flat.data_ptr() % 2 == 0
    return flat, flat.data_ptr() + 1


@pytest.mark.parametrize("in_w,in_h,out_w,out_h,repeats", GEOMETRIES)
def test_launch_equals_the_restatement(ops, in_w, in_h, out_w, out_h, repeats):
    """the launch itself: a picture at an odd address, a descriptor with no frames, a second picture of another size and a constant
    colour; the output lies one float into a larger NaN-filled allocation, so frames start off the 16-byte grid in every geometry and
    the floats around it must stay NaN"""
    from comfyui_vrgamedevgirl_amd import _hip
    dev = torch.device("cuda", 0)
    if in_w == 8:
        assert LS.has_both_column_kinds(ops.lanczos4_taps(in_h, in_w, out_h, out_w)["s"][:out_w], in_w)
    first = LS.random_frames((1, in_h, in_w, 3), 7 * in_w + in_h)[0]
    second = LS.smooth_frames((1, in_h + 3, in_w + 2, 3), 5)[0]
    colour = (3, 127, 252)
    plan = ops.msr_plan([first.shape[:2], first.shape[:2], second.shape[:2]], (out_w, out_h), 0, fill=colour)
    counts = [repeats, 0, 1, 2]
    desc = plan.desc.copy()
    desc["repeats"] = counts
    desc["first_frame"] = np.cumsum(counts) - counts
    frames = int(sum(counts))
    with torch.cuda.device(dev):
        keep_first, desc["src"][0] = odd_copy(first, dev)
        desc["src"][1] = desc["src"][0]
        keep_second = torch.from_numpy(second).to(dev)
        desc["src"][2] = keep_second.data_ptr()
        plan.frames = frames
        plan.check(desc)
        table = torch.from_numpy(plan.table()).to(dev)
        d = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(dev)
        n = frames * out_h * out_w * 3
        for lead in (GUARD, GUARD + 1):                      # the output on and off the 16-byte grid
            whole = torch.full((n + 2 * GUARD + 1,), float("nan"), dtype=torch.float32, device=dev)
            out = whole[lead:lead + n]
            _hip.check(_hip.lib().vrg_msr_frames_f32(_hip.ptr(d), len(desc), _hip.ptr(table), plan.n_taps, _hip.ptr(out), frames, out_h, out_w,
                                                     _hip.current_stream()), "vrg_msr_frames_f32")
            got = whole.cpu().numpy()
            want = M.expected_frames([first, first, second, colour], (out_w, out_h), counts)
            assert np.array_equal(bits(got[lead:lead + n]), bits(want.reshape(-1))), lead
            assert np.isnan(got[:lead]).all() and np.isnan(got[lead + n:]).all(), lead
    del keep_first, keep_second


def test_frame_counts_of_the_builder(ops):
    """17 frames from 3 pictures (6, 6, 5) and 41 from 5 (9, 8, 8, 8, 8), CPU and device pictures mixed, a picture as background"""
    dev = torch.device("cuda", 0)
    pics = [LS.random_frames((1, h, w, 3), 90 + i)[0] for i, (w, h) in enumerate(((37, 53), (64, 96), (301, 203), (7, 5), (50, 40)))]
    for n, frame_count, counts in ((3, 17, [6, 6, 5]), (5, 41, [9, 8, 8, 8, 8])):
        assert ops.expand_counts(n, frame_count) == counts
        given = [torch.from_numpy(p).to(dev) if i % 2 else p for i, p in enumerate(pics[:n - 1])]
        before = [p.copy() for p in pics]
        out = ops.msr_reference_frames(given, (64, 96), frame_count, background=torch.from_numpy(pics[n - 1]))
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (frame_count, 96, 64, 3)
        want = M.expected_frames(pics[:n], (64, 96), counts)
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
        assert all(np.array_equal(a, b) for a, b in zip(before, pics))                    # inputs are never written
    colour = ops.msr_reference_frames([pics[0]], (32, 32), 3, background=(127, 127, 127)).cpu().numpy()
    assert np.array_equal(bits(colour), bits(M.expected_frames([pics[0], (127, 127, 127)], (32, 32), [2, 1])))
    few = ops.msr_reference_frames(pics[:3], (32, 32), 2).cpu().numpy()                   # the third picture gets no frame
    assert np.array_equal(bits(few), bits(M.expected_frames(pics[:2], (32, 32), [1, 1])))
    assert tuple(ops.msr_reference_frames(pics[:1], (32, 32), 0).shape) == (0, 32, 32, 3)


def test_bytes_to_image(ops):
    for shape, seed in (((5, 7, 3), 1), ((96, 64, 3), 2), ((33, 130, 3), 3)):
        pic = LS.random_frames((1, *shape), seed)[0]
        out = ops.bytes_to_image(pic)
        assert out.is_cuda and tuple(out.shape) == (1, *shape)
        assert np.array_equal(bits(out.cpu().numpy()), bits(M.unit(pic)[None]))
    with pytest.raises(ValueError):
        ops.bytes_to_image(np.zeros((4, 4, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        ops.bytes_to_image(np.zeros((4, 4, 3), dtype=np.float32))


def test_builder_node_equals_the_reference(fixture, nodes):
    node = nodes.VRGDG_LTXMSRReferenceBuilder()
    for name, case in M.BUILDER_CASES.items():
        (out,) = node.build_reference(**case)
        assert isinstance(out, torch.Tensor) and out.device.type == "cpu" and out.dtype == torch.float32, name
        assert np.array_equal(bits(out.numpy()), bits(M.unit(fixture[f"builder.{name}"]))), name


def test_loader_node_equals_the_reference(fixture, nodes):
    node = nodes.VRGDG_LTX25MSRReferenceLoader()
    for name, case in M.LOADER_CASES.items():
        outs = node.load_references(**case)
        present = fixture[f"loader.{name}.present"].tolist()
        assert len(outs) == 5 and [o is not None for o in outs] == present, name
        for i, o in enumerate(outs):
            if o is not None:
                assert o.device.type == "cpu" and o.dtype == torch.float32, (name, i)
                assert np.array_equal(bits(o.numpy()), bits(M.unit(fixture[f"loader.{name}.{i}"]))), (name, i)
    with pytest.raises(ValueError, match=r"^background_image is required when background_mode is use_uploaded_background\.$"):
        node.load_references("a.png", M.NONE_IMAGE, M.NONE_IMAGE, M.NONE_IMAGE, M.NONE_IMAGE, "use_uploaded_background", 64, 32)


def test_msr_equals_cv2(ops):
    """equality with cv2 itself, wherever tests/golden/lanczos4_cv2.npz or the cv2 package exists"""
    if os.path.exists(LS.cv2_fixture_path()):
        data = np.load(LS.cv2_fixture_path())
        keys = json.loads(str(data["provenance"]))["cases"]
        cases = [(data[k + ".in"][0], data[k + ".out"][0]) for k in keys]
    else:
        cv2 = pytest.importorskip("cv2", reason="neither tests/golden/lanczos4_cv2.npz nor the cv2 package (opencv-python) is available")
        cases = []
        for in_w, in_h, out_w, out_h, _ in GEOMETRIES[:5]:
            pic = LS.random_frames((1, in_h, in_w, 3), 31)[0]
            cases.append((pic, cv2.resize(pic, (out_w, out_h), interpolation=cv2.INTER_LANCZOS4)))
    for pic, want in cases:
        out = ops.msr_reference_frames([pic], (want.shape[1], want.shape[0]), 2).cpu().numpy()
        assert np.array_equal(bits(out), bits(M.unit(np.stack([want, want]))))

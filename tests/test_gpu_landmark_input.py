"""The landmark estimator's input on the MI355X: vrg_face_thumbs_u8 against the numpy restatement of tests/landmark_input_support.py byte
for byte at every rule, with guard bytes round the output and the inputs unchanged; one launch of mixed descriptors at odd offsets with one
image past the end of the buffer; ops.face_bytes -> ops.face_thumbs; and VRGDGFaceFixCompositeLandmarkAligned through its thumbnail route
(`landmark_detector` / `transform_fit`) against its `estimator` route built from the same two functions, bit for bit, device-resident and
host-fed.  Reads nothing outside the repository."""
import ctypes as C

import numpy as np
import pytest
import torch

import landmark_input_support as L
from cut_support import smooth_frames

pytestmark = pytest.mark.gpu
FILL, GUARD = 0xA5, 64
SWEEP = [(box, mode) for box, mode, _ in L.GEOMETRIES + L.SEGMENTED]


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def hip(pkg):
    from comfyui_vrgamedevgirl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def FF(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes
    return VRGDG_StandaloneFaceFixNodes


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().numpy()


def launch(ops, hip, generated, source, jobs, n_bytes=None, check=True):
    """jobs [(which, offset, w, h)] through the C ABI: the output with its guards ([GUARD | n thumbnails | GUARD] uint8, FILL before)"""
    n_bytes = int(generated.numel()) if n_bytes is None else int(n_bytes)
    desc, tables, fix = ops.thumb_descriptors(jobs)
    records = torch.empty(desc.nbytes + tables.nbytes, dtype=torch.uint8, device=generated.device)
    for i, field, at in fix:
        desc[field][i] = records.data_ptr() + desc.nbytes + at
    lib = hip.lib()
    if check:
        assert lib.vrg_face_thumbs_check(C.c_void_p(desc.ctypes.data), len(desc), n_bytes, int(source is not None)) == hip.VRG_OK
    records.copy_(torch.from_numpy(np.concatenate([desc.view(np.uint8), tables])))
    out = torch.full((GUARD + len(jobs) * L.THUMB_BYTES + GUARD,), FILL, dtype=torch.uint8, device=generated.device)
    assert (out.data_ptr() + GUARD) % 16 == 0
    status = lib.vrg_face_thumbs_u8(hip.ptr(generated), hip.ptr(source) if source is not None else None, n_bytes, hip.ptr(records), len(desc),
                                    C.c_void_p(out.data_ptr() + GUARD), hip.current_stream())
    assert status == hip.VRG_OK
    torch.cuda.synchronize()
    return bits(out)


def split(raw, n):
    assert (raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all(), "a guard byte was written"
    return raw[GUARD:-GUARD].reshape(n, L.SIDE, L.SIDE, 3)


@pytest.mark.parametrize("box,mode", SWEEP, ids=[f"{h}x{w}" for (h, w), _ in SWEEP])
def test_abi_equals_the_restatement(ops, hip, box, mode):
    h, w = box
    assert ops.thumb_plan(h, w)[0] == mode
    kinds = L.KINDS if h * w <= 640 * 640 else ("uniform",)
    images = [L.make_box(kind, h, w, 7 + k) for k, kind in enumerate(kinds)]
    # generated holds the images at odd offsets one after the other, source the same images reversed in order
    size = h * w * 3
    offsets = [7 + k * (size + 1 - size % 2) for k in range(len(images))]
    total = offsets[-1] + size + 5
    gen, src = np.full(total, 0x3C, dtype=np.uint8), np.full(total, 0xC3, dtype=np.uint8)
    for k, image in enumerate(images):
        gen[offsets[k]:offsets[k] + size] = image.reshape(-1)
        src[offsets[k]:offsets[k] + size] = images[len(images) - 1 - k].reshape(-1)
    gen_dev, src_dev = torch.from_numpy(gen).to(dev()), torch.from_numpy(src).to(dev())
    jobs = [(which, offsets[k], w, h) for k in range(len(images)) for which in (0, 1)]
    got = split(launch(ops, hip, gen_dev, src_dev, jobs), len(jobs))
    want = [L.restated(image) for image in images]
    for k in range(len(images)):
        for which, expect in ((0, want[k]), (1, want[len(images) - 1 - k])):
            worst = int(np.abs(got[2 * k + which].astype(np.int16) - expect.astype(np.int16)).max())
            print(f"{h} x {w} {L.mode_name(mode)} {kinds[k]} which={which}: largest difference {worst} levels")
            assert np.array_equal(got[2 * k + which], expect), (kinds[k], which)
    assert np.array_equal(bits(gen_dev), gen) and np.array_equal(bits(src_dev), src)                # the inputs are never written


def test_one_launch_of_mixed_descriptors(ops, hip):
    """24 descriptors of mixed sizes and rules, both buffers, at odd offsets (boxes whose byte count is odd follow each other); one image
    lies past n_bytes: its thumbnail keeps the fill"""
    boxes = [(33, 47), (320, 320), (5, 3), (641, 333), (640, 640), (3, 3), (960, 640), (201, 399), (319, 321), (2, 2), (77, 1001), (1, 1)]
    rng = np.random.Generator(np.random.PCG64(11))
    offsets, at = [], 1
    for h, w in boxes:
        offsets.append(at)
        at += h * w * 3
    assert sum(o % 2 for o in offsets) >= 4 and sum(o % 16 != 0 for o in offsets) >= 10
    total = at
    gen = rng.integers(0, 256, total + 64, dtype=np.uint8)
    src = rng.integers(0, 256, total + 64, dtype=np.uint8)
    gen_dev, src_dev = torch.from_numpy(gen).to(dev()), torch.from_numpy(src).to(dev())
    jobs = [(which, offsets[i], w, h) for i, (h, w) in enumerate(boxes) for which in ((0, 1) if i % 2 == 0 else (1, 0))]
    assert len(jobs) == 24 and len({ops.thumb_plan(h, w)[0] for h, w in boxes}) == 5
    n_bytes = total - 1                                                                             # the last image ends one byte past it
    d = ops.thumb_descriptors(jobs)[0]
    d["xtab"] = d["ytab"] = 4096                                                                    # never dereferenced on the host
    assert hip.lib().vrg_face_thumbs_check(C.c_void_p(d.ctypes.data), 24, total, 1) == hip.VRG_OK   # the host check refuses exactly that image
    assert hip.lib().vrg_face_thumbs_check(C.c_void_p(d.ctypes.data), 24, n_bytes, 1) == hip.VRG_ERR_BAD_ARG
    got = split(launch(ops, hip, gen_dev, src_dev, jobs, n_bytes=n_bytes, check=False), len(jobs))
    for j, (which, offset, w, h) in enumerate(jobs):
        if offset + h * w * 3 > n_bytes:
            assert (got[j] == FILL).all(), j
            continue
        image = (gen, src)[which][offset:offset + h * w * 3].reshape(h, w, 3)
        assert np.array_equal(got[j], L.restated(image)), (j, which, h, w)
    assert sum(offset + h * w * 3 > n_bytes for _, offset, w, h in jobs) == 2
    assert np.array_equal(bits(gen_dev), gen) and np.array_equal(bits(src_dev), src)


def test_face_thumbs_of_face_bytes(ops):
    rng = np.random.Generator(np.random.PCG64(5))
    originals = torch.from_numpy(rng.random((5, 360, 400, 3), dtype=np.float32) * 1.2 - 0.1).to(dev())
    work = torch.from_numpy(rng.random((5, 48, 40, 3), dtype=np.float32) * 1.2 - 0.1).to(dev())
    boxes = [(10, 5, 340, 335), (336, 312, 400, 360), None, (100, 100, 140, 140), (7, 9, 12, 10)]   # 330 x 330, 64 x 48 at the corner, none, 40 x 40, 5 x 1
    rows = [{"original": i, "crop": i, "box": b} for i, b in enumerate(boxes)]
    faces = ops.face_bytes(work, rows, 360, 400, originals=originals)
    thumbs, index = ops.face_thumbs(faces)
    assert index == [0, 1, -1, 2, -1] and tuple(thumbs.shape) == (3, 2, L.SIDE, L.SIDE, 3) and thumbs.dtype == torch.uint8 and thumbs.is_cuda
    gen, src, got = bits(faces.generated), bits(faces.source), bits(thumbs)
    for f, row in enumerate(index):
        if row >= 0:
            assert np.array_equal(got[row, 0], L.restated(faces.image(src, f))) and np.array_equal(got[row, 1], L.restated(faces.image(gen, f))), f
    only, index_one = ops.face_thumbs(faces, ("generated",))
    assert index_one == index and np.array_equal(bits(only)[:, 0], got[:, 1])
    assert np.array_equal(bits(faces.generated), gen) and np.array_equal(bits(faces.source), src)
    # without device originals the caller brings the source bytes, or there are none
    alone = ops.face_bytes(work, rows, 360, 400)
    with pytest.raises(ValueError, match="no source bytes"):
        ops.face_thumbs(alone)
    brought, _ = ops.face_thumbs(alone, source=faces.source)
    assert np.array_equal(bits(brought), got)
    with pytest.raises(ValueError):
        ops.face_thumbs(faces, ("left",))
    empty, none = ops.face_thumbs(ops.face_bytes(work, [{"original": 0, "crop": 0, "box": None}], 360, 400, originals=originals))
    assert tuple(empty.shape) == (0, 2, L.SIDE, L.SIDE, 3) and none == [-1]


class Counted:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *args):
        self.calls += 1
        return self.fn(*args)


@pytest.mark.parametrize("where", ["device", "cpu"])
def test_node_routes_agree(FF, capsys, where):
    """the thumbnail route (the resize on the GPU, thumbnails downloaded) and the `estimator` route (both faces downloaded, the same resize
    by the numpy restatement) give the same bits: 5 frames with a hole, a hard_cut, a shot change, a frame without a face in the source
    and ltx_frame_offset = 1"""
    originals_np = np.clip(smooth_frames((5, 360, 400, 3), 21), 0.0, 1.0).astype(np.float32)
    originals_np[1, 5:335, 10:340] = 0.0                                                           # no face in the source of frame 1
    work_np = np.clip(smooth_frames((6, 48, 40, 3), 22), 0.02, 1.0).astype(np.float32)
    entries = [{"box": (10, 5, 340, 335), "shot_id": 0}, {"box": (10, 5, 340, 335), "shot_id": 0}, {"box": None, "shot_id": 0},
               {"box": (336, 312, 400, 360), "shot_id": 0, "hard_cut": True}, {"box": (100, 100, 140, 140), "shot_id": 1}]

    def run(route):
        originals, work = torch.from_numpy(originals_np.copy()), torch.from_numpy(work_np.copy())
        if where == "device":
            originals, work = originals.to(dev()), work.to(dev())
        ctx = {"original_frames": originals, "entries": [dict(e) for e in entries], "ltx_frame_offset": 1}
        detect, fit = Counted(L.steady_detector), Counted(L.similarity_fit)

        class Node(FF.VRGDGFaceFixCompositeLandmarkAligned):
            pass

        if route == "thumbnails":
            Node.landmark_detector, Node.transform_fit = staticmethod(detect), staticmethod(fit)
        else:
            def estimator(source_u8, generated_u8):
                h, w = source_u8.shape[:2]
                assert source_u8.shape == generated_u8.shape and source_u8.dtype == generated_u8.dtype == np.uint8
                found_source, found_generated = detect(L.restated(source_u8)), detect(L.restated(generated_u8))
                source_points, generated_points = FF.landmark_points(found_source, w, h), FF.landmark_points(found_generated, w, h)
                if source_points is None or generated_points is None:
                    return None
                return fit(generated_points, source_points)

            Node.estimator = staticmethod(estimator)
        capsys.readouterr()
        image, mask, repaired = Node().composite(work, ctx, 6, 0.75)
        logged = capsys.readouterr().out
        assert torch.equal(originals.cpu(), torch.from_numpy(originals_np)) and torch.equal(work.cpu(), torch.from_numpy(work_np))
        return bits(image), bits(mask), repaired, logged, detect.calls, fit.calls

    new, old = run("thumbnails"), run("estimator")
    assert new[2] == old[2] == 4 and new[3] == old[3] and "aligned=4, fallback=0," in new[3]       # frame 1 reuses frame 0's transform
    assert new[4] == old[4] == 8 and new[5] == old[5] == 3                                         # both faces always; a fit when both have points
    assert np.array_equal(new[0].view(np.uint32), old[0].view(np.uint32)) and np.array_equal(new[1].view(np.uint32), old[1].view(np.uint32))
    plain = FF.VRGDGFaceFixCompositeOpaque().composite(torch.from_numpy(work_np).to(dev()), {"original_frames": torch.from_numpy(originals_np).to(dev()),
                                                                                              "entries": entries, "ltx_frame_offset": 1}, 6)
    assert not np.array_equal(new[0], bits(plain[0]))                                              # the transforms did take part

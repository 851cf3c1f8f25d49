"""The multi-reference image batches on the GPU (csrc/vrg_refbatch.hip through ops.scale_reference_images, ops.batch_reference_images and
the node module): every picture of every case bit for bit (NaN by position) against torch itself, which runs the reference's expressions
in a child process on this machine's CPU with its plain kernels; the lanczos path against live Pillow.  Same operations in the same order
without contraction, so there is no tolerance.  Nothing reads a reference checkout."""
import importlib
import os

import numpy as np
import pytest
import torch

import refbatch_support as S
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def truth(tmp_path_factory):
    return S.torch_results(S.CASES, tmp_path_factory.mktemp("refbatch_torch"))


def _index(name):
    return next(i for i, c in enumerate(S.CASES) if c["name"] == name)


def _equal(got, want):
    assert [tuple(g.shape) for g in got] == [w.shape for w in want]
    return sum(S.same_bits(g.cpu().numpy(), w) for g, w in zip(got, want)) == 0


def test_tile_constant(ops):
    from comfyui_vrgamedevgirl_amd import _hip
    assert _hip.REFBATCH_TILE == S.TILE


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=[c["name"] for c in S.CASES])
def test_kernel_equals_torch(ops, truth, i):
    """the ragged call per method and budget, several frames, equal sizes with Inf and NaN, torch's kernel choice, the batch rule"""
    c = S.CASES[i]
    pictures = [p.cuda() for p in truth.inputs(i)]
    before = [p.clone() for p in pictures]
    got = S.run_case(ops, pictures, c)
    assert all(g.is_cuda and g.dtype == torch.float32 for g in got)
    assert _equal(got, truth.pictures(i)), (c["name"], truth.describe())
    assert all(S.same_bits(a.cpu().numpy(), b.cpu().numpy()) == 0 for a, b in zip(pictures, before))


def test_not_clamped(ops, truth):
    i = _index("ragged-bicubic-0.008")
    got = torch.cat([g.reshape(-1) for g in S.run_case(ops, [p.cuda() for p in truth.inputs(i)], S.CASES[i])]).cpu().numpy()
    want = np.concatenate([w.reshape(-1) for w in truth.pictures(i)])
    assert (want < 0).any() and (want > 1).any() and (got < 0).any() and (got > 1).any() and S.same_bits(got, want) == 0


def test_copy_passes_every_bit(ops, truth):
    """the picture that already fits: -0.0, a subnormal, Inf, -Inf and NaN come out unchanged, next to a channel of 1.0"""
    i = _index("rule-area")
    pictures = truth.inputs(i)
    got = ops.batch_reference_images([p.cuda() for p in pictures], "area").cpu().numpy()
    src = pictures[3].numpy()[0]
    assert got.shape == (4, 20, 37, 4) and S.same_bits(got[3][..., :3], src) == 0 and (got[3][..., 3] == 1).all()
    assert np.signbit(got[3][..., :3][src == 0]).any() and (got[3] == np.float32(1e-40)).any() and np.isinf(got[3]).sum() == 6
    assert S.same_bits(got[0][..., :3], pictures[0].numpy()[0]) == 0 and (got[0][..., 3] == 1).all()          # the base, re-padded


@pytest.mark.parametrize("method", S.FILTERS)
def test_dense_out_off_the_grid(ops, truth, method):
    """out=: the pictures back to back from an off-grid start of a larger zero-filled buffer; nothing around them changes"""
    i = _index(f"ragged-{method}-0.008")
    want = truth.pictures(i)
    total = sum(w.size for w in want)
    big = torch.zeros(total + 9, dtype=torch.float32, device="cuda")
    got = S.run_case(ops, [p.cuda() for p in truth.inputs(i)], S.CASES[i], out=big[5:])
    assert got[0].data_ptr() == big.data_ptr() + 20 and sum(g.data_ptr() % 16 != 0 for g in got) >= 3
    assert _equal(got, want)
    host = big.cpu().numpy()
    assert not host[:5].any() and not host[5 + total:].any()
    assert S.same_bits(host[5:5 + total], np.concatenate([w.reshape(-1) for w in want])) == 0
    with pytest.raises(ValueError):
        S.run_case(ops, [p.cuda() for p in truth.inputs(i)], S.CASES[i], out=big[:total - 1])


def test_batch_out(ops, truth):
    i = _index("rule-bilinear")
    want = truth.pictures(i)[0]
    big = torch.full((want.shape[0] + 2, *want.shape[1:]), 7.25, dtype=torch.float32, device="cuda")
    got = ops.batch_reference_images([p.cuda() for p in truth.inputs(i)], "bilinear", out=big[1:-1])
    assert got.data_ptr() == big[1:].data_ptr()
    host = big.cpu().numpy()
    assert S.same_bits(host[1:-1], want) == 0 and (host[0] == 7.25).all() and (host[-1] == 7.25).all()
    with pytest.raises(ValueError):
        ops.batch_reference_images([p.cuda() for p in truth.inputs(i)], "bilinear", out=big[:-1])


def test_host_fed_equals_device_resident(ops, truth):
    for name in ("ragged-bilinear-0.0005", "frames-area", "rule-bicubic"):
        i = _index(name)
        pictures = truth.inputs(i)
        mixed = [p.cuda() if k % 2 else p for k, p in enumerate(pictures)]
        for fed in (pictures, mixed):
            assert _equal(S.run_case(ops, fed, S.CASES[i]), truth.pictures(i)), name
    single = truth.inputs(_index("rule-area"))[1]
    assert ops.batch_reference_images([single], "area") is single
    assert ops.scale_reference_images([], "area") == []


def test_lanczos_equals_pillow(ops):
    """3-channel pictures of two sizes, two frames in one: quantise -> vrg_pil_resize_u8 -> bytes / 255 equals Pillow bytes / 255"""
    pytest.importorskip("PIL")
    c = S.scale_case("lanczos", ((1, 20, 37, 3), (2, 33, 29, 3)), "lanczos", 0.0005, seed=9)
    pictures = S.ref_pictures(c)
    for mp, steps in ((0.0005, 1), (0.008, 4)):
        sizes = [ops.total_pixels_size(p.shape[1], p.shape[2], mp, steps) for p in pictures]
        got = ops.scale_reference_images([pictures[0].cuda(), pictures[1]], "lanczos", mp, steps)
        assert _equal(got, S.pil_lanczos(pictures, sizes))
    x, y, w, h = ops.center_crop_rect(29, 33, 37, 20)
    batch = ops.batch_reference_images([p.cuda() for p in pictures], "lanczos").cpu().numpy()
    want = S.pil_lanczos([pictures[1][:, y:y + h, x:x + w]], [(20, 37)])[0]
    assert batch.shape == (3, 20, 37, 3) and S.same_bits(batch[:1], pictures[0].numpy()) == 0 and S.same_bits(batch[1:], want) == 0
    with pytest.raises(NotImplementedError, match="3-channel"):
        ops.scale_reference_images([torch.rand(1, 4, 4, 4).cuda()], "lanczos")


def test_bytes_to_images(ops):
    rng = np.random.default_rng(4)
    ramp = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3).astype(np.uint8)
    pictures = [ramp, rng.integers(0, 256, (7, 5, 3), dtype=np.uint8), rng.integers(0, 256, (33, 29, 3), dtype=np.uint8)]
    for fed in (pictures, [torch.from_numpy(p).cuda() for p in pictures]):
        got = ops.reference_bytes_to_images(fed)
        assert all(g.is_cuda and g.data_ptr() % 16 == 0 for g in got)
        assert _equal(got, [p.astype(np.float32)[None] / 255.0 for p in pictures])


class Fakes:
    def __init__(self):
        self.encoded, self.appended = [], []

    def encode(self, pixels):
        self.encoded.append(pixels)
        return torch.full((1, 16, 2, 2), float(len(self.encoded)), device=pixels.device)

    def append(self, conditioning, latent):
        self.appended.append((conditioning, latent["samples"]))
        return conditioning + "+"


@pytest.mark.parametrize("inference", (False, True))
def test_nodes_end_to_end(ops, pkg, truth, monkeypatch, tmp_path, inference):
    """the order of the encode calls, the encoded device pictures, the appended latents and the returned batch"""
    node = importlib.import_module(PKG_NAME + ".VRGDG_MultiReference")
    fakes = Fakes()
    monkeypatch.setattr(node, "conditioning_appender", fakes.append)
    i = _index("ragged-bicubic-0.0005")
    c = S.CASES[i]
    pictures = truth.inputs(i)
    rgb = [k for k, p in enumerate(pictures) if p.shape[3] == 3]                     # bilinear joins them; RGBA after RGB pictures cannot be
    images = {f"image{2 * n + 1}": pictures[k] for n, k in enumerate(rgb)}         # image2, image4, ... are not connected
    with torch.inference_mode(inference):
        pos, neg, batch = node.VRGDG_MultiReferenceConditioning().apply("P", "N", fakes, 2 * len(rgb), "bicubic", c["megapixels"], c["steps"], **images)
        want = [truth.pictures(i)[k] for k in rgb]
        assert len(fakes.encoded) == len(rgb) and all(e.is_cuda for e in fakes.encoded) and _equal(fakes.encoded, want)
        assert (pos, neg) == ("P" + "+" * len(rgb), "N" + "+" * len(rgb))
        assert [float(s.flatten()[0]) for _, s in fakes.appended] == [float(n // 2 + 1) for n in range(2 * len(rgb))]
        assert [t for t, _ in fakes.appended[:4]] == ["P", "N", "P+", "N+"]
        joined = ops.batch_reference_images(fakes.encoded, "bilinear")
        assert tuple(batch.shape) == (len(rgb), *want[0].shape[1:]) and S.same_bits(batch.cpu().numpy(), joined.cpu().numpy()) == 0
        assert S.same_bits(batch[:1].cpu().numpy(), want[0]) == 0

        files = {"a.png": (pictures[3][0].clamp(0, 1) * 255).to(torch.uint8).numpy(), "b.png": (pictures[6][0].clamp(0, 1) * 255).to(torch.uint8).numpy()}
        for name in files:
            (tmp_path / name).write_bytes(b"x")
        monkeypatch.setattr(node, "path_roots", lambda: [str(tmp_path)])
        monkeypatch.setattr(node, "image_loader", lambda path: files[os.path.basename(path)])
        loaded = [torch.from_numpy(files[n].astype(np.float32) / 255.0).unsqueeze(0) for n in ("a.png", "b.png")]
        (got,) = node.VRGDG_ImageBatchMultiFromPaths().load_batch('{"images": ["a.png", "b.png"]}', "area")
        assert S.same_bits(got.cpu().numpy(), ops.batch_reference_images(loaded, "area").cpu().numpy()) == 0
        del fakes.encoded[:]
        pos, neg, out = node.VRGDG_MultiReferenceConditioningFromPaths().apply("P", "N", fakes, "a.png\nb.png", "nearest-exact", 0.0005, 1)
        scaled = ops.scale_reference_images(loaded, "nearest-exact", 0.0005, 1)
        assert (pos, neg) == ("P++", "N++") and _equal(fakes.encoded, [s.cpu().numpy() for s in scaled])
        assert tuple(out.shape) == (2, *scaled[0].shape[1:])

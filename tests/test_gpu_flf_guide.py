"""The LTX First / Last guide on the GPU (csrc/vrg_flf.hip through ops.flf_guide_frames and the node): every frame of every case bit for
bit (NaN by position) against torch itself, which runs the reference's expressions in a child process on this machine's CPU with its
plain kernels.  Same operations in the same order without contraction, so there is no tolerance.  Nothing reads a reference checkout."""
import importlib
import types

import numpy as np
import pytest
import torch

import flf_support as S
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def truth(tmp_path_factory):
    return S.torch_results(S.CASES, tmp_path_factory.mktemp("flf_torch"))


def _index(name):
    return next(i for i, c in enumerate(S.CASES) if c["name"] == name)


def _run(ops, first, last, c, **kw):
    return ops.flf_guide_frames(first, last, c["frames"], c["start"], c["end"], c["curve"], **kw)


def test_chunk_constant(ops):
    assert ops.FLF_CHUNK == S.CHUNK


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=[c["name"] for c in S.CASES])
def test_kernel_equals_torch(ops, truth, i):
    c = S.CASES[i]
    first, last = truth.inputs(i)
    got = _run(ops, first.cuda(), last.cuda(), c)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == truth[i].shape
    assert S.same_bits(got.cpu().numpy(), truth[i]) == 0, (c["name"], truth.describe())


def test_specials_come_out_where_torch_puts_them(ops, truth):
    """equal sizes: the bits of `last` pass through (-0.0, a subnormal, Inf, NaN); a weight of 0 still multiplies"""
    i = _index("plain-specials")
    first, last = truth.inputs(i)
    got = _run(ops, first.cuda(), last.cuda(), S.CASES[i]).cpu().numpy()
    src = last.numpy()[0]
    finite = np.isfinite(src)
    assert (got[-1].view(np.uint32)[finite] == (first.numpy()[0] * np.float32(0) + src).view(np.uint32)[finite]).all()      # w0 = 0, w1 = 1
    assert (got[-1] == np.float32(1e-40)).any() and np.isnan(got[-1][np.isnan(src)]).all() and np.isinf(got[-1][np.isinf(src)]).all()
    assert np.isnan(got[0][np.isinf(src)]).all()                                                                              # 0 * Inf
    j = _index("first-specials")
    first, last = truth.inputs(j)
    got = _run(ops, first.cuda(), last.cuda(), S.CASES[j]).cpu().numpy()
    inf_at = np.isinf(first.numpy()[0])
    assert np.isinf(got[0][inf_at]).all() and np.isnan(got[-1][inf_at]).all()
    assert (np.isnan(got) == np.isnan(truth[j])).all()


def test_out_slice_off_the_grid(ops, truth):
    """out= a slice that starts at frame 1 of a batch of 105-float frames: an off-grid base pointer; nothing around it is touched"""
    i = _index("odd-33")
    c = S.CASES[i]
    first, last = truth.inputs(i)
    big = torch.full((c["frames"] + 3, 7, 5, 3), 7.25, dtype=torch.float32, device="cuda")
    out = big[1:1 + c["frames"]]
    assert out.data_ptr() % 16 != 0
    got = _run(ops, first.cuda(), last.cuda(), c, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = big.cpu().numpy()
    assert S.same_bits(host[1:1 + c["frames"]], truth[i]) == 0
    assert (host[0] == 7.25).all() and (host[1 + c["frames"]:] == 7.25).all()
    with pytest.raises(ValueError):
        _run(ops, first.cuda(), last.cuda(), c, out=big[:c["frames"], :, :, :2])


def test_host_fed_equals_device_resident(ops, truth):
    for name in ("rows-smoothstep", "odd-33", "down-4x-rgba"):
        i = _index(name)
        first, last = truth.inputs(i)
        for a, b in ((first, last), (first.cuda(), last), (first, last.cuda())):
            assert S.same_bits(_run(ops, a, b, S.CASES[i]).cpu().numpy(), truth[i]) == 0, name
    # only the first picture of a batch is taken
    first, last = truth.inputs(_index("rows-linear"))
    got = _run(ops, torch.cat([first, first + 1]), torch.cat([last, last * 2, last]), S.CASES[_index("rows-linear")])
    assert S.same_bits(got.cpu().numpy(), truth[_index("rows-linear")]) == 0


class _Recorder:
    def __init__(self, shape):
        self.shape, self.calls = shape, []

    def __call__(self, vae, width, height, guide_video, formula):
        self.calls.append(guide_video)
        return guide_video, torch.zeros(self.shape, dtype=torch.float32, device=guide_video.device)


@pytest.mark.parametrize("inference", (False, True))
def test_node_hands_the_encoder_the_device_batch(ops, pkg, truth, monkeypatch, inference):
    node = importlib.import_module(PKG_NAME + ".VRGDG_LTXFirstLastGuide")
    i = _index("rows-smoothstep")                      # 9 frames = (2 - 1) * 8 + 1, the node's default transition and curve
    c = S.CASES[i]
    assert (c["frames"], c["start"], c["end"], c["curve"]) == (9, 0.05, 0.90, "smoothstep")
    first, last = truth.inputs(i)
    rec = _Recorder((1, 128, 2, 1, 1))
    monkeypatch.setattr(node, "guide_encoder", rec)
    vae = types.SimpleNamespace(downscale_index_formula=(8, 32, 32))
    latent = {"samples": torch.zeros(1, 128, 2, 3, 5)}
    with torch.inference_mode(inference):
        _, _, out = node.VRGDG_LTXFirstLastGuide().add_first_last_guide("P", "N", vae, latent, first, last)
        video = rec.calls[0]
        assert video.is_cuda and S.same_bits(video.cpu().numpy(), truth[i]) == 0
        assert torch.equal(video, _run(ops, first, last, c))
        assert out["noise_mask"].is_cuda and tuple(out["noise_mask"].shape) == (1, 1, 2, 1, 1) and float(out["noise_mask"].flatten()[0]) == np.float32(1.0 - 0.35)

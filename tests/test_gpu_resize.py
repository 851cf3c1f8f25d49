"""Frame resize / Video Enhance restore on the MI355X: csrc/vrg_resize.hip against the recorded reference results
(tests/golden/resize.npz, torch's plain CPU kernels) and, on shapes too large for a fixture, against the same arithmetic compiled for the
host (tests/host_math/resize_check.cpp, itself bit-equal to the fixture: tests/test_resize_host.py) -- bit for bit everywhere.

Left out: a batch past 2^31 elements (a 4K RGB output of 87 frames, 8.6 GB, plus its host-side expected value does not fit the time
limit of a test run); frames are addressed with 64-bit offsets per frame as in the other entry points, and the in-frame offsets are
bounded by the entry point's own size check."""
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import resize_support as RS
from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")]

BICUBIC, BILINEAR, AREA, NEAREST = "Bicubic (recommended)", "Bilinear", "Area", "Nearest"
STRETCH, CROP, LETTERBOX = "Stretch to dimensions", "Crop to fill", "Fit with letterbox (preserve all)"


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return RS.build_host_lib(tmp_path_factory.mktemp("resize_check"))


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def ven(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_VideoEnhanceNodes
    return VRGDG_VideoEnhanceNodes


@pytest.fixture(scope="module")
def golden():
    return RS.arrays()


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def frames(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 1.2 - 0.1).contiguous()


def same_bits(got: torch.Tensor, want) -> int:
    return RS.mismatches(torch.as_tensor(got).detach().cpu().contiguous().numpy(), np.asarray(want))


def test_resize_fixtures_bit_equal(ops, ven, golden):
    for c in RS.META["resize"]:
        x = torch.from_numpy(golden[c["in"]])
        keep = x.clone()
        got = ops.resize_frames(x.to(dev()), c["target_width"], c["target_height"], c["fit_mode"], c["resize_method"])
        assert same_bits(got, golden[c["key"]]) == 0, c
        via_node = ven._resize_batch(x, c["target_width"], c["target_height"], c["fit_mode"], c["resize_method"])      # CPU in, CPU out
        assert not via_node.is_cuda and same_bits(via_node, golden[c["key"]]) == 0, c
        assert torch.equal(x, keep)
    for c in RS.META["restore_batch"]:
        x = torch.from_numpy(golden[c["in"]]).to(dev())
        got = ven._restore_batch(x, c["source_width"], c["source_height"], c["fit_mode"], c["resize_method"])          # device in, device out
        assert got.is_cuda and same_bits(got, golden[c["key"]]) == 0, c


@pytest.mark.parametrize("where", ["cpu", "device", "inference_mode"])
def test_restore_node_fixtures_bit_equal(ven, golden, where):
    node = ven.VRGDGVideoEnhanceRestoreOriginal()
    for c in RS.META["restore"]:
        work, originals = torch.from_numpy(golden[c["key"] + ".work"]), torch.from_numpy(golden[c["key"] + ".originals"])
        if where != "cpu":
            work, originals = work.to(dev()), originals.to(dev())
        keep_w, keep_o = work.clone(), originals.clone()
        ctx = {"original_frames": originals, "source_width": int(originals.shape[2]), "source_height": int(originals.shape[1]),
               "frame_count": c["frame_count"], "fit_mode": c["fit_mode"], "fps": 24.0}
        if where == "inference_mode":
            with torch.inference_mode():
                out = node.restore(work, ctx, c["resize_method"], c["strength"])
        else:
            out = node.restore(work, ctx, c["resize_method"], c["strength"])
        assert out[0].is_cuda == (where != "cpu")
        assert same_bits(out[0], golden[c["key"] + ".out"]) == 0, c
        assert list(out[1:]) == c["returns"]
        assert torch.equal(work, keep_w) and torch.equal(originals, keep_o)            # inputs unchanged


LARGE = [("1080p_to_4k_bicubic", (1, 1080, 1920, 3), 3840, 2160, STRETCH, BICUBIC),
         ("4k_to_768x432_area", (1, 2160, 3840, 3), 768, 432, STRETCH, AREA),
         ("odd_width_bilinear", (2, 201, 333, 4), 1001, 603, STRETCH, BILINEAR),
         ("odd_width_nearest_crop", (2, 201, 333, 3), 1001, 515, CROP, NEAREST),
         ("odd_width_bicubic_letterbox", (2, 201, 333, 3), 1001, 719, LETTERBOX, BICUBIC),
         ("down_bicubic_crop", (1, 1080, 1920, 4), 483, 401, CROP, BICUBIC)]


@pytest.mark.parametrize("name,shape,tw,th,fit,method", LARGE, ids=[c[0] for c in LARGE])
def test_resize_large_shapes_equal_the_host_arithmetic(hm, ops, name, shape, tw, th, fit, method):
    x = frames(shape, 11)
    g = ops.resize_geometry(shape[1], shape[2], tw, th, fit)
    want = RS.host_resize(hm, ops, x.numpy(), g, method)
    got = ops.resize_frames(x.to(dev()), tw, th, fit, method)
    assert tuple(got.shape) == want.shape and same_bits(got, want) == 0


@pytest.mark.parametrize("strength", [1.0, 0.5])
def test_letterbox_undo_960x544_to_4k_restore(hm, ops, strength):
    """the node's default geometry: 960 x 544 working frames (16:9 content inside a letterbox) back to 3840 x 2160, fused with the blend;
    3 working frames for 4 originals, so the last original is the preserved tail"""
    work, originals = frames((3, 544, 960, 3), 5), frames((4, 2160, 3840, 3), 6)
    g = ops.restore_geometry(544, 960, 3840, 2160, LETTERBOX)
    assert g.src == (0, 2, 960, 540)
    want = RS.host_restore(hm, ops, work.numpy(), originals.numpy(), g, BICUBIC, strength, 3)
    got = ops.restore_frames(work.to(dev()), originals.to(dev()), 3840, 2160, LETTERBOX, BICUBIC, strength, 4)
    assert same_bits(got, want) == 0


@pytest.mark.parametrize("method", [BICUBIC, BILINEAR, AREA, NEAREST])
@pytest.mark.parametrize("channels", [3, 4])
def test_fused_restore_equals_resize_then_torch_blend(ops, method, channels):
    """bit-equal: the blend is three single-rounding ops (two products, one sum) and a clamp, done here with torch ops on the device"""
    strength = 0.35
    work, originals = frames((5, 136, 240, 3), 7).to(dev()), frames((7, 405, 721, channels), 8).to(dev())
    restored = ops.resize_geometry_frames(work, ops.restore_geometry(136, 240, 721, 405, LETTERBOX), method)
    want = originals.clone()
    want[:5, ..., :3] = originals[:5, ..., :3] * (1.0 - strength) + restored * strength
    want = want.clamp(0, 1)
    got = ops.restore_frames(work, originals, 721, 405, LETTERBOX, method, strength)
    assert torch.equal(got, want)


def test_two_host_threads_at_once(ven, golden):
    node = ven.VRGDGVideoEnhanceRestoreOriginal()
    c = RS.META["restore"][1]
    work, originals = torch.from_numpy(golden[c["key"] + ".work"]), torch.from_numpy(golden[c["key"] + ".originals"])
    ctx = {"original_frames": originals, "frame_count": c["frame_count"], "fit_mode": c["fit_mode"]}
    results, errors = {}, []

    def run(k):
        try:
            for _ in range(4):
                results[k] = node.restore(work, ctx, c["resize_method"], c["strength"])[0]
        except Exception as exc:      # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert same_bits(results[k], golden[c["key"] + ".out"]) == 0


_CHILD = r"""
import sys, numpy as np, torch, torch.nn.functional as F
x = torch.from_numpy(np.load(sys.argv[1]))
out = {m: F.interpolate(x.permute(0, 3, 1, 2), size=(int(sys.argv[3]), int(sys.argv[4])), mode=m,
                        **({"align_corners": False} if m in ("bilinear", "bicubic") else {})).permute(0, 2, 3, 1).clamp(0, 1).contiguous().numpy()
       for m in ("bicubic", "bilinear", "area", "nearest")}
np.savez(sys.argv[2], capability=np.array(torch.backends.cpu.get_cpu_capability()), **out)
"""


def test_distance_to_in_process_torch_is_torch_s_own(ops, tmp_path):
    """Informational, asserted only as far as it can be: F.interpolate run in THIS process on the CPU uses whatever vector build torch
    dispatches to here, which differs from torch's own plain build (ATEN_CPU_CAPABILITY=default, run in a child process) by a few
    ulp(1.0).  The kernels equal the plain build, so their distance to the in-process result must not exceed the plain build's own."""
    import torch.nn.functional as F
    x = frames((1, 270, 480, 3), 21)
    np.save(tmp_path / "x.npy", x.numpy())
    env = dict(os.environ, ATEN_CPU_CAPABILITY="default")
    subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path / "x.npy"), str(tmp_path / "plain.npz"), "1080", "1920"], check=True, env=env, cwd=ROOT)
    plain = np.load(tmp_path / "plain.npz")
    ulp = 2.0 ** -23
    print(f"\nin-process torch CPU capability: {torch.backends.cpu.get_cpu_capability()}; child: {plain['capability']}")
    for widget, mode in ((BICUBIC, "bicubic"), (BILINEAR, "bilinear"), (AREA, "area"), (NEAREST, "nearest")):
        kw = {"align_corners": False} if mode in ("bilinear", "bicubic") else {}
        here = F.interpolate(x.permute(0, 3, 1, 2), size=(1080, 1920), mode=mode, **kw).permute(0, 2, 3, 1).clamp(0, 1).contiguous().numpy()
        got = ops.resize_frames(x.to(dev()), 1920, 1080, STRETCH, widget).cpu().numpy()
        ours = float(np.abs(got.astype(np.float64) - here).max()) / ulp
        torchs = float(np.abs(plain[mode].astype(np.float64) - here).max()) / ulp
        differing = float((got != here).mean())
        print(f"{mode}: kernel vs in-process torch {ours:.2f} ulp(1.0) ({100 * differing:.1f} % of the elements differ); "
              f"torch default vs in-process torch {torchs:.2f} ulp(1.0); kernel vs torch default: {RS.mismatches(got, plain[mode])} elements")
        assert ours <= torchs

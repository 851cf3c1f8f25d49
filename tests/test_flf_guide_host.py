"""The LTX First / Last guide without a GPU: csrc/vrg_flf_math.hpp compiled for the host against torch itself (run live, plain CPU
kernels), the host plan against the reference's own loop and the recorded fixture, the node's surface and data flow, the ABI."""
import ast
import ctypes as C
import importlib
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import flf_support as S
from conftest import PKG_NAME, ROOT

REFERENCE_FILE = os.path.join(os.environ.get("VRGDG_REFERENCE_ROOT", "/root/reference"), "VRGDG_LTXFirstLastGuide.py")


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext, ops
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return ops


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return S.build_host_lib(tmp_path_factory.mktemp("flf_host"))


@pytest.fixture(scope="module")
def truth(tmp_path_factory):
    return S.torch_results(S.CASES, tmp_path_factory.mktemp("flf_torch"))


@pytest.fixture()
def node(pkg):
    return importlib.import_module(PKG_NAME + ".VRGDG_LTXFirstLastGuide")


def test_chunk_constant(ops):
    from comfyui_vrgamedevgirl_amd import _hip
    text = open(os.path.join(ROOT, "comfyui-vrgamedevgirl_amd", "csrc", "vrg_flf_math.hpp")).read()
    assert f"constexpr int FLF_CHUNK = {S.CHUNK};" in text and _hip.FLF_CHUNK == S.CHUNK == ops.FLF_CHUNK


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=[c["name"] for c in S.CASES])
def test_header_equals_torch(ops, host, truth, i):
    """every frame of every case, bit for bit (NaN by position), against the reference's expressions executed by torch"""
    c = S.CASES[i]
    first, last = truth.inputs(i)
    got, want = S.host_guide(host, ops, first, last, c), truth[i]
    assert want.shape == (c["frames"], *c["first"][1:])
    assert S.same_bits(got, want) == 0, (c["name"], truth.describe())


def test_the_cases_reach_what_they_are_for(ops, truth):
    """specials survive into the expectation as NaN and Inf; the weight 0 frames exist; the kernel-choice cases lie on both sides"""
    by_name = {c["name"]: i for i, c in enumerate(S.CASES)}
    want = truth[by_name["first-specials"]]
    w = ops.flf_weights(9, 0.5, 0.90, "linear")
    assert (w[:4, 1] == 0).all() and w[-1, 0] == 0 and w[-1, 1] == 1
    first, _ = truth.inputs(by_name["first-specials"])
    inf_at = np.isinf(first.numpy()[0])
    assert inf_at.sum() >= 4 and np.isnan(want[-1][inf_at]).all() and np.isinf(want[0][inf_at]).all()       # 0 * Inf = NaN in the last frame only
    plain = truth[by_name["plain-specials"]]
    _, last = truth.inputs(by_name["plain-specials"])
    assert np.isnan(plain[0][np.isinf(last.numpy()[0])]).all()                                               # w1 = 0 in frame 0
    sub = np.float32(1e-40)
    assert sub != 0 and (last.numpy() == sub).any() and (plain[-1] == sub).any()                           # the subnormal passes unflushed
    for name, (h, w_, c), paired in (("sum-128", (64, 64, 3), True), ("sum-129", (64, 65, 3), False)):
        assert S.CASES[by_name[name]]["first"][1:] == [h, w_, c] and (h + w_ <= 128) == paired


def test_weights_equal_the_reference_loop_and_the_fixture(ops):
    for rec in S.FIXTURE["weights"]:
        got = ops.flf_weights(rec["frame_count"], rec["transition_start"], rec["transition_end"], rec["curve"])
        assert got.dtype == np.float32 and got.shape == (rec["frame_count"], 2)
        assert np.array_equal(got, np.array(rec["weights"], dtype=np.float32)), rec
    pts = S.FIXTURE["curves"]["points"]
    for name, values in S.FIXTURE["curves"]["values"].items():
        assert [ops.flf_curve(p, name) for p in pts] == values, name
    with pytest.raises(ValueError):
        ops.flf_weights(0)


class _Recorder:
    """stands in for LTXVAddGuide.encode: keeps what it is handed, returns a latent of the asked shape"""

    def __init__(self, shape, dtype=torch.float16):
        self.shape, self.dtype, self.calls = tuple(shape), dtype, []

    def __call__(self, vae, width, height, guide_video, formula):
        self.calls.append({"vae": vae, "width": width, "height": height, "frames": guide_video, "formula": formula})
        return guide_video, torch.zeros(self.shape, dtype=self.dtype)


@pytest.mark.skipif(not os.path.isfile(REFERENCE_FILE), reason="no reference checkout")
def test_weights_equal_the_reference_class_run_live(ops):
    """the reference's class, taken from its source by the AST and executed: its guide batch of 1 x 1 pictures (1, 0) and (0, 1) IS the
    weight table"""
    with open(REFERENCE_FILE, encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=REFERENCE_FILE)
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "VRGDG_LTXFirstLastGuide"]
    rec = _Recorder((1, 4, 1, 1, 1))
    ns = {"torch": torch, "comfy": None, "LTXVAddGuide": types.SimpleNamespace(encode=rec)}
    exec(compile(ast.Module(body=body, type_ignores=[]), REFERENCE_FILE, "exec"), ns)
    first, last = torch.tensor([1.0, 0.0, 0.5]).reshape(1, 1, 1, 3), torch.tensor([0.0, 1.0, 0.5]).reshape(1, 1, 1, 3)
    for length, start, end, curve in ((2, 0.05, 0.90, "smoothstep"), (13, 0.3, 0.6, "ease_out"), (16, 0.0, 1.0, "ease_in"), (4, 0.5, 0.9, "linear")):
        frames = (length - 1) * 8 + 1
        rec.shape = (1, 4, length, 1, 1)
        vae = types.SimpleNamespace(downscale_index_formula=(8, 32, 32))
        ns["VRGDG_LTXFirstLastGuide"]().add_first_last_guide(None, None, vae, {"samples": torch.zeros(1, 4, length, 1, 1)}, first, last,
                                                             transition_start=start, transition_end=end, curve=curve)
        video = rec.calls[-1]["frames"].reshape(frames, 3).numpy()
        assert np.array_equal(ops.flf_weights(frames, start, end, curve), video[:, :2]), (frames, start, end, curve)


def test_center_crop_rect_equals_the_fixture(ops):
    for rec in S.FIXTURE["rects"]:
        (old_w, old_h), (new_w, new_h) = rec["old"], rec["new"]
        got = ops.center_crop_rect(old_w, old_h, new_w, new_h)
        assert list(got) == (rec["rect"] or [0, 0, old_w, old_h]), rec
    assert sum(r["half"] for r in S.FIXTURE["rects"]) >= 2


def test_the_half_pair_really_lands_on_a_half(ops):
    """HALF_PAIR: half the surplus is exactly 2.5 -- Python's round gives 2, round-half-up would give 3"""
    old_w, old_h, new_w, new_h = S.HALF_PAIR
    half = (old_w - old_w * ((new_w / new_h) / (old_w / old_h))) / 2
    assert half == 2.5 and round(half) == 2 and int(half + 0.5) == 3
    assert ops.center_crop_rect(*S.HALF_PAIR) == (2, 0, 5, 4)
    c = next(c for c in S.CASES if c["name"] == "half-rect")
    assert (c["last"][2], c["last"][1], c["first"][2], c["first"][1]) == S.HALF_PAIR


def test_center_crop_rect_equals_comfy():
    """unpinned unless ComfyUI is installed: the narrowing of the real comfy.utils.common_upscale, read off the view it resamples"""
    comfy_utils = pytest.importorskip("comfy.utils")
    from comfyui_vrgamedevgirl_amd import ops
    for rec in S.FIXTURE["rects"]:
        (old_w, old_h), (new_w, new_h) = rec["old"], rec["new"]
        if old_w * old_h > 1 << 16:
            continue
        ramp = torch.arange(old_h * old_w, dtype=torch.float32).reshape(1, 1, old_h, old_w)
        x, y, w, h = ops.center_crop_rect(old_w, old_h, new_w, new_h)
        want = torch.nn.functional.interpolate(ramp[:, :, y:y + h, x:x + w], size=(new_h, new_w), mode="bilinear")
        assert torch.equal(comfy_utils.common_upscale(ramp, new_w, new_h, "bilinear", "center"), want), rec


def test_surface_equals_the_reference(node, pkg):
    want = S.FIXTURE["surface"]
    cls = node.VRGDG_LTXFirstLastGuide
    import json
    assert json.loads(json.dumps(cls.INPUT_TYPES())) == want["INPUT_TYPES"]
    assert list(cls.INPUT_TYPES()["required"]) == list(want["INPUT_TYPES"]["required"])
    assert [list(cls.RETURN_TYPES), list(cls.RETURN_NAMES), cls.FUNCTION, cls.CATEGORY] == \
        [want["RETURN_TYPES"], want["RETURN_NAMES"], want["FUNCTION"], want["CATEGORY"]]
    assert node.NODE_CLASS_MAPPINGS == {"VRGDG_LTXFirstLastGuide": cls}
    assert node.NODE_DISPLAY_NAME_MAPPINGS == {"VRGDG_LTXFirstLastGuide": want["display_name"]}
    pts = S.FIXTURE["curves"]["points"]
    for name, values in S.FIXTURE["curves"]["values"].items():
        assert [cls._curve(p, name) for p in pts] == values
    # the package's merged mappings keep their pinned key set
    assert "VRGDG_LTXFirstLastGuide" not in pkg.NODE_CLASS_MAPPINGS and "VRGDG_LTXFirstLastGuide" not in pkg.NODE_DISPLAY_NAME_MAPPINGS


def test_module_imports_without_comfyui(pkg):
    code = ("import sys; sys.path.insert(0, %r); import conftest; conftest.load_package(); import importlib; "
            "m = importlib.import_module(conftest.PKG_NAME + '.VRGDG_LTXFirstLastGuide'); "
            "assert not [n for n in sys.modules if n.split('.')[0] in ('comfy', 'comfy_extras', 'folder_paths')]; "
            "assert len(m.NODE_CLASS_MAPPINGS) == 1 and callable(m.guide_encoder)") % os.path.join(ROOT, "tests")
    ran = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stderr


def test_node_data_flow_with_a_recording_encoder(node, ops, host, monkeypatch):
    """frame count, what the encoder is handed, the latent dictionary, the noise mask and both refusals, as recorded from the reference.
    No GPU here: the op is stood in for by the host-compiled header, called with the op's own arguments."""
    want = S.FIXTURE["node"]

    def on_host(first, last, frame_count, transition_start=0.05, transition_end=0.90, curve="smoothstep", out=None):
        c = {"frames": frame_count, "start": transition_start, "end": transition_end, "curve": curve}
        return torch.from_numpy(S.host_guide(host, ops, first, last, c))

    monkeypatch.setattr(ops, "flf_guide_frames", on_host)
    rec = _Recorder(want["encoded_shape"])
    monkeypatch.setattr(node, "guide_encoder", rec)
    vae = types.SimpleNamespace(downscale_index_formula=(want["time_scale"], 32, 32))
    latent = {"samples": torch.zeros(want["latent_shape"]), "batch_index": [0]}
    first, last = torch.rand(3, 4, 6, 3), torch.rand(2, 4, 6, 3)
    pos, neg, got = node.VRGDG_LTXFirstLastGuide().add_first_last_guide("P", "N", vae, latent, first, last, guide_strength=want["guide_strength"])
    call = rec.calls[0]
    assert [pos, neg] == want["returns"] and sorted(got) == want["keys"] and "noise_mask" not in latent
    assert (call["width"], call["height"], list(call["frames"].shape)) == (want["encoder"]["width"], want["encoder"]["height"], want["encoder"]["frames_shape"])
    assert call["vae"] is vae and call["formula"] is vae.downscale_index_formula
    expected = torch.cat([first[:1] * (1.0 - a) + last[:1] * a for a in ops.flf_weights(33).astype(np.float64)[:, 1]])
    assert call["frames"].shape == expected.shape
    assert list(got["samples"].shape) == want["samples_shape"] and got["batch_index"] == [0]
    mask = got["noise_mask"]
    assert list(mask.shape) == want["noise_mask"]["shape"] and str(mask.dtype) == want["noise_mask"]["dtype"]
    assert (mask == want["noise_mask"]["value"]).all()
    for strength, value in want["strengths"]:
        rec.shape = (1, 128, 1, 2, 3)
        _, _, r = node.VRGDG_LTXFirstLastGuide().add_first_last_guide("P", "N", vae, {"samples": torch.zeros(1, 128, 1, 4, 6)}, first, last,
                                                                       guide_strength=strength)
        assert float(r["noise_mask"].flatten()[0]) == value
    for error in want["errors"].values():
        rec.shape = tuple(error["encoded_shape"])
        with pytest.raises(ValueError) as caught:
            node.VRGDG_LTXFirstLastGuide().add_first_last_guide("P", "N", vae, latent, first, last)
        assert str(caught.value) == error["message"]


def test_operator_refusals(ops):
    """the reference's failures, as ValueError, before anything goes to a device"""
    ok = torch.zeros(1, 4, 6, 3)
    for first, last, frames in ((torch.zeros(4, 6, 3), ok, 9), (ok, torch.zeros(0, 4, 6, 3), 9), (ok, torch.zeros(1, 4, 6, 4), 9),
                                (torch.zeros(1, 4, 6, 2), torch.zeros(1, 4, 6, 2), 9), (torch.zeros(1, 4, 6, 5), torch.zeros(1, 4, 6, 5), 9),
                                (ok, ok, 0), (ok, ok.double(), 9), (ok, torch.zeros(1, 0, 6, 3), 9)):
        with pytest.raises(ValueError):
            ops.flf_guide_frames(first, last, frames)
    rect, weights = ops.flf_plan((7, 5, 3), (5, 13, 3), 33)
    assert rect == (5, 0, 3, 5) == ops.center_crop_rect(13, 5, 5, 7)
    assert ops.flf_plan((7, 5, 3), (7, 5, 3), 2)[0] == (0, 0, 5, 7) and weights.shape == (33, 2)


def test_abi(ops):
    """both symbols are declared, exported and bound; vrg_flf_check's refusals; the launch entry refuses null pointers and takes zero
    frames without a device"""
    from comfyui_vrgamedevgirl_amd import _hip
    header = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    lib = _hip.load_library()
    for name in ("vrg_flf_check", "vrg_flf_guide_f32"):
        assert name + "(" in header and name in _hip.EXPORTED_SYMBOLS and hasattr(lib._cdll, name)
    assert lib.vrg_abi_version() == 8
    check = lib.vrg_flf_check
    assert check(9, 7, 5, 3, 5, 13, 5, 0, 3, 5) == 0 and check(0, 7, 5, 3, 7, 5, 0, 0, 5, 7) == 0
    assert check(9, 7, 5, 4, 5, 13, 0, 0, 13, 5) == 0
    for bad in ((-1, 7, 5, 3, 5, 13, 5, 0, 3, 5),                      # negative frames
                (9, 7, 5, 2, 5, 13, 5, 0, 3, 5), (9, 7, 5, 5, 5, 13, 5, 0, 3, 5),            # channels 2 / 5
                (9, 0, 5, 3, 5, 13, 5, 0, 3, 5), (9, 7, 0, 3, 5, 13, 5, 0, 3, 5), (9, 7, 5, 3, 0, 13, 5, 0, 3, 5), (9, 7, 5, 3, 5, 0, 0, 0, 1, 1),
                (9, 7, 5, 3, 5, 13, 11, 0, 3, 5), (9, 7, 5, 3, 5, 13, 5, 1, 3, 5),           # the rectangle passes the right / lower edge
                (9, 7, 5, 3, 5, 13, -1, 0, 3, 5), (9, 7, 5, 3, 5, 13, 0, -1, 3, 5),
                (9, 7, 5, 3, 5, 13, 5, 0, 0, 5), (9, 7, 5, 3, 5, 13, 5, 0, 3, 0),
                (9, 7, 5, 3, 5, 13, 2 ** 31 - 1, 0, 3, 5)):
        assert check(*bad) == 1, bad
    assert check(9, 46341, 46341, 3, 1, 1, 0, 0, 1, 1) == 2                                 # more than 2^31 - 1 floats a frame
    assert check(65535 * 32 + 1, 1, 1, 3, 1, 1, 0, 0, 1, 1) == 2 and check(65535 * 32, 1, 1, 3, 1, 1, 0, 0, 1, 1) == 0
    null, one, two, three, four = (C.c_void_p(v) for v in (0, 16, 32, 48, 64))            # never dereferenced
    geometry = (7, 5, 3, 5, 13, 5, 0, 3, 5)
    guide = lib.vrg_flf_guide_f32
    for args in ((null, two, three, four), (one, null, three, four), (one, two, null, four), (one, two, three, null),
                 (one, two, three, one), (one, two, three, two), (C.c_void_p(18), two, three, four)):
        assert guide(*args, 9, *geometry, null) == 1, args
    assert guide(one, two, three, four, 0, *geometry, null) == 0
    assert guide(null, null, null, null, 0, *geometry, null) == 0
    assert guide(one, two, three, four, 9, 7, 5, 2, 5, 13, 5, 0, 3, 5, null) == 1

"""The enhancer upscale without a GPU: csrc/vrg_lanczos_math.hpp compiled for the host (tests/host_math/lanczos_check.cpp) against the
independent numpy restatement and the float64 yardstick of tests/lanczos_support.py; cv2 itself where a fixture or the package is at
hand; the enhancer's size helpers against the reference's recorded answers (tests/golden/enhancer_dimensions.json); the C ABI of the
new entry points and their refusals.  No test here reads the reference checkout."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import lanczos_support as LS
from conftest import GOLDEN, ROOT

# (source h, w) -> (out h, w), kind of input: the geometries the limits of the yardstick were established on
YARDSTICK_CASES = (((54, 96), (108, 192), "random"), ((54, 96), (96, 170), "random"), ((72, 128), (216, 384), "random"),
                   ((54, 96), (108, 192), "smooth"), ((60, 80), (90, 120), "random"))
EXACT_CASES = YARDSTICK_CASES + (((1, 1), (1, 1), "random"), ((1, 1), (5, 7), "random"), ((40, 60), (20, 30), "random"), ((5, 3), (11, 2), "random"),
                                 ((37, 53), (89, 131), "random"), ((48, 85), (77, 137), "random"), ((9, 200), (27, 100), "smooth"))


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return LS.build_host_lib(tmp_path_factory.mktemp("lanczos_check"))


def frames_of(src, kind, seed, n=2):
    make = LS.random_frames if kind == "random" else LS.smooth_frames
    return make((n, src[0], src[1], 3), seed)


@pytest.mark.parametrize("src,dst,kind", EXACT_CASES)
def test_host_header_equals_the_restatement(hm, src, dst, kind):
    x = frames_of(src, kind, 100 + src[0] + dst[1])
    keep = x.copy()
    want = LS.restated(x, dst[1], dst[0])
    got = LS.host_resize(hm, x, dst[1], dst[0])
    worst, share = LS.differences(got, want)
    print(f"{src} -> {dst} {kind}: largest difference {worst} levels, {share:.4%} of the bytes differ")
    assert np.array_equal(got, np.asarray(want)) and np.array_equal(x, keep)


def test_table_of_the_library_equals_the_header_and_the_restatement(hm, pkg):
    from comfyui_vrgamedevgirl_amd import ops
    for (h, w), (oh, ow) in (((54, 96), (108, 192)), ((1080, 1920), (2160, 3840)), ((480, 854), (768, 1366)), ((7, 5), (3, 11))):
        table = ops.lanczos4_taps(h, w, oh, ow)
        assert table.shape == (ow + oh,) and table.dtype.itemsize == ops.LANCZOS_TAP_BYTES == 20
        raw = np.zeros((ow + oh) * 20, dtype=np.uint8)
        hm.hm_lanczos4_taps(h, w, oh, ow, raw.ctypes.data)
        assert np.array_equal(raw, table.view(np.uint8))
        sx, wx = LS.axis_table(w, ow)
        sy, wy = LS.axis_table(h, oh)
        assert np.array_equal(table["s"], np.concatenate([sx, sy])) and np.array_equal(table["w"], np.concatenate([wx, wy]))
        assert np.abs(table["w"].astype(np.int64).sum(axis=1) - 2048).max() <= 3          # the sum is not fixed up: near 2048, not always equal


@pytest.mark.parametrize("src,dst,kind", YARDSTICK_CASES)
def test_float64_yardstick(hm, src, dst, kind):
    """the byte output is at most 1 level from the float64 Lanczos filter, on at most 15 % of the values"""
    x = frames_of(src, kind, 7)
    got = LS.host_resize(hm, x, dst[1], dst[0])
    worst, share = LS.differences(got, LS.yardstick64(x, dst[1], dst[0]))
    print(f"{src} -> {dst} {kind}: largest difference {worst} levels, {share:.4%} of the bytes differ")
    assert worst <= LS.YARDSTICK_MAX_LEVELS and share <= LS.YARDSTICK_MAX_SHARE


def test_lanczos_equals_cv2(hm):
    """the pin: cv2's own bytes, from the fixture if it was made, else from an importable cv2; neither is at hand everywhere"""
    if os.path.exists(LS.cv2_fixture_path()):
        data = np.load(LS.cv2_fixture_path())
        keys = json.loads(str(data["provenance"]))["cases"]
        cases = [(data[k + ".in"], data[k + ".out"]) for k in keys]
    else:
        cv2 = pytest.importorskip("cv2", reason="neither tests/golden/lanczos4_cv2.npz nor the cv2 package (opencv-python) is available")
        cases = []
        for (h, w), (oh, ow), kind in EXACT_CASES:
            if (h, w) == (oh, ow):
                continue
            x = frames_of((h, w), kind, 31)
            cases.append((x, np.stack([cv2.resize(f, (ow, oh), interpolation=cv2.INTER_LANCZOS4) for f in x])))
    for x, want in cases:
        got = LS.host_resize(hm, x, want.shape[2], want.shape[1])
        worst, share = LS.differences(got, want)
        print(f"{x.shape} -> {want.shape}: largest difference {worst} levels, {share:.4%} of the bytes differ")
        assert np.array_equal(got, want)
        assert np.array_equal(LS.restated(x, want.shape[2], want.shape[1]), want)


def test_equal_sizes_hand_back_the_same_objects(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneVideoEnhancerNodes as E
    frames = [LS.random_frames((6, 8, 3), i) for i in range(3)]
    back = E._resize_frames(frames, 8, 6)                                  # no GPU is touched: nothing to resize
    assert isinstance(back, list) and len(back) == 3 and all(a is b for a, b in zip(back, frames))
    x = LS.random_frames((1, 6, 8, 3), 9)
    assert LS.restated(x, 8, 6) is x


def test_size_helpers_give_the_reference_s_answers(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneVideoEnhancerNodes as E
    with open(os.path.join(GOLDEN, "enhancer_dimensions.json")) as fh:
        table = json.load(fh)
    assert len(table["output_dimensions"]) >= 200 and len(table["auto_batch_size"]) >= 30
    for row in table["output_dimensions"]:
        got = E._output_dimensions(row["width"], row["height"], row["upscale_resolution"])
        assert isinstance(got, tuple) and list(got) == row["result"], row
    for row in table["auto_batch_size"]:
        assert E._auto_batch_size(row["width"], row["height"]) == row["result"], row
    assert E._output_dimensions(1920, 1080, "4k") == (3840, 2160) and E._output_dimensions(854, 480, "2k") == (2560, 1438)


def _prototype(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vrgdg_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_library_exports_the_symbols_and_the_abi_is_8(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    lib = _hip.load_library()
    assert lib.vrg_abi_version() == 8 == _hip.ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read(), flags=re.S)
    assert "#define VRG_ABI_VERSION 8" in header
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    for name in ("vrg_lanczos4_u8", "vrg_upscale_sharpen_grain_u8", "vrg_lanczos4_taps"):
        assert name in _hip.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        proto = _prototype(header, name)
        res, args = _hip._SIGNATURES[name]
        assert res is C.c_int and len(proto) == len(args), name
        for text, ctype in zip(proto, args):
            want = C.c_void_p if "*" in text else kinds[text.split()[0]]
            assert ctype is want or (ctype is C.POINTER(_hip.NoiseDesc) and "vrg_noise_desc" in text), (name, text)
    assert set(pkg.NODE_CLASS_MAPPINGS) == set(pkg.NODE_DISPLAY_NAME_MAPPINGS)
    assert not [k for k in pkg.NODE_CLASS_MAPPINGS if "lanczos" in k.lower() or "upscale" in k.lower()]


def test_refusals_without_device(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    lib = _hip.load_library()
    null, a, b, t = C.c_void_p(0), C.c_void_p(64), C.c_void_p(1 << 20), C.c_void_p(1 << 21)      # far apart: operands that overlap are argument errors
    nd = _hip.NoiseDesc(seed0=1, seed_stride=1, offset0=0, offset_stride=0, chunk0=0, chunk_frames=1, grid_threads=256)

    def plain(i=a, o=b, frames=1, ih=4, iw=4, oh=8, ow=8, taps=t):
        return lib.vrg_lanczos4_u8(i, o, frames, ih, iw, oh, ow, taps, null)

    def fused(i=a, o=b, frames=1, ih=4, iw=4, oh=8, ow=8, taps=t, border=0, intensity=0.04, noise=nd):
        return lib.vrg_upscale_sharpen_grain_u8(i, o, frames, ih, iw, oh, ow, taps, 0.5, border, intensity, 0.5, 0.5,
                                                C.byref(noise) if noise is not None else None, null)

    for call in (plain, fused):
        assert call(frames=0) == _hip.VRG_OK                                        # zero frames: no launch
        assert call(i=null) == call(o=null) == call(taps=null) == _hip.VRG_ERR_BAD_ARG
        assert call(o=a) == _hip.VRG_ERR_BAD_ARG                                    # in == out
        assert call(frames=-1) == _hip.VRG_ERR_BAD_ARG
        for key in ("ih", "iw", "oh", "ow"):
            assert call(**{key: 0}) == _hip.VRG_ERR_BAD_ARG and call(**{key: -3}) == _hip.VRG_ERR_BAD_ARG
        assert call(i=null, frames=0) == _hip.VRG_ERR_BAD_ARG
    assert fused(border=2) == fused(border=-1) == _hip.VRG_ERR_BAD_ARG
    assert fused(noise=None) == _hip.VRG_ERR_BAD_ARG and fused(noise=None, intensity=0.0, frames=0) == _hip.VRG_OK
    assert fused(frames=1, ih=64, iw=8, oh=16, ow=8) == _hip.VRG_ERR_UNSUPPORTED    # a 4x downscale: the caller runs the two launches
    assert lib.vrg_lanczos4_taps(4, 4, 8, 8, null) == _hip.VRG_ERR_BAD_ARG and lib.vrg_lanczos4_taps(0, 4, 8, 8, a) == _hip.VRG_ERR_BAD_ARG


def test_python_surface(pkg):
    import torch
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneVideoEnhancerNodes as E
    from comfyui_vrgamedevgirl_amd import ops
    assert list(inspect.signature(ops.resize_frames_u8).parameters) == ["frames_u8", "out_w", "out_h"]
    assert list(inspect.signature(ops.upscale_sharpen_then_seeded_grain).parameters) == [
        "frames_u8", "out_w", "out_h", "strength", "use_gpu", "intensity", "saturation_mix", "seed", "frame_start"]
    assert list(inspect.signature(E._resize_frames).parameters) == ["frames", "output_width", "output_height"]
    assert list(inspect.signature(E._enhance_decoded).parameters) == ["frames", "output_width", "output_height", "settings", "frame_start"]
    assert inspect.signature(E._enhance_decoded).parameters["frame_start"].default == 0
    with pytest.raises(ValueError):
        ops.resize_frames_u8(torch.zeros(1, 4, 4, 3), 8, 8)                # fp32 frames are refused before any device work
    with pytest.raises(ValueError):
        ops.upscale_sharpen_then_seeded_grain(torch.zeros(4, 4, 3, dtype=torch.uint8), 8, 8, 0.5, True, 0.04, 0.5, 42, 0)
    with pytest.raises(ValueError):
        ops.lanczos4_taps(0, 4, 8, 8)

"""The enhancer upscale on the MI355X: vrg_lanczos4_u8 against the numpy restatement of tests/lanczos_support.py (itself equal to the
host-compiled header, tests/test_lanczos_host.py), the fused vrg_upscale_sharpen_grain_u8 against the two launches it replaces, and
_enhance_decoded on host lists and DecodedFrames.  Everything is compared byte for byte."""
import ctypes as C

import numpy as np
import pytest
import torch

import lanczos_support as LS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def E(pkg):
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneVideoEnhancerNodes
    return VRGDG_StandaloneVideoEnhancerNodes


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return LS.build_host_lib(tmp_path_factory.mktemp("lanczos_check"))


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def report(name, got, want):
    worst, share = LS.differences(got, want)
    print(f"{name}: largest difference {worst} levels, {share:.4%} of the bytes differ")
    return worst == 0 and got.shape == want.shape


# frames, (h, w) -> (oh, ow)
RESIZE_CASES = ((1, (1, 1), (1, 1)), (1, (1, 1), (5, 7)), (2, (480, 854), (768, 1366)), (2, (60, 80), (90, 120)), (3, (54, 96), (108, 192)),
                (1, (72, 128), (216, 384)), (2, (64, 96), (32, 48)), (5, (37, 53), (89, 131)), (2, (3, 200), (41, 7)), (1, (130, 70), (131, 260)),
                (1, (2, 8), (3, 16)))          # 8 wide: the one column position (s == 3) whose 24-byte window is the whole row; the others gather


@pytest.mark.parametrize("frames,src,dst", RESIZE_CASES)
def test_lanczos4_equals_the_restatement(ops, frames, src, dst):
    if src[1] == 8:
        assert LS.has_both_column_kinds(ops.lanczos4_taps(src[0], src[1], dst[0], dst[1])["s"][:dst[1]], src[1])
    x = LS.random_frames((frames, src[0], src[1], 3), 3 + src[1])
    xd = torch.from_numpy(x).to(dev())
    got = ops.resize_frames_u8(xd, dst[1], dst[0])
    if src == dst:
        assert got is xd
    assert got.dtype == torch.uint8 and tuple(got.shape) == (frames, dst[0], dst[1], 3)
    assert report(f"{src} -> {dst}", got.cpu().numpy(), np.asarray(LS.restated(x, dst[1], dst[0])))
    assert np.array_equal(xd.cpu().numpy(), x)


def test_lanczos4_1080p_to_4k_equals_the_host_header(ops, hm):
    x = LS.random_frames((1, 1080, 1920, 3), 2160)
    xd = torch.from_numpy(x).to(dev())
    got = ops.resize_frames_u8(xd, 3840, 2160).cpu().numpy()
    assert report("1080p -> 4K", got, LS.host_resize(hm, x, 3840, 2160))
    assert np.array_equal(xd.cpu().numpy(), x)


def test_lanczos4_offset_base_pointers(ops, pkg):
    """input and output that start 1 and 3 bytes off the dword grid, table as uploaded: same bytes"""
    from comfyui_vrgamedevgirl_amd import _hip
    x = LS.random_frames((2, 45, 67, 3), 17)
    want = np.asarray(LS.restated(x, 101, 91))
    src = torch.zeros(x.size + 8, dtype=torch.uint8, device=dev())
    src[1:1 + x.size] = torch.from_numpy(x.reshape(-1)).to(dev())
    dst = torch.full((want.size + 8,), 0xAB, dtype=torch.uint8, device=dev())
    taps = torch.from_numpy(ops.lanczos4_taps(45, 67, 91, 101).view(np.uint8).copy()).to(dev())
    st = _hip.lib().vrg_lanczos4_u8(C.c_void_p(src.data_ptr() + 1), C.c_void_p(dst.data_ptr() + 3), 2, 45, 67, 91, 101, _hip.ptr(taps), _hip.current_stream())
    assert st == _hip.VRG_OK
    out = dst.cpu().numpy()
    assert report("offset pointers", out[3:3 + want.size].reshape(want.shape), want)
    assert (out[:3] == 0xAB).all() and (out[3 + want.size:] == 0xAB).all()
    assert np.array_equal(src.cpu().numpy()[1:1 + x.size], x.reshape(-1))


SETTINGS = [(strength, zero, intensity) for zero in (False, True) for strength, intensity in ((0.6, 0.04), (0.6, 0.0), (0.0, 0.05), (0.0, 0.0))]


@pytest.mark.parametrize("strength,zero,intensity", SETTINGS)
@pytest.mark.parametrize("src,dst", (((54, 96), (108, 192)), ((48, 85), (77, 137)), ((1, 1), (5, 7)), ((270, 480), (540, 960)),
                                     ((2, 8), (3, 16))))
def test_fused_equals_the_two_launches(ops, src, dst, strength, zero, intensity):
    if src[1] == 8:
        assert LS.has_both_column_kinds(ops.lanczos4_taps(src[0], src[1], dst[0], dst[1])["s"][:dst[1]], src[1])
    x = LS.random_frames((3, src[0], src[1], 3), 23)
    xd = torch.from_numpy(x).to(dev())
    args = (strength, zero, intensity, 0.35, 42, 5)                       # frame_start = 5
    want = ops.sharpen_then_seeded_grain(ops.resize_frames_u8(xd, dst[1], dst[0]), *args)
    got = ops.upscale_sharpen_then_seeded_grain(xd, dst[1], dst[0], *args)
    assert report(f"{src} -> {dst} strength {strength} zero {zero} intensity {intensity}", got.cpu().numpy(), want.cpu().numpy())
    assert np.array_equal(xd.cpu().numpy(), x)
    # a batch split in two equals the batch whole
    a = ops.upscale_sharpen_then_seeded_grain(xd[:1], dst[1], dst[0], strength, zero, intensity, 0.35, 42, 5)
    b = ops.upscale_sharpen_then_seeded_grain(xd[1:], dst[1], dst[0], strength, zero, intensity, 0.35, 42, 6)
    assert torch.equal(torch.cat((a, b)), got)


def test_fused_falls_back_where_the_kernel_refuses(ops):
    x = torch.from_numpy(LS.random_frames((2, 96, 64, 3), 4)).to(dev())
    want = ops.sharpen_then_seeded_grain(ops.resize_frames_u8(x, 48, 24), 0.5, True, 0.04, 0.5, 7, 0)
    assert torch.equal(ops.upscale_sharpen_then_seeded_grain(x, 48, 24, 0.5, True, 0.04, 0.5, 7, 0), want)
    same = ops.upscale_sharpen_then_seeded_grain(x, 64, 96, 0.5, True, 0.04, 0.5, 7, 0)                  # equal sizes: the effects alone
    assert torch.equal(same, ops.sharpen_then_seeded_grain(x, 0.5, True, 0.04, 0.5, 7, 0))
    with pytest.raises(ValueError):
        ops.resize_frames_u8(x, 0, 4)
    assert tuple(ops.resize_frames_u8(x[:0], 10, 12).shape) == (0, 12, 10, 3)


@pytest.mark.parametrize("fused_with_grain", (False, True))
def test_enhance_decoded_on_lists_and_decoded_frames(ops, E, monkeypatch, fused_with_grain):
    monkeypatch.setattr(E, "FUSED_UPSCALE_WITH_GRAIN", fused_with_grain)
    x = LS.random_frames((4, 90, 160, 3), 77)
    frames = [x[i].copy() for i in range(4)]
    w, h = E._output_dimensions(160, 90, "2k")
    assert (w, h) == (2560, 1440)
    w, h = 320, 180
    for settings in ({"sharpen_enabled": True, "sharpen_strength": 0.5, "grain_enabled": True, "grain_intensity": 0.04, "seed": 9, "use_gpu": True},
                     {"sharpen_enabled": True, "grain_enabled": False, "use_gpu": False}, {"sharpen_enabled": False, "grain_enabled": False}):
        from_list = E._enhance_decoded(frames, w, h, settings, frame_start=3)
        decoded = E._frames_to_tensor(frames)
        from_decoded = E._enhance_decoded(decoded, w, h, settings, frame_start=3)
        assert isinstance(from_list, E.DecodedFrames) and isinstance(from_decoded, E.DecodedFrames)
        assert tuple(from_list.shape) == (4, h, w, 3) and from_list.smallest_batch == 4
        assert torch.equal(from_list.u8, from_decoded.u8)
        # = the reference's loop lines with this pack's helpers: resize, then the effects on the resized frames
        want = E._apply_effects_batch(E._resize_frames(decoded, w, h), settings, 3)
        assert torch.equal(from_list.u8, want.u8)
        assert all(np.array_equal(a, b) for a, b in zip(frames, x)) and np.array_equal(decoded.u8.cpu().numpy(), x)
        out = E._tensor_to_frames(from_list)
        assert len(out) == 4 and out[0].shape == (h, w, 3) and out[0].dtype == np.uint8
    resized = E._resize_frames(frames, w, h)
    assert isinstance(resized, list) and np.array_equal(np.stack(resized), np.asarray(LS.restated(x, w, h)))
    assert E._resize_frames(decoded, 160, 90) is decoded and ops.resize_frames_u8(decoded.u8, 160, 90) is decoded.u8

"""The skeleton that the four shared-Philox grain kernels of csrc/vrg_pointwise.hip share (csrc/vrg_grain_block.hpp) without a GPU:
grain_block and xcd_block compiled for the host (tests/host_math/grain_block_check.cpp) against the restatement below, and the shapes
of the two fused parametrisations of tests/test_gpu_parity.py classified with that restatement: each of the three fused kernels must
meet every seam of the block geometry there (a model of the geometry, no kernel is called)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_gpu_parity as P
from conftest import PKG_DIR, ROOT, load_package

GRAIN_N = 1024
#: the MI355X as torch reports it (multi_processor_count, max_threads_per_multi_processor): an input of the formula at the top of rng.py
#: (G = min(CUs * (max threads per CU / 256), ceil(numel / 256)) * 256), not a measurement
MI355X_CUS, MI355X_THREADS_PER_CU = 256, 2048
NOISE = (0x1234_5678_9ABC_DEF0, 0xFFFF_FFFF_0000_0001, 0xFFFF_FFFF_FFFF_FFF0, 12, 5)      # seed0, seed_stride, off0, off_stride, chunk0
M64 = (1 << 64) - 1


def grain_block(b, G, groups, noise=NOISE):
    """(unit, k, idx_base, valid_n, seed, off, ctr) of linear block b: units of `groups` calls of ceil(G / 1024) segments each"""
    seed0, seed_stride, off0, off_stride, chunk0 = noise
    segs = -(-G // GRAIN_N)
    unit, rem = divmod(b, segs * groups)
    k, seg = divmod(rem, segs)
    idx_base = seg * GRAIN_N
    off = (off0 + (chunk0 + unit) * off_stride) & M64
    return (unit, k, idx_base, min(GRAIN_N, G - idx_base), (seed0 + (chunk0 + unit) * seed_stride) & M64, off, ((off >> 2) + k) & M64)


def xcd_block(block, total):
    """linear index of workgroup `block` of the grid 8 * ceil(total / 8), None for a padding block: XCD block % 8 takes one contiguous run"""
    per_xcd = (total + 7) // 8
    b = (block % 8) * per_xcd + block // 8
    return b if block // 8 < per_xcd and b < total else None


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("grain_block_check")), "libgrain_block_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(PKG_DIR, "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host_math", "grain_block_check.cpp"), "-o", out], check=True)
    lib = C.CDLL(out)
    lib.hm_grain_n.restype = C.c_int32
    lib.hm_grain_blocks.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, np.ctypeslib.ndpointer(np.uint64, flags="C"),
                                    np.ctypeslib.ndpointer(np.uint64, flags="C")]
    lib.hm_xcd_blocks.argtypes = [C.c_uint32, C.c_uint32, np.ctypeslib.ndpointer(np.int64, flags="C")]
    return lib


@pytest.mark.parametrize("G", [256, 768, 1024, 1280, 3584, 524288])
def test_grain_block_decodes_every_block_once(hm, G):
    assert hm.hm_grain_n() == GRAIN_N
    segs = -(-G // GRAIN_N)
    for groups in (1, 2, 3):
        for units in (1, 2, 3):
            n = units * groups * segs
            got = np.zeros((n, 7), np.uint64)
            hm.hm_grain_blocks(n, G, groups, np.array(NOISE, np.uint64), got)
            assert [tuple(int(x) for x in row) for row in got] == [grain_block(b, G, groups) for b in range(n)], (G, groups, units)
            cells = sorted((int(u), int(k), int(i)) for u, k, i in got[:, :3])
            assert cells == [(u, k, s * GRAIN_N) for u in range(units) for k in range(groups) for s in range(segs)]      # each exactly once
            assert all(int(v) == min(GRAIN_N, G - int(i)) for i, v in got[:, 2:4])
            assert all(int(v) % 256 == 0 and int(v) > 0 for v in got[:, 3])                                               # whole waves


@pytest.mark.parametrize("total", [1, 7, 8, 9, 15, 16, 17, 1000])
def test_xcd_block_hands_out_every_block_once(hm, total):
    grid = 8 * ((total + 7) // 8)
    got = np.zeros(grid, np.int64)
    hm.hm_xcd_blocks(grid, total, got)
    assert [None if b < 0 else int(b) for b in got] == [xcd_block(block, total) for block in range(grid)]
    assert sorted(int(b) for b in got if b >= 0) == list(range(total))               # every b < total exactly once, all other blocks rejected
    assert int((got < 0).sum()) == grid - total
    for x in range(8):                                                               # one contiguous run per XCD
        run = [int(b) for b in got[x::8] if b >= 0]
        assert run == list(range(run[0], run[0] + len(run))) if run else True


# ---------------------------------------------------------------------------------------- the seams the fused tests reach
def _shapes(test):
    return next(m.args[1] for m in test.pytestmark if m.name == "parametrize" and m.args[0] == "shape")


def _kernel(shape, u8):
    """the kernel vrg_sharpen_grain_f32 / vrg_sharpen_grain_u8 launches for frames on aligned bases (None: the entry point refuses)"""
    F, H, W, _ = shape
    grid_kernel = W % 4 == 0 and W * 3 // 4 >= 256
    if not u8:
        return "k_sharpen_grain" if grid_kernel else None
    if F * H * W * 3 < 4:
        return None
    return "k_sharpen_grain_u8" if grid_kernel else "k_sharpen_grain_u8_any"


def _classes(shape):
    """the seams of the block geometry that one frame of `shape` meets: element = byte index, four per thread, 256 per wave and run"""
    rng = __import__("comfyui_vrgamedevgirl_amd.rng", fromlist=["rng"])
    F, H, W, _ = shape
    fe, E = H * W * 3, W * 3
    G = rng.grid_threads(fe, rng.DeviceGeometry(MI355X_CUS, MI355X_THREADS_PER_CU))
    groups = -(-fe // (4 * G))
    found = set()
    if fe % 4:
        found.add("frame bytes % 4 != 0")
    for b in range(groups * -(-G // GRAIN_N)):
        unit, k, idx_base, valid_n = grain_block(b, G, groups)[:4]
        assert unit == 0
        if valid_n < GRAIN_N:
            found.add("short last segment")
        if k >= 1:
            found.add("call k >= 1")
        for ii in range(4):
            first = 4 * G * k + idx_base + G * ii                                  # the run's first element in the frame
            if first >= fe:
                found.add("run starts past the frame")
                continue
            for wave in range(valid_n // 256):
                a0 = first + 256 * wave
                a1 = min(a0 + 255, fe - 1)
                if a0 < fe and a0 // E != a1 // E:
                    found.add("row end inside a wave")
    return found


SEAMS = ["short last segment", "call k >= 1", "run starts past the frame", "row end inside a wave"]


def test_the_fused_parametrisations_reach_every_seam_of_every_kernel():
    load_package()
    reached = {"k_sharpen_grain": set(), "k_sharpen_grain_u8": set(), "k_sharpen_grain_u8_any": set()}
    for test, u8 in ((P.test_fused_sharpen_then_seeded_grain_equals_the_two_kernels, False),
                     (P.test_u8_sharpen_then_seeded_grain_equals_the_converter_route, True)):
        for shape in _shapes(test):
            kernel = _kernel(shape, u8)
            assert kernel is not None, shape                                       # both tests assert VRG_OK of the entry point
            reached[kernel] |= _classes(shape)
    print(reached)
    for kernel, found in reached.items():
        want = SEAMS + (["frame bytes % 4 != 0"] if kernel == "k_sharpen_grain_u8_any" else [])
        assert not [s for s in want if s not in found], (kernel, [s for s in want if s not in found])
    assert "frame bytes % 4 != 0" not in reached["k_sharpen_grain"] | reached["k_sharpen_grain_u8"]      # those sit on the frame's dword grid

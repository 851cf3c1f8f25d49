"""The overlap rule without a GPU: vrg_ranges_overlap as a stand-alone program under the sanitizers, the C entry points refusing made-up
overlapping addresses before they touch a device, ops._disjoint on CPU tensors carved from one buffer, and the table of
tests/overlap_support.py held complete against the public functions of ops."""
import ast
import ctypes as C
import inspect
import os
import subprocess
import textwrap

import pytest
import torch

import overlap_support as S
from conftest import PKG_DIR, ROOT

HOST_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse"]
HOST_SOURCE = os.path.join(ROOT, "tests", "host_math", "overlap_check.cpp")


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def hip(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return _hip


def test_helper_under_the_sanitizers(tmp_path):
    """vrg_ranges_overlap against the 128-bit interval test: arrangements (a) .. (h), zero and negative lengths, ranges that end at the top
    of the address space, both argument orders (tests/host_math/overlap_check.cpp)"""
    exe = str(tmp_path / "overlap_check")
    cmd = ["g++", *HOST_FLAGS, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(PKG_DIR, "csrc"),
           HOST_SOURCE, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr + built.stdout and ("cannot find" in built.stderr or "unrecognized" in built.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and ran.stdout.startswith("overlap_check:") and not ran.stderr, ran.stderr
    assert int(ran.stdout.split()[1]) > 100000


def test_no_private_copy_of_the_interval_test_is_left():
    for name in sorted(n for n in os.listdir(os.path.join(PKG_DIR, "csrc")) if n.endswith((".hip", ".hpp", ".inc"))):
        with open(os.path.join(PKG_DIR, "csrc", name), encoding="utf-8") as fh:
            text = fh.read()
        assert not any(old in text for old in ("prep_overlap", "asm_overlap", "th_overlap")), name


# ---------------------------------------------------------------------------------------------------------------------------------
# the C entry points, with made-up addresses: every operand on its own 4 GiB page unless an arrangement moves it
# ---------------------------------------------------------------------------------------------------------------------------------
def _entries(hip, ops):
    """name -> (operands {name: (bytes, element bytes)}, written operand names, call(addresses) -> return code)"""
    from comfyui_vrgamedevgirl_amd import VRGDG_LUTVideoTools as LVT
    lib, null, P = hip.load_library(), C.c_void_p(0), C.c_void_p
    table = {}
    far = [P(0x7000_0000_0000 + (k << 20)) for k in range(6)]                          # records, tables, statistics: never dereferenced
    terms = ops.adjust_terms(LVT._normalize_adjust_settings({"clarity": 45, "sharpen": 30}))
    F, H, W = 2, 24, 40
    for name, elem in (("vrg_adjust_f32", 12), ("vrg_adjust_u8", 3)):
        fn = getattr(lib, name)
        table[name] = ({"in": (F * H * W * elem, elem // 3), "out": (F * H * W * elem, elem // 3), "tmp": (F * H * W * 12, 4)}, ("out", "tmp"),
                       lambda a, fn=fn: fn(P(a["in"]), P(a["out"]), P(a["tmp"]), F, H, W, C.byref(terms), null))
    chain = hip.ChainDesc(stages=hip.STAGE_SHARPEN, variant=1, stencil_op=0, border=0)
    for name, elem in (("vrg_fused_chain_f32", 12), ("vrg_fused_chain_u8", 3)):
        fn = getattr(lib, name)
        table[name] = ({"in": (F * H * W * elem, elem // 3), "out": (F * H * W * elem, elem // 3)}, ("out",),
                       lambda a, fn=fn: fn(P(a["in"]), P(a["out"]), F, H, W, C.byref(chain), null))
    for channels in (3, 2):                                                               # the flat march / tile kernel and the generic kernel
        table[f"vrg_stencil3x3_f32[{channels}]"] = (
            {"in": (F * H * W * channels * 4, 4), "out": (F * H * W * channels * 4, 4)}, ("out",),
            lambda a, c=channels: lib.vrg_stencil3x3_f32(P(a["in"]), P(a["out"]), F, H, W, c, 0, 0, 0.5, null))
    nd = hip.NoiseDesc(seed0=1, seed_stride=1, offset0=0, offset_stride=0, chunk0=0, chunk_frames=1, grid_threads=256)
    for name, elem in (("vrg_sharpen_grain_f32", 4), ("vrg_sharpen_grain_u8", 1)):
        fn = getattr(lib, name)
        table[name] = ({"in": (2 * 8 * 512 * 3 * elem, elem), "out": (2 * 8 * 512 * 3 * elem, elem)}, ("out",),
                       lambda a, fn=fn: fn(P(a["in"]), P(a["out"]), 2, 8, 512, 0.5, 0, 0.04, 0.5, 0.5, C.byref(nd), null))
    for oh, ow in ((5, 7), (13, 16)):                                                     # shrinking and enlarging
        geometry = (9, 11, 3, 0, 0, 11, 9, oh, ow, 0, 0, ow, oh)
        table[f"vrg_resize_f32[{oh}x{ow}]"] = ({"in": (F * 9 * 11 * 3 * 4, 4), "out": (F * oh * ow * 3 * 4, 4)}, ("out",),
                                               lambda a, g=geometry: lib.vrg_resize_f32(P(a["in"]), P(a["out"]), F, *g, 0, null))
    geometry = (5, 7, 3, 0, 0, 7, 5, 9, 11, 0, 0, 11, 9)
    table["vrg_restore_f32"] = ({"work": (2 * 5 * 7 * 3 * 4, 4), "originals": (3 * 9 * 11 * 4 * 4, 4), "out": (3 * 9 * 11 * 4 * 4, 4)}, ("out",),
                                lambda a: lib.vrg_restore_f32(P(a["work"]), P(a["originals"]), P(a["out"]), 2, 3, *geometry, 4, 0, 0.6, 0.4, null))
    table["vrg_crop_resize_f32"] = ({"in": (2 * 20 * 24 * 3 * 4, 4), "out": (2 * 6 * 7 * 3 * 4, 4)}, ("out",),
                                    lambda a: lib.vrg_crop_resize_f32(P(a["in"]), 2 * 20 * 24 * 3, P(a["out"]), far[0], 2, 6, 7, null))
    table["vrg_lanczos4_u8"] = ({"in": (F * 9 * 11 * 3, 1), "out": (F * 18 * 22 * 3, 1)}, ("out",),
                                lambda a: lib.vrg_lanczos4_u8(P(a["in"]), P(a["out"]), F, 9, 11, 18, 22, far[0], null))
    table["vrg_upscale_sharpen_grain_u8"] = (
        {"in": (F * 9 * 11 * 3, 1), "out": (F * 18 * 22 * 3, 1)}, ("out",),
        lambda a: lib.vrg_upscale_sharpen_grain_u8(P(a["in"]), P(a["out"]), F, 9, 11, 18, 22, far[0], 0.5, 0, 0.04, 0.5, 0.5, C.byref(nd), null))
    comp = {"crops": (2 * 6 * 5 * 3 * 4, 4), "originals": (2 * 12 * 14 * 3 * 4, 4), "user_mask": (2 * 6 * 5 * 4, 4), "out": (3 * 12 * 14 * 3 * 4, 4),
            "mask_out": (3 * 12 * 14 * 4, 4)}
    geom = (3, 2, 2, 2, 6, 5, 3, 12, 14, 3, 6, 5, 1, 3)
    table["vrg_composite_apply_f32"] = (comp, ("out", "mask_out"), lambda a: lib.vrg_composite_apply_f32(
        P(a["crops"]), P(a["originals"]), P(a["user_mask"]), far[0], far[1], P(a["out"]), P(a["mask_out"]), *geom, null))
    warp = dict(comp, bytes=(1000, 1))
    table["vrg_composite_warp_apply_f32"] = (warp, ("out", "mask_out"), lambda a: lib.vrg_composite_warp_apply_f32(
        P(a["crops"]), P(a["originals"]), P(a["user_mask"]), far[0], far[1], far[2], P(a["bytes"]), 1000, far[3], P(a["out"]), P(a["mask_out"]),
        *geom, null))
    table["vrg_warp_affine_u8"] = ({"in": (F * 9 * 11 * 3, 1), "out": (F * 6 * 7 * 3, 1)}, ("out",),
                                   lambda a: lib.vrg_warp_affine_u8(P(a["in"]), F * 9 * 11 * 3, P(a["out"]), far[0], far[1], F, 6, 7, null))
    return table


def test_c_entry_points_refuse_every_overlap_before_touching_a_device(hip, ops):
    """every refused arrangement of every (written, other) operand pair of every entry point that knows its operands' sizes returns
    VRG_ERR_BAD_ARG, on a machine without a GPU.  The accepted arrangements would launch and are not called here."""
    failures, calls = [], 0
    for name, (operands, written, call) in _entries(hip, ops).items():
        home = {operand: 0x1000_0000_0000 + (k << 32) for k, operand in enumerate(operands)}
        names = list(operands)
        for w in written:
            for other in names:
                if other == w or (other in written and names.index(other) < names.index(w)):
                    continue
                (w_bytes, w_item), (r_bytes, _) = operands[w], operands[other]
                for arrangement in S.REFUSED:
                    offset = S.placement(arrangement, w_bytes, w_item, r_bytes)
                    if offset is None:
                        continue
                    assert S.overlap_truth(offset, w_bytes, r_bytes)
                    rc = call(dict(home, **{w: home[other] + offset}))
                    calls += 1
                    if rc != hip.VRG_ERR_BAD_ARG:
                        failures.append(f"{name}: {w} against {other}, ({arrangement}) {S.ARRANGEMENTS[arrangement][1]}: returned "
                                        f"{'VRG_OK/launched' if rc == hip.VRG_OK else rc}")
    print(f"{calls} overlapping calls")
    assert not failures, "\n".join(failures)
    assert calls > 100


# ---------------------------------------------------------------------------------------------------------------------------------
# ops._disjoint
# ---------------------------------------------------------------------------------------------------------------------------------
def _carved(w_shape, w_dtype, r_shape, r_dtype, offset):
    """a written and a read CPU tensor in one buffer, the written one `offset` bytes from the read one's start"""
    w_bytes, r_bytes = S.nbytes_of(w_shape, w_dtype), S.nbytes_of(r_shape, r_dtype)
    buffer = torch.zeros(2 * (w_bytes + r_bytes) + 64, dtype=torch.uint8)
    base = (-buffer.data_ptr()) % 16 + (w_bytes + 15) // 16 * 16
    return S.carve(buffer, base + offset, w_shape, w_dtype), S.carve(buffer, base, r_shape, r_dtype), buffer


@pytest.mark.parametrize("w_shape,w_dtype,r_shape,r_dtype", [
    ((2, 3, 4, 3), torch.float32, (2, 3, 4, 3), torch.float32), ((1, 2, 2, 3), torch.float32, (3, 5, 4, 3), torch.float32),
    ((4, 6, 5, 3), torch.float32, (1, 3, 3, 3), torch.float32), ((2, 4, 4, 3), torch.uint8, (2, 5, 5, 3), torch.float32),
    ((2, 3, 3, 3), torch.float32, (1, 5, 5, 3), torch.uint8), ((1, 1, 1, 1), torch.float32, (1, 1, 1, 1), torch.float32)],
    ids=["same", "write-smaller", "write-larger", "bytes-out", "bytes-in", "one-element"])
def test_disjoint_on_tensors_carved_from_one_buffer(ops, w_shape, w_dtype, r_shape, r_dtype):
    w_bytes, r_bytes = S.nbytes_of(w_shape, w_dtype), S.nbytes_of(r_shape, r_dtype)
    w_item = torch.empty((), dtype=w_dtype).element_size()
    seen = set()
    for arrangement, (refused, what) in S.ARRANGEMENTS.items():
        offset = S.placement(arrangement, w_bytes, w_item, r_bytes)
        if offset is None:
            continue
        seen.add(arrangement)
        w, r, _keep = _carved(w_shape, w_dtype, r_shape, r_dtype, offset)
        assert S.overlap_truth(offset, w_bytes, r_bytes) == refused
        for writes, reads in (([("out", w)], [("images", r)]), ([("mask_out", r), ("out", w)], []), ([("out", w)], [("first", None), ("images", r)])):
            if refused:
                with pytest.raises(ValueError, match=r"^some operator: (out|mask_out) must not alias (images|out)") as caught:
                    ops._disjoint("some operator", writes, reads)
                assert "some operator" in str(caught.value) and "out" in str(caught.value), what
            else:
                assert ops._disjoint("some operator", writes, reads) is None, what
    assert {"a", "c", "f"} <= seen and ("g" in seen or r_bytes % w_item)
    # (h) the operand of a zero-frame call overlaps nothing, wherever it points
    w, r, _keep = _carved(w_shape, w_dtype, r_shape, r_dtype, 0)
    for empty in (w[:0], w[1:1] if w.shape[0] > 1 else w[:0]):
        ops._disjoint("op", [("out", empty)], [("images", r)])
        ops._disjoint("op", [("out", w)], [("images", r[:0])])


def test_disjoint_compares_within_one_address_space_and_judges_the_copy(ops):
    x = torch.zeros((2, 3, 4, 3))
    ops._disjoint("op", [("out", None), ("mask_out", None)], [("images", x), ("user_mask", None)])
    ops._disjoint("op", [], [("images", x), ("again", x)])                             # two reads may share memory
    elsewhere = torch.empty((2, 3, 4, 3), device="meta")                                 # another device: another address space
    ops._disjoint("op", [("out", elsewhere)], [("images", x)])
    ops._disjoint("op", [("out", x)], [("images", elsewhere)])
    with pytest.raises(ValueError, match="^op: out must not alias workspace"):
        ops._disjoint("op", [("out", x), ("workspace", x[1:])], [])
    # a non-contiguous input reaches the kernel as the contiguous copy _check_frames makes: out may lie in the view's storage
    storage = torch.zeros((2, 3, 4, 6))
    view = storage[..., :3]
    copy = view if view.is_contiguous() else view.contiguous()
    out = storage.view(-1)[:72].view(2, 3, 4, 3)
    assert not view.is_contiguous() and out.data_ptr() == view.data_ptr()
    ops._disjoint("op", [("out", out)], [("images", copy)])
    with pytest.raises(ValueError, match="^op: out must not alias images"):
        ops._disjoint("op", [("out", out)], [("images", storage)])


def test_out_like_is_checked_out_plus_disjoint(ops):
    x = torch.zeros((4, 3, 4, 3))
    with pytest.raises(ValueError, match="^stencil3x3: out must not alias images"):
        ops._out_like(x[:-1], x[1:], "stencil3x3", "images")
    assert ops._out_like(x[:2], x[2:], "stencil3x3", "images").data_ptr() == x[2:].data_ptr()


# ---------------------------------------------------------------------------------------------------------------------------------
# completeness
# ---------------------------------------------------------------------------------------------------------------------------------
def _public_writers(ops):
    found = {}
    for name, fn in vars(ops).items():
        if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != ops.__name__:
            continue
        written = [p for p in inspect.signature(fn).parameters if p in S.WRITE_PARAMETERS]
        if written:
            found[name] = written
    return found


def _called(fn):
    """{name: [keyword and positional argument names]} of the calls in the source of `fn`"""
    tree = ast.parse(textwrap.dedent(inspect.getsource(fn)))
    calls = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name):
            passed = [a.id for a in node.args if isinstance(a, ast.Name)] + [k.value.id for k in node.keywords if isinstance(k.value, ast.Name)]
            calls.setdefault(node.func.id, []).extend(passed)
    return calls


def guarded(ops, name, rows, depth=0):
    """does the source of ops.<name> call _disjoint or _out_like, or hand every write operand to a function of the table (or to a
    private helper of ops that is itself guarded)?"""
    fn = inspect.unwrap(getattr(ops, name))
    calls = _called(fn)
    if "_disjoint" in calls or "_out_like" in calls:
        return True
    written = [p for p in inspect.signature(fn).parameters if p in S.WRITE_PARAMETERS]
    for callee, passed in calls.items():
        if not hasattr(ops, callee) or not inspect.isfunction(getattr(ops, callee)) or not all(w in passed for w in written):
            continue
        if callee in rows or (callee.startswith("_") and depth < 2 and guarded(ops, callee, rows, depth + 1)):
            return True
    return False


def test_every_operator_with_a_write_operand_has_a_row_and_a_guard(ops):
    writers = _public_writers(ops)
    rows = {row.op for row in S.ROWS}
    assert sorted(writers) == sorted(rows), (sorted(set(writers) - rows), sorted(rows - set(writers)))
    assert len(writers) >= 25
    for row in S.ROWS:
        assert set(row.writes) <= set(writers[row.op]), row.op                         # a row names write operands of its operator
        assert row.reads and len(set(S.row_id(r) for r in S.ROWS)) == len(S.ROWS)
    for name, written in writers.items():
        covered = set().union(*(row.writes for row in S.ROWS if row.op == name))
        assert covered == set(written), (name, written, covered)                        # ... and together they name all of them
        assert guarded(ops, name, rows), f"ops.{name} takes {written} and neither calls _disjoint / _out_like nor hands them to an operator that does"


def test_the_completeness_check_notices_a_missing_guard(ops, monkeypatch):
    """the check above fails for an operator without a guard and for a table without its row"""
    def unguarded(images, out=None):
        return _checked_out(out, images.shape, images.dtype, images.device, "unguarded")      # noqa: F821
    unguarded.__module__ = ops.__name__
    monkeypatch.setattr(ops, "unguarded", unguarded, raising=False)
    rows = {row.op for row in S.ROWS}
    assert "unguarded" in _public_writers(ops) and "unguarded" not in rows
    assert not guarded(ops, "unguarded", rows)
    assert guarded(ops, "resize_frames", rows) and not guarded(ops, "resize_frames", rows - {"resize_geometry_frames"})

"""The Face Fix crop sequence without a GPU: the arithmetic of csrc/vrg_resize_math.hpp on a box view, compiled for the host
(tests/host_math/crop_check.cpp), against the recorded results of the reference's VRGDGFaceFixPrepare.prepare and
VRGDGFaceFixPrepareShotAware.prepare (tests/golden/crop.json: SHA-256 digests of torch's plain CPU kernels' output,
ATEN_CPU_CAPABILITY=default; the input frames are rebuilt from the recorded seeds); ops.crop_sequence_plan against the recorded hole
filling and prefix; the C ABI of vrg_crop_resize_f32; the public surface.  No test here reads the reference checkout."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import crop_support as CS
from conftest import ROOT

META = CS.meta()
CASES = META["cases"]
KEYS = [c["key"] for c in CASES]


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return CS.build_host_lib(tmp_path_factory.mktemp("crop_check"))


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def golden():
    return CS.arrays()


def plan_of(ops, case):
    n, h, w, _ = case["shape"]
    return ops.crop_sequence_plan(CS.entries_of(case), n, h, w, per_shot=case["per_shot"])


def test_fixture_was_made_by_the_plain_torch_kernels_and_covers_the_ground():
    prov = META["provenance"]
    assert prov["ATEN_CPU_CAPABILITY"] == "default" and prov["cpu_capability"].upper() in ("DEFAULT", "NO AVX")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "crop.npz")) < (1 << 20)
    assert len(CASES) == 11 and META["samples"] == CS.SAMPLES
    boxes = [(e["box"][2] - e["box"][0], e["box"][3] - e["box"][1], c) for c in CASES for e in c["entries"] if e["box"]]
    widths = [b[0] for b in boxes]
    assert 9 in widths and 300 in widths and 1 in widths                                   # up from 9 .. 300, the 1 x 1 box
    assert any(512 < w <= 2048 for w in widths) and any(w > 2048 for w in widths)          # down, and past 4x down
    assert any(w == min(c["shape"][1], c["shape"][2]) for w, _, c in boxes)                # the whole short side
    edges = set()
    for c in CASES:
        for e in c["entries"]:
            if e["box"]:
                l, t, r, b = e["box"]
                edges |= {name for name, hit in (("left", l == 0), ("top", t == 0), ("right", r == c["shape"][2]), ("bottom", b == c["shape"][1])) if hit}
    assert edges == {"left", "top", "right", "bottom"}
    assert {c["shape"][3] for c in CASES} == {3, 4}
    has = lambda c: [e["box"] is not None for e in c["entries"]]                           # noqa: E731
    assert any(not has(c)[0] for c in CASES) and any(not has(c)[-1] for c in CASES)        # leading and trailing holes
    assert any(False in has(c)[has(c).index(True):len(has(c)) - has(c)[::-1].index(True)] for c in CASES)     # inner holes
    assert any(sum(has(c)) == 1 and len(has(c)) > 1 for c in CASES)                        # a single valid frame
    assert {0, 7} <= {c["ltx_frame_offset"] for c in CASES}
    shots = [c for c in CASES if c["per_shot"] and len({e["shot_id"] for e in c["entries"]}) > 1]
    assert any(any(all(e["box"] is None for e in c["entries"] if e["shot_id"] == s) for s in {e["shot_id"] for e in c["entries"]}) for c in shots)
    assert all(c["value_range"][0] == 0.0 and c["value_range"][1] == 1.0 for c in CASES if c["key"] != "one_by_one")       # the clamp acts
    assert [e["text"] for e in META["errors"] if e["shape"][0]] == ["No face was detected in the video. Lower confidence or minimum face pixels."] * 2


@pytest.mark.parametrize("key", KEYS)
def test_host_arithmetic_has_the_reference_s_digests(hm, ops, golden, key):
    """(a) the header's arithmetic on whole cases: 0 differing elements -- the batch digest, every frame's digest, the anchors' digest and
    the sampled values are the reference's"""
    case = CASES[KEYS.index(key)]
    x = CS.make_frames(case["shape"], case["seed"])
    plan = plan_of(ops, case)
    got = CS.host_crop(hm, x, CS.plan_records(plan, case["shape"][3]))
    assert list(got.shape) == case["crop_shape"]
    samples = golden[key + ".samples"]
    print(CS.describe_difference(case, got, samples))
    assert CS.mismatches(got.reshape(-1)[CS.sample_positions(got.size, case["seed"])], samples) == 0
    assert CS.frame_shas(got) == case["frame_sha256"]
    assert CS.sha(got) == case["crop_sha256"]
    anchors = got[plan.ltx_offset:][np.asarray(case["anchors"], dtype=np.int64)]
    assert list(anchors.shape) == case["anchor_shape"] and CS.sha(anchors) == case["anchor_sha256"]


@pytest.mark.parametrize("key", KEYS)
def test_plan_is_the_recorded_fill_and_prefix(ops, key):
    """(b) which output frame repeats which: two output frames of the plan name the same (frame, box) exactly where the reference's
    frames have the same digest; the prefix length and the frame count are the reference's; a frame with a box reads itself"""
    case = CASES[KEYS.index(key)]
    plan = plan_of(ops, case)
    assert plan.ltx_offset == case["ltx_frame_offset"] == (-(case["shape"][0] - 1)) % 8
    assert plan.count == case["crop_shape"][0] == plan.ltx_offset + case["shape"][0]
    shas = case["frame_sha256"]
    for j in range(plan.count):
        for k in range(j):
            assert (plan.sources[j] == plan.sources[k]) == (shas[j] == shas[k]), (key, j, k)
    assert all(s == plan.sources[plan.ltx_offset] for s in plan.sources[:plan.ltx_offset])
    for i, e in enumerate(case["entries"]):
        if e["box"]:
            assert plan.sources[plan.ltx_offset + i] == (i, tuple(e["box"]))


def test_plan_fill_rules_by_hand(ops):
    a, b, c = (1, 2, 5, 6), (0, 0, 8, 8), (2, 2, 4, 7)
    entries = [{"box": None, "shot_id": 0}, {"box": a, "shot_id": 0}, {"box": None, "shot_id": 1}, {"box": None, "shot_id": 2},
               {"box": b, "shot_id": 2}, {"box": c, "shot_id": 2}, {"box": None, "shot_id": 2}, {"box": None, "shot_id": 3}, {"box": [], "shot_id": 3}]
    plan = ops.crop_sequence_plan(entries, 9, 8, 8)
    assert plan.ltx_offset == 0 and plan.sources == ((1, a), (1, a), (1, a), (1, a), (4, b), (5, c), (5, c), (5, c), (5, c))
    shot = ops.crop_sequence_plan(entries, 9, 8, 8, per_shot=True)
    assert shot.sources == ((1, a), (1, a), (1, a), (4, b), (4, b), (5, c), (4, b), (1, a), (1, a))
    two = ops.crop_sequence_plan(entries[:2], 2, 8, 8)
    assert two.ltx_offset == 7 and two.sources == ((1, a),) * 9 and two.count == 9
    assert (two.frames, two.height, two.width) == (2, 8, 8)
    for n in range(1, 20):
        assert ops.crop_sequence_plan([{"box": a}] * n, n, 8, 8).ltx_offset == (-(n - 1)) % 8
        assert (ops.crop_sequence_plan([{"box": a}] * n, n, 8, 8).count - 1) % 8 == 0


def test_plan_refusals_and_their_messages(ops):
    for e in META["errors"]:
        if not e["shape"][0]:
            continue
        n, h, w, _ = e["shape"]
        with pytest.raises(ValueError) as exc:
            ops.crop_sequence_plan([{"box": None, "shot_id": 0}] * n, n, h, w, per_shot=e["per_shot"])
        assert str(exc.value) == e["text"]
    ok = {"box": (1, 1, 4, 4)}
    for box, words in (((1, 1, 4), "not four integers"), ((1, 1, 4, 4.5), "not four integers"), ("abcd", "not four integers"),
                       ((3, 1, 3, 4), "is empty"), ((1, 5, 4, 2), "is empty"), ((-1, 1, 4, 4), "does not lie inside the 8 x 6 frame"),
                       ((1, 1, 9, 4), "does not lie inside"), ((1, 1, 4, 7), "does not lie inside"), ((1, -2, 4, 4), "does not lie inside")):
        with pytest.raises(ValueError) as exc:
            ops.crop_sequence_plan([ok, {"box": box}], 2, 6, 8)
        assert words in str(exc.value) and "refused" in str(exc.value), (box, str(exc.value))
    with pytest.raises(ValueError) as exc:
        ops.crop_sequence_plan([ok, ok, ok], 2, 6, 8)
    assert "3 Face Fix entries for 2 video frames" in str(exc.value)
    assert ops.crop_sequence_plan([{"box": (np.int64(0), np.int32(0), 8, 6)}], 1, 6, 8).sources[0] == (0, (0, 0, 8, 6))     # numpy integers are integers


def test_surface_refuses_before_any_device_work(pkg):
    """face_crop_sequence: the reference's message for an empty batch, the plan's refusals -- all raised before a GPU is needed"""
    import torch
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes as FF
    empty = next(e for e in META["errors"] if not e["shape"][0])
    for frames in (torch.zeros(empty["shape"]), torch.zeros(4, 4, 3)):
        with pytest.raises(ValueError) as exc:
            FF.face_crop_sequence(frames, [])
        assert str(exc.value) == empty["text"]
    with pytest.raises(ValueError, match="No face was detected in the video"):
        FF.face_crop_sequence(torch.zeros(2, 8, 8, 3), [{"box": None}, {"box": None}])
    with pytest.raises(ValueError, match="does not lie inside"):
        FF.face_crop_sequence(torch.zeros(1, 8, 8, 3), [{"box": (0, 0, 9, 9)}])


def _prototype(name):
    header = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vrgdg_hip.h"
    return header, [" ".join(a.split()) for a in m.group(1).split(",")]


def test_prototype_struct_and_ctypes_agree(pkg):
    """(c) header <-> _hip for the new entry point, argument by argument; vrg_crop_desc <-> CropDesc field by field; the ABI is still 8"""
    from comfyui_vrgamedevgirl_amd import _hip, ops
    header, proto = _prototype("vrg_crop_resize_f32")
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    assert "vrg_crop_resize_f32" in _hip.EXPORTED_SYMBOLS
    res, args = _hip._SIGNATURES["vrg_crop_resize_f32"]
    assert res is C.c_int and len(proto) == len(args)
    for text, ctype in zip(proto, args):
        assert ctype is (C.c_void_p if "*" in text else kinds[text.split()[0]]), text
    assert [a.split()[-1].lstrip("*") for a in proto] == ["in", "in_floats", "out", "desc", "n_out", "size_h", "size_w", "stream"]
    body = re.search(r"typedef struct vrg_crop_desc \{(.*?)\} vrg_crop_desc;", header, flags=re.S).group(1)
    fields = []
    for kind, names in re.findall(r"(int64_t|int32_t)\s+([^;]+);", body):
        for name in names.split(","):
            name = name.strip()
            m = re.match(r"(\w+)\[(\d+)\]", name)
            fields.append((m.group(1), kinds[kind] * int(m.group(2))) if m else (name, kinds[kind]))
    assert [f[0] for f in fields] == [f[0] for f in _hip.CropDesc._fields_]
    for (name, want), (_, got) in zip(fields, _hip.CropDesc._fields_):
        assert C.sizeof(want) == C.sizeof(got) and (got is want or got._length_ == want._length_), name
    assert C.sizeof(_hip.CropDesc) == 32 == ops._CROP_DESC.itemsize and _hip.CropDesc.row_pitch.offset == 8 and _hip.CropDesc.box_w.offset == 16
    assert [ops._CROP_DESC.fields[n][1] for n, _ in _hip.CropDesc._fields_] == [getattr(_hip.CropDesc, n).offset for n, _ in _hip.CropDesc._fields_]
    assert _hip.ABI_VERSION == 8 and "#define VRG_ABI_VERSION 8" in header


def test_argument_validation_without_device(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    lib = _hip.load_library()
    assert lib.vrg_abi_version() == 8
    null, one, two, three = C.c_void_p(0), C.c_void_p(16), C.c_void_p(32), C.c_void_p(48)

    def crop(a=one, floats=1000, out=two, desc=three, n_out=1, size_h=512, size_w=512):
        return lib.vrg_crop_resize_f32(a, floats, out, desc, n_out, size_h, size_w, null)

    assert crop(n_out=0) == 0                                                      # zero frames: no launch
    assert crop(a=null) == 1 and crop(out=null) == 1 and crop(desc=null) == 1
    assert crop(a=null, n_out=0) == 1 and crop(n_out=-1) == 1 and crop(floats=-1) == 1
    assert crop(size_h=0) == 1 and crop(size_w=0) == 1 and crop(size_h=-512) == 1 and crop(out=one) == 1


def test_public_surface(pkg):
    """(d) face_crop_sequence as the issue states it; no Prepare node class; the module's and the package's mappings are untouched"""
    from comfyui_vrgamedevgirl_amd import VRGDG_StandaloneFaceFixNodes as FF
    from comfyui_vrgamedevgirl_amd import ops
    sig = inspect.signature(FF.face_crop_sequence)
    assert list(sig.parameters) == ["video_frames", "entries", "per_shot", "anchors"]
    assert sig.parameters["per_shot"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["per_shot"].default is False
    assert sig.parameters["anchors"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["anchors"].default is None
    assert list(inspect.signature(ops.crop_sequence_plan).parameters) == ["entries", "frames", "height", "width", "per_shot"]
    assert list(inspect.signature(ops.crop_frames).parameters) == ["frames", "plan", "size", "out"]
    assert list(inspect.signature(ops.crop_frames_host).parameters) == ["frames_cpu", "plan", "size"]
    assert inspect.signature(ops.crop_frames).parameters["size"].default == (512, 512)
    assert set(FF.NODE_CLASS_MAPPINGS) == {"VRGDGFaceFixComposite", "VRGDGFaceFixCompositeOpaque"} == set(FF.NODE_DISPLAY_NAME_MAPPINGS)
    assert not [n for n in dir(FF) if "Prepare" in n]
    assert not [k for k in pkg.NODE_CLASS_MAPPINGS if "FaceFix" in k or "crop" in k.lower()]

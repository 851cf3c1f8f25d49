"""The anchor round trip without a GPU: csrc/vrg_anchor_math.hpp compiled for the host against live Pillow and numpy; the five node classes
-- their Meta Batch protocol, folders, messages and contexts -- against the fixture recorded from the reference's classes
(tests/golden/anchor_roundtrip.*), with the two launches replaced by the host-compiled header; the surfaces, the mappings and the ABI."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import anchor_support as S
from conftest import PKG_NAME, ROOT

NEW_SYMBOLS = ("vrg_anchor_check", "vrg_anchor_frames_f32", "vrg_anchor_store_u8")
NODES = ("VRGDGVideoEnhanceLoadAnchorsMetaBatch", "VRGDGVideoEnhanceStoreAnchors", "VRGDGVideoEnhanceCollectLTXInputs",
         "VRGDGFaceFixLoadAnchorsMetaBatch", "VRGDGFaceFixStoreAnchors")


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext, ops
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return ops


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return S.build_host_lib(tmp_path_factory.mktemp("anchor_host"))


@pytest.fixture()
def nodes(ops, host, monkeypatch):
    with S.nodes_on_host(monkeypatch, PKG_NAME, ops, host) as found:
        yield found


# ---------------------------------------------------------------------------------------------------------------------------------
# the load rule
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", (S.FIRST,) + S.FIRSTS, ids=lambda s: "%dx%d" % s)
def test_load_rule_equals_pillow_and_numpy(ops, host, first):
    """every picture of the geometry list, bit for bit, for every first picture"""
    pictures = S.load_pictures(first, 1 + len(S.OTHERS), seed=3)
    got = S.host_frames(ops, host, pictures)
    assert S.same_bits(got, S.load_expected(pictures)) == 0


def test_the_copy_route_is_what_pillow_does_at_an_equal_size(ops, host):
    from PIL import Image
    a = S.picture(9, S.FIRST)
    assert np.array_equal(np.asarray(Image.fromarray(a).resize(S.FIRST, Image.Resampling.LANCZOS)), a)       # Pillow returns the bytes unchanged
    desc, tables, src_bytes, size = ops.anchor_plan([a.shape[:2], a.shape[:2]])
    assert not tables.size and not desc["h_ksize"].any() and not desc["v_ksize"].any() and size == (24, 40)
    got = S.host_frames(ops, host, [a, a])
    assert S.same_bits(got[1], a.astype(np.float32) / 255.0) == 0 and S.same_bits(got[0], got[1]) == 0
    every = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 256, 3)                                        # every byte / 255.0, IEEE
    assert S.same_bits(S.host_frames(ops, host, [every])[0], every.astype(np.float32) / 255.0) == 0


def test_a_given_size_and_the_vertical_chunks(ops, host):
    """size= for a later chunk of a sequence; 333 source rows onto 24 pass through LDS in several chunks of ANC_SLOTS rows"""
    slots = host.hm_anchor_constant(2)
    tall = S.picture(4, (7, 333))
    desc, tables, _, _ = ops.anchor_plan([tall.shape[:2]], S.FIRST)
    bounds = tables[int(desc["v_table"][0]):][:2 * 24].reshape(24, 2)
    assert bounds[15].sum() - bounds[0][0] > 2 * slots                                                         # the first tile's rows: three chunks
    pictures = [tall, S.picture(5, (97, 61))]
    assert S.same_bits(S.host_frames(ops, host, pictures, S.FIRST), S.load_expected(pictures, S.FIRST)) == 0


def test_the_launch_chunks_tile_the_records(ops, host):
    n = host.hm_anchor_constant(3) + 3
    assert n == S.LAUNCH_RECORDS + 3
    pictures = [np.full((1, 1, 3), i % 251, dtype=np.uint8) + np.arange(3, dtype=np.uint8) for i in range(n)]
    calls = np.zeros(1, dtype=np.int32)
    got = S.host_frames(ops, host, pictures, calls=calls)
    assert int(calls[0]) == 2 and S.same_bits(got, np.stack(pictures).astype(np.float32) / 255.0) == 0


def test_the_host_check_refuses_bad_records(ops, host):
    """the refusal code only: nothing is launched for a record the kernel would not follow"""
    shapes = [(24, 40), (61, 97), (9, 17)]
    desc, tables, src_bytes, (h, w) = ops.anchor_plan(shapes)
    lib = ops._host_lib()

    def rc(d, t=tables, nbytes=src_bytes, hh=h, ww=w, check=None):
        d, t = np.ascontiguousarray(d), np.ascontiguousarray(t)
        return (check or lib.vrg_anchor_check)(C.c_void_p(d.ctypes.data), len(d), C.c_void_p(t.ctypes.data), t.size, nbytes, hh, ww)

    for check in (lib.vrg_anchor_check, host.hm_anchor_check):
        assert rc(desc, check=check) == 0
        assert rc(desc, nbytes=src_bytes - 1, check=check) == 1                                                 # the last picture leaves the buffer
        assert rc(desc, t=tables[:-1], check=check) == 1                                                        # a table leaves the buffer
        assert rc(desc, hh=0, check=check) == 1
        for field, value in (("src_offset", -1), ("in_w", 0), ("in_h", -3), ("h_ksize", 0), ("v_table", -4), ("h_table", tables.size)):
            bad = desc.copy()
            bad[field][1] = value
            assert rc(bad, check=check) == 1, field
        worse = tables.copy()
        worse[int(desc["h_table"][1])] = 97                                                                    # the first tap of column 0 outside the row
        assert rc(desc, t=worse, check=check) == 1
        worse = tables.copy()
        worse[int(desc["v_table"][2]) + 1] = int(desc["v_ksize"][2]) + 1                                        # more taps than the table holds
        assert rc(desc, t=worse, check=check) == 1
    with pytest.raises(ValueError, match="vrg_anchor_check refuses"):
        ops.anchor_check(desc, tables, src_bytes - 1, h, w)
    # Image.resize takes a picture more than 100 times as tall as wide vertically first when its height shrinks: not built, refused
    for shape, code in (((301, 3), 2), ((300, 3), 0), ((301, 3000), 0)):
        tall = ops.anchor_plan([shape], S.FIRST)
        for check in (lib.vrg_anchor_check, host.hm_anchor_check):
            assert rc(tall[0], t=tall[1], nbytes=tall[2], check=check) == code, shape
    with pytest.raises(RuntimeError, match="100 times as tall"):
        ops.anchor_check(*ops.anchor_plan([(301, 3)], S.FIRST)[:3], 24, 40)
    edge = [S.picture(8, (3, 300))]
    assert S.same_bits(S.host_frames(ops, host, edge, S.FIRST), S.load_expected(edge, S.FIRST)) == 0          # exactly 100 times: Pillow's usual order
    with pytest.raises(ValueError, match="at least one picture"):
        ops.anchor_plan([])
    with pytest.raises(ValueError, match="uint8"):
        ops.anchor_frames([np.zeros((4, 4, 3), dtype=np.float32)])
    with pytest.raises(ValueError, match="uint8"):
        ops.anchor_frames([np.zeros((0, 4, 3), dtype=np.uint8)])


# ---------------------------------------------------------------------------------------------------------------------------------
# the store rule
# ---------------------------------------------------------------------------------------------------------------------------------
def test_store_rule_equals_numpy(host):
    """ties to even at every (k +- 0.5) / 255 and its neighbours, the clamp, -0.0, subnormals, the infinities, and NaN as live numpy gives it"""
    values = S.tie_table()
    want = S.store_expected(values.reshape(-1, 1, 1, 1).repeat(3, axis=3)).reshape(-1, 3)[:, 0]
    got = S.host_store(host, values.reshape(-1, 1, 1, 1).repeat(3, axis=3)).reshape(-1, 3)[:, 0]
    nan = np.isnan(values)
    print("numpy's uint8 of NaN on this host:", want[nan].tolist(), "-- the kernel's:", host.hm_anchor_constant(4))
    assert np.array_equal(got, want), [(float(v), int(g), int(w)) for v, g, w in zip(values, got, want) if g != w][:8]
    assert nan.sum() == 2 and (want[nan] == host.hm_anchor_constant(4)).all() and host.hm_anchor_constant(4) == 0
    assert np.float32(0.5 / 255) * np.float32(255) == np.float32(0.5) and want[256] == 0                        # a tie fp32 holds exactly: to even


@pytest.mark.parametrize("channels", S.STORE_CHANNELS)
@pytest.mark.parametrize("bgr", (False, True), ids=("rgb", "bgr"))
def test_store_batches_equal_numpy(host, channels, bgr):
    for hw in S.STORE_SHAPES:
        for n in S.STORE_FRAMES:
            x = S.store_batch(n, hw, channels, seed=n + hw[1])
            assert np.array_equal(S.host_store(host, x, bgr), S.store_expected(x, bgr)), (hw, n)
    x = S.seam_batch(channels)
    assert np.array_equal(S.host_store(host, x, bgr), S.store_expected(x, bgr))


# ---------------------------------------------------------------------------------------------------------------------------------
# the nodes against the fixture
# ---------------------------------------------------------------------------------------------------------------------------------
def _loader(module, which):
    return getattr(module, {"video_enhance": "VRGDGVideoEnhanceLoadAnchorsMetaBatch", "face_fix": "VRGDGFaceFixLoadAnchorsMetaBatch"}[which])()


@pytest.mark.parametrize("which", ("video_enhance", "face_fix"))
def test_load_nodes_follow_the_recorded_protocol(nodes, tmp_path, which):
    """frames_per_batch of 1, 3, the file count and more: every chunk, the state after every call, the clamped total, the exhausted
    generator's error; the file filter and the order (a_10.bmp before a_9.PNG, the .txt and .gif left out); one launch per call"""
    ve, ff, launches = nodes
    node = _loader({"video_enhance": ve, "face_fix": ff}[which], which)
    sources = S.write_sources(str(tmp_path / "anchor_sources"))
    context = {"anchor_sources_folder": sources, "job_id": "job_a"}
    order = [S.FIXTURE["pictures"][i]["name"] for i in S.FIXTURE["order"]]
    anchors = importlib.import_module(PKG_NAME + "._anchors")
    assert [os.path.basename(p) for p in anchors.anchor_files(sources)] == order == ["a_10.bmp", "a_9.PNG", "b_2.png", "c_0.png", "d_1.png"]
    assert S.same_bits(S.ARRAYS["frames"], S.load_expected([S.ARRAYS[f"picture.{i}"] for i in S.FIXTURE["order"]])) == 0     # live Pillow = recorded
    assert [s["frames_per_batch"] for s in S.FIXTURE["load"][which]["schedules"]] == [1, 3, 5, 7]
    for schedule in S.FIXTURE["load"][which]["schedules"]:
        del launches[:]
        S.run_schedule(node, context, schedule, S.ARRAYS["frames"], lambda t: t.numpy())
        assert launches == [("load", c["count"]) for c in schedule["calls"] if "count" in c]
    assert S.FIXTURE["load"][which]["schedules"][2]["calls"][0]["state"]["total_frames"] == 3                   # min(3, 5 files)


@pytest.mark.parametrize("which", ("video_enhance", "face_fix"))
def test_load_nodes_raise_the_recorded_errors(nodes, tmp_path, which):
    ve, ff, launches = nodes
    node = _loader({"video_enhance": ve, "face_fix": ff}[which], which)
    os.makedirs(tmp_path / "empty")
    contexts = {"missing folder": {"anchor_sources_folder": str(tmp_path / "nowhere")}, "no folder": {},
                "empty folder": {"anchor_sources_folder": str(tmp_path / "empty")}}
    for rec in S.FIXTURE["load"][which]["errors"]:
        mb = S.MetaBatch(2, 9)
        with pytest.raises(FileNotFoundError) as caught:
            node.load(contexts[rec["what"]], mb, 3)
        assert str(caught.value) == rec["text"].replace("{tmp}", str(tmp_path)) and mb.state() == rec["state"]
    assert not launches


def test_the_decode_seam_is_looked_up_when_the_node_runs(nodes, tmp_path, monkeypatch):
    ve, ff, launches = nodes
    sources = S.write_sources(str(tmp_path / "anchor_sources"))
    seen = []

    def loader(path):
        seen.append(os.path.basename(path))
        return S.picture(len(seen), (8, 6))

    for module, node in ((ve, ve.VRGDGVideoEnhanceLoadAnchorsMetaBatch()), (ff, ff.VRGDGFaceFixLoadAnchorsMetaBatch())):
        del seen[:]
        monkeypatch.setattr(module, "image_loader", loader)
        images, masks, count, _ = node.load({"anchor_sources_folder": sources}, S.MetaBatch(2, 9), "n")
        assert seen == ["a_10.bmp", "a_10.bmp", "a_9.PNG"] and tuple(images.shape) == (2, 6, 8, 3) and tuple(masks.shape) == (2, 64, 64)


def test_store_nodes_write_the_recorded_bytes(nodes, tmp_path, monkeypatch):
    """the count error, the folders, which old files go, the file names, the bytes of the files, the context copy; one launch per store"""
    ve, ff, launches = nodes
    x = torch.from_numpy(S.ARRAYS["store.input"].copy())
    from PIL import Image
    # Video Enhance: job_folder/enhanced_anchors through _save_image_batch, image files of an earlier run deleted first
    rec = S.FIXTURE["store"]["video_enhance"]
    job = str(tmp_path / "jobs" / "job_a")
    os.makedirs(os.path.join(job, rec["folder"]))
    for name in rec["stale"]:
        open(os.path.join(job, rec["folder"], name), "wb").close()
    ctx_in = {k: (job if k == "job_folder" else rec["context_in"][k]) for k in rec["context_keys"] if k != "enhanced_anchor_folder"}
    keep = dict(ctx_in)
    folder, joined, count, ctx = ve.VRGDGVideoEnhanceStoreAnchors().store(x, ctx_in)
    assert folder == os.path.join(job, rec["folder"]) and (joined, count) == (rec["indices"], rec["count"])
    assert sorted(os.listdir(folder)) == rec["files_after"] and list(ctx) == rec["context_keys"] and ctx["enhanced_anchor_folder"] == folder
    assert ctx_in == keep and ctx is not ctx_in and {k: ctx[k] for k in keep} == keep
    got = np.stack([np.asarray(Image.open(os.path.join(folder, n)).convert("RGB")) for n in rec["files_after"] if n.endswith(".png")])
    assert np.array_equal(got, S.ARRAYS["store.video_enhance.png"]) and np.array_equal(got, S.store_expected(x.numpy()))
    with pytest.raises(ValueError) as caught:
        ve.VRGDGVideoEnhanceStoreAnchors().store(x[:rec["count_error"]["given"]], ctx_in)
    assert str(caught.value) == rec["count_error"]["text"]
    # Face Fix: <output>/face_fix_standalone/<job>/enhanced_anchors_512, old .png files deleted, anchor_%04d.png through png_writer in B,G,R
    rec = S.FIXTURE["store"]["face_fix"]
    out_dir = tmp_path / "output"
    os.makedirs(out_dir / rec["folder"])
    for name in rec["stale"]:
        open(out_dir / rec["folder"] / name, "wb").close()
    written = []
    real = ff.png_writer
    monkeypatch.setattr(ff, "png_writer", lambda path, data: (written.append((os.path.basename(path), np.array(data))), real(path, data)))
    with S.output_directory(monkeypatch, out_dir):
        folder, joined, count, ctx = ff.VRGDGFaceFixStoreAnchors().store(x, dict(rec["context_in"]))
        with pytest.raises(ValueError) as caught:
            ff.VRGDGFaceFixStoreAnchors().store(x[:rec["count_error"]["given"]], dict(rec["context_in"]))
    assert str(caught.value) == rec["count_error"]["text"]
    assert folder == str(out_dir / rec["folder"]) and (joined, count) == (rec["indices"], rec["count"])
    assert sorted(os.listdir(folder)) == rec["files_after"] and [n for n, _ in written] == rec["written"]
    assert list(ctx) == rec["context_keys"] and ctx["enhanced_anchor_folder"] == folder
    assert np.array_equal(np.stack([d for _, d in written]), S.ARRAYS["store.face_fix.bgr"])
    decoded = np.stack([np.asarray(Image.open(os.path.join(folder, n)).convert("RGB")) for n in rec["written"]])
    assert np.array_equal(decoded, S.ARRAYS["store.face_fix.bgr"][..., ::-1])                                    # the default writer: the same pixels
    assert launches == [("store", 3), ("store", 3)]


def test_collect_follows_the_recorded_logic(nodes, tmp_path):
    ve, _, _ = nodes
    cls = ve.VRGDGVideoEnhanceCollectLTXInputs
    assert any("error" in rec for rec in S.FIXTURE["safe_indices"])
    for rec in S.FIXTURE["safe_indices"]:
        if "error" in rec:
            with pytest.raises(ValueError) as caught:
                cls._safe_indices(rec["indices"], rec["frame_count"])
            assert str(caught.value) == rec["text"]
        else:
            assert cls._safe_indices(rec["indices"], rec["frame_count"]) == rec["result"]
    fx = S.FIXTURE["collect"]
    video, folder = str(tmp_path / "ltx_working_video.mp4"), str(tmp_path / "collected")
    open(video, "wb").close()
    os.makedirs(folder)
    for name in fx["files"]:
        open(os.path.join(folder, name), "wb").close()
    ok = next(run for run in fx["runs"] if run["what"] == "ok")
    prepared = {k: (video if k == "ltx_video_path" else fx["prepared"][k]) for k in ok["context_keys"] if k != "enhanced_anchor_folder"}
    enhanced = dict(fx["enhanced"], enhanced_anchor_folder=folder)
    changes = {"other job": (prepared, dict(enhanced, job_id="job_b")), "no job": (dict(prepared, job_id=""), dict(enhanced, job_id="")),
               "no video": (dict(prepared, ltx_video_path=str(tmp_path / "none.mp4")), enhanced),
               "no folder": (prepared, dict(enhanced, enhanced_anchor_folder=str(tmp_path / "none"))),
               "count": (prepared, dict(enhanced, anchor_indices=[0, 17])), "unsafe": (dict(prepared, frame_count=2), dict(enhanced, anchor_indices=[1, 1, 1]))}
    for run in fx["runs"]:
        if run["what"] == "ok":
            out = cls().collect(prepared, enhanced)
            assert [out[0] == video, out[1] == folder, *out[2:6]] == run["returns"] and list(out[6]) == run["context_keys"]
            assert {k: v for k, v in out[6].items() if k not in ("ltx_video_path", "enhanced_anchor_folder")} == run["context"]
            assert out[6]["enhanced_anchor_folder"] == folder and out[6] is not prepared and prepared["anchor_indices"] == fx["prepared"]["anchor_indices"]
            continue
        with pytest.raises({"ValueError": ValueError, "FileNotFoundError": FileNotFoundError}[run["error"]]) as caught:
            cls().collect(*changes[run["what"]])
        assert str(caught.value) == run["text"].replace("{tmp}", str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------------------------
# surface, mappings, ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_surface_of_the_five_nodes_and_their_mappings(pkg):
    """fails on the parent commit: no ANCHOR_NODE_CLASS_MAPPINGS, none of the five classes"""
    ve = importlib.import_module(PKG_NAME + ".VRGDG_VideoEnhanceNodes")
    ff = importlib.import_module(PKG_NAME + ".VRGDG_StandaloneFaceFixNodes")
    classes, names = {}, {}
    for module in (ve, ff):
        assert set(module.ANCHOR_NODE_CLASS_MAPPINGS) == set(module.ANCHOR_NODE_DISPLAY_NAME_MAPPINGS)
        classes.update(module.ANCHOR_NODE_CLASS_MAPPINGS)
        names.update(module.ANCHOR_NODE_DISPLAY_NAME_MAPPINGS)
    assert tuple(classes) == NODES == tuple(S.FIXTURE["surface"])
    for name, want in S.FIXTURE["surface"].items():
        cls = classes[name]
        assert cls.__name__ == name and callable(getattr(cls, cls.FUNCTION))
        got = {"INPUT_TYPES": _plain(cls.INPUT_TYPES()), "RETURN_TYPES": list(cls.RETURN_TYPES), "RETURN_NAMES": list(cls.RETURN_NAMES),
               "FUNCTION": cls.FUNCTION, "CATEGORY": cls.CATEGORY, "OUTPUT_NODE": bool(getattr(cls, "OUTPUT_NODE", False)), "display_name": names[name]}
        assert got == want, name
    # the pinned mappings keep their keys
    assert set(ve.NODE_CLASS_MAPPINGS) == {"VRGDGVideoEnhanceRestoreOriginal"}
    assert set(ff.NODE_CLASS_MAPPINGS) == {"VRGDGFaceFixComposite", "VRGDGFaceFixCompositeOpaque"}
    assert not set(pkg.NODE_CLASS_MAPPINGS) & set(NODES) and set(pkg.NODE_CLASS_MAPPINGS) == set(pkg.NODE_DISPLAY_NAME_MAPPINGS)


def _plain(value):
    """tuples as lists, as JSON holds them"""
    if isinstance(value, dict):
        return {k: _plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    return value


def test_header_and_bindings_agree_on_the_new_entry_points(ops):
    from comfyui_vrgamedevgirl_amd import _hip
    header = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _hip.load_library()
    assert lib.vrg_abi_version() == 8 == _hip.ABI_VERSION and "#define VRG_ABI_VERSION 8" in header
    for name in NEW_SYMBOLS:
        prototype = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert prototype and name in _hip.EXPORTED_SYMBOLS and hasattr(lib._cdll, name)
        assert len(prototype.group(1).split(",")) == len(_hip._SIGNATURES[name][1]), name
    assert text.index("vrg_anchor_check") > text.index("vrg_assemble_labelled_u8")                              # appended, nothing moved
    assert (_hip.ANCHOR_RGB, _hip.ANCHOR_BGR) == tuple(int(re.search(r"#define VRG_ANCHOR_%s (\d+)" % n, header).group(1)) for n in ("RGB", "BGR"))
    null = C.c_void_p(0)
    one = C.c_void_p(16)
    assert lib.vrg_anchor_frames_f32(null, 0, null, 0, null, 0, null, 4, 4, null) == 0                           # no records: nothing to do
    assert lib.vrg_anchor_frames_f32(null, 8, one, 1, null, 0, one, 4, 4, null) == 1
    assert lib.vrg_anchor_frames_f32(one, 8, one, -1, null, 0, one, 4, 4, null) == 1
    assert lib.vrg_anchor_frames_f32(one, 8, one, 1, null, 0, one, 0, 4, null) == 1
    assert lib.vrg_anchor_store_u8(null, null, 0, 3, 0, null) == 0
    assert lib.vrg_anchor_store_u8(one, one, 4, 2, 0, null) == 1 and lib.vrg_anchor_store_u8(one, one, 4, 3, 2, null) == 1
    assert lib.vrg_anchor_store_u8(null, one, 4, 3, 0, null) == 1 and lib.vrg_anchor_store_u8(one, one, -1, 3, 0, null) == 1

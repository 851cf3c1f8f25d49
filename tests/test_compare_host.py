"""The Video Compare Slider without a GPU: csrc/vrg_compare_math.hpp compiled for the host against numpy running the reference's
expression live; the legacy path resolution against the cases recorded from the reference (tests/golden/compare_paths.json); the
node's surface; compare() with stub seams; the header, the bindings and the entry point's refusals."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

import compare_support as S
from conftest import PKG_NAME, ROOT


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext, ops
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    return ops


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return S.build_host_lib(tmp_path_factory.mktemp("compare_host"))


@pytest.fixture(scope="module")
def node(pkg):
    return importlib.import_module(PKG_NAME + ".VRGDG_VideoCompareNode")


# ---------------------------------------------------------------------------------------------------------------------------------
# the arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rule_equals_numpy_on_the_sweep(host):
    """every k / 255 with both neighbours, (k + 0.5) / 255, 1.0, its upper neighbour and 256 / 255, +-0.0, the smallest subnormal, -1e-30,
    -3, the infinities and NaN: byte for byte what numpy makes of np.clip(x * 255.0, 0, 255).astype(np.uint8), NaN as 0"""
    values = S.sweep()
    assert values.dtype == np.float32 and values.size == 4 * 256 + 11
    x = values.reshape(-1, 1, 1, 1).repeat(3, axis=3)
    want, got = S.expected(x).reshape(-1, 3)[:, 0], S.host_rgb24(host, x).reshape(-1, 3)[:, 0]
    assert np.array_equal(got, want), [(float(v), int(g), int(w)) for v, g, w in zip(values, got, want) if g != w][:8]
    assert host.hm_rgb24_nan_byte() == S.NAN_BYTE == 0
    by_value = {repr(float(v)): int(g) for v, g in zip(values[-11:], got[-11:])}
    assert by_value == {"1.0": 255, "1.0000001192092896": 255, "1.003921627998352": 255, "0.0": 0, "-0.0": 0, "1.401298464324817e-45": 0,
                        "-1.0000000031710769e-30": 0, "-3.0": 0, "inf": 255, "-inf": 0, "nan": 0}


def test_the_sweep_is_not_vacuous(host):
    """Why this kernel exists: the sweep holds values that truncate to k - 1 where the rounding rule of anchor_store_bytes gives k.

    The issue behind this test expected some LEVELS k / 255 to be such values ("(k / 255f) * 255f lands one ulp under k").  None is:
    measured here, 0 of the 256 products lie under k, in fp32 division, in k * fl32(1 / 255) and in the fp64 quotient rounded to fp32
    alike, and live numpy gives k for every level.  The reason is arithmetic, not this code: 1 / 255 is 0.(00000001) in binary, the 24
    significant bits of k / 255 end on a whole period, the first dropped bit is the leading 1 of k, so the quotient always rounds up.
    The assertion "at least one level truncates to k - 1" can therefore hold for no implementation, numpy's included, and is replaced by
    what the sweep does hold: the float just UNDER every level k >= 1 truncates to k - 1 and rounds to k (255 values), and every
    (k + 0.5) / 255 up to 254 truncates to k where rounding -- each of these products is the exact tie k + 0.5 -- gives the even one of
    k and k + 1, so k + 1 for the 127 odd k."""
    k = S.levels()
    ks = np.arange(256)

    def both(values):
        return (S.host_rgb24(host, values.reshape(-1, 1, 1, 1).repeat(3, axis=3)).reshape(-1, 3)[:, 0].astype(np.int64),
                S.host_anchor(host, values).astype(np.int64))
    truncated, rounded = both(k)
    assert np.array_equal(rounded, ks) and np.array_equal(rounded, S.rounded(k))
    print(f"{int((truncated == ks - 1).sum())} of the 256 levels truncate to k - 1; {int((k * np.float32(255.0) < ks).sum())} products lie under k")
    assert np.array_equal(truncated, ks) and (k * np.float32(255.0) >= ks.astype(np.float32)).all()
    under = np.nextafter(k[1:], np.float32(-2))
    truncated, rounded = both(under)
    assert np.array_equal(truncated, ks[1:] - 1) and np.array_equal(rounded, ks[1:]) and np.array_equal(S.expected(under.reshape(-1, 1))[:, 0], ks[1:] - 1)
    half = ((ks[:255] + 0.5) / 255.0).astype(np.float32)
    truncated, rounded = both(half)
    assert np.array_equal(truncated, ks[:255]) and np.array_equal(rounded, S.rounded(half))
    assert np.array_equal(rounded, ks[:255] + ks[:255] % 2)                            # every product is the exact tie k + 0.5: to even
    assert all(np.isin(values, S.sweep()).all() for values in (under, half))           # ... and these values are in the sweep


@pytest.mark.parametrize("channels", (3, 4, 5))
def test_batches_equal_numpy_and_further_channels_are_not_read(host, channels):
    for shape in ((1, 1, 1), (5, 1, 3), (2, 3, 7), (3, 5, 11)):
        x = S.batch(shape + (channels,), seed=sum(shape) + channels)
        x[..., 3:] = np.nan
        assert np.array_equal(S.host_rgb24(host, x), S.expected(x)), shape
    x = S.sweep_batch(channels)
    assert np.array_equal(S.host_rgb24(host, x), S.expected(x)) and np.isnan(x[..., :3]).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the legacy inputs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.FIXTURE["cases"], ids=[c["name"] for c in S.FIXTURE["cases"]])
def test_paths_resolve_as_recorded(node, tmp_path, monkeypatch, case):
    tmp = os.path.realpath(str(tmp_path))
    S.lay_out(tmp, case["files"])
    monkeypatch.setattr(node, "folder_paths", lambda: S.Folders(tmp))
    monkeypatch.chdir(os.path.join(tmp, "cwd"))
    value = S.decoded(case["value"], tmp)
    assert [c.replace(tmp, "{tmp}") for c in node.video_path_candidates(value)] == case["candidates"]
    if "error" in case:
        with pytest.raises(ValueError) as caught:
            node.resolve_video_path(value, S.FIXTURE["label"])
        assert type(caught.value).__name__ == case["error"] and str(caught.value) == case["text"]
    else:
        assert node.resolve_video_path(value, S.FIXTURE["label"]).replace(tmp, "{tmp}") == case["path"]


def test_the_recorded_cases_cover_the_list():
    names = " | ".join(c["name"] for c in S.FIXTURE["cases"])
    for wanted in ("metadata png, silent and -audio mp4", "bare", "dictionary inside a tuple", "missing file", "wrong extension"):
        assert wanted in names
    assert sum("path" in c for c in S.FIXTURE["cases"]) >= 8 and sum("error" in c for c in S.FIXTURE["cases"]) >= 4
    assert sorted(importlib.import_module(PKG_NAME + ".VRGDG_VideoCompareNode").VIDEO_SUFFIXES) == S.FIXTURE["suffixes"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the node
# ---------------------------------------------------------------------------------------------------------------------------------
def _plain(value):
    if isinstance(value, dict):
        return {k: _plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    return value


def test_surface_and_mappings(pkg, node):
    """fails on the parent commit: the module is not there"""
    want = S.FIXTURE["surface"]
    assert list(node.NODE_CLASS_MAPPINGS) == [want["key"]] == list(node.NODE_DISPLAY_NAME_MAPPINGS)
    cls = node.NODE_CLASS_MAPPINGS[want["key"]]
    got = {"key": want["key"], "class": cls.__name__, "display_name": node.NODE_DISPLAY_NAME_MAPPINGS[want["key"]],
           "INPUT_TYPES": _plain(cls.INPUT_TYPES()), "RETURN_TYPES": list(cls.RETURN_TYPES), "RETURN_NAMES": list(cls.RETURN_NAMES),
           "FUNCTION": cls.FUNCTION, "OUTPUT_NODE": cls.OUTPUT_NODE, "CATEGORY": cls.CATEGORY}
    assert got == _plain(want)
    for group in ("required", "optional"):
        assert list(cls.INPUT_TYPES()[group]) == list(want["INPUT_TYPES"][group])                      # widget order
    assert callable(getattr(cls, cls.FUNCTION)) and node.IMAGE_FPS == 24.0
    assert want["key"] not in pkg.NODE_CLASS_MAPPINGS                                                    # a mapping of its own
    assert "folder_paths" not in sys.modules or not hasattr(sys.modules["folder_paths"], "__file__")     # imported without ComfyUI


class _Writer:
    def __init__(self, log, path, width, height, fps):
        self.log, self.path, self.args, self.chunks, self.closed, self.aborted = log, path, (width, height, fps), [], False, False
        log.append(self)

    def write(self, buffer):
        assert isinstance(buffer, memoryview) and not self.closed
        self.chunks.append(bytes(buffer))

    def close(self):
        self.closed = True
        with open(self.path, "wb") as fh:
            fh.write(b"".join(self.chunks))

    def abort(self):
        self.aborted = True


@pytest.fixture()
def stubbed(node, tmp_path, monkeypatch):
    """the node over a temporary folder, a list-collecting writer and a numpy stand-in for ops.stream_rgb24 that hands over two pieces"""
    writers, streamed = [], []

    def stream_rgb24(images, sink, piece_bytes=0):
        data = S.expected(images.numpy().reshape((-1,) + tuple(images.shape[-3:])))
        streamed.append(images)
        cut = max(1, data.shape[0] // 2)
        for part in (data[:cut], data[cut:]):
            if part.size:
                sink(memoryview(np.ascontiguousarray(part).reshape(-1)))
        return data.shape[0]

    monkeypatch.setattr(node, "folder_paths", lambda: S.Folders(tmp_path))
    monkeypatch.setattr(node, "video_writer", lambda path, width, height, fps: _Writer(writers, path, width, height, fps))
    monkeypatch.setattr(node.ops, "stream_rgb24", stream_rgb24)
    return node, writers, streamed


SETTINGS = (0.25, "", "Graded", 1, 0, True, 0.1)


def test_compare_streams_each_image_input_into_its_own_writer(stubbed, tmp_path):
    node, writers, streamed = stubbed
    before, after = torch.from_numpy(S.batch((3, 4, 6, 3), 1)), torch.from_numpy(S.batch((2, 5, 7, 4), 2))
    got = node.VRGDG_VideoCompareSlider().compare(*SETTINGS, before_images=before, after_images=after,
                                                  before_video="never.mp4", after_video="never.mp4")           # legacy inputs are not looked at
    assert [w.args for w in writers] == [(6, 4, 24.0), (7, 5, 24.0)] and all(w.closed and not w.aborted for w in writers)
    assert streamed[0] is before and streamed[1] is after
    assert b"".join(writers[0].chunks) == S.expected(before.numpy()).tobytes() and len(writers[0].chunks) == 2
    assert b"".join(writers[1].chunks) == S.expected(after.numpy()).tobytes()
    temp = os.path.join(str(tmp_path), "temp")
    for w, role in zip(writers, ("before", "after")):
        assert os.path.dirname(w.path) == temp and re.fullmatch(rf"vrgdg_compare_{role}_[0-9a-f]{{32}}\.mp4", os.path.basename(w.path))
    paths = [w.path for w in writers]
    assert list(got) == ["ui", "result"] and list(got["ui"]) == ["compare_videos", "compare_video_settings"]
    assert got["ui"]["compare_videos"] == [{"compare_role": role, "path": p, "name": os.path.basename(p)} for role, p in zip(("before", "after"), paths)]
    assert got["ui"]["compare_video_settings"] == {"slider_position": 0.25, "before_label": "Before", "after_label": "Graded", "show_labels": True,
                                                   "loop": False, "muted": True, "record_duration": 0.5}
    assert [type(v) for v in got["ui"]["compare_video_settings"].values()] == [float, str, str, bool, bool, bool, float]
    assert got["result"] == ((True, [paths[0]]), (True, [paths[1]]))


def test_compare_uses_a_legacy_input_only_where_the_image_input_is_absent(stubbed, tmp_path):
    node, writers, streamed = stubbed
    S.lay_out(str(tmp_path), ["output/old_00001.png", "output/old_00001.mp4"])
    legacy = (True, [os.path.join(str(tmp_path), "output", "old_00001.png"), os.path.join(str(tmp_path), "output", "old_00001.mp4")])
    after = torch.from_numpy(S.batch((4, 6, 3), 3))                                                             # one [H, W, C] frame
    got = node.VRGDG_VideoCompareSlider().compare(*SETTINGS, before_video=legacy, after_images=after)
    assert len(writers) == 1 and writers[0].args == (6, 4, 24.0) and len(streamed) == 1
    assert b"".join(writers[0].chunks) == S.expected(after.numpy()).tobytes()
    assert got["result"] == ((True, [os.path.realpath(legacy[1][1])]), (True, [writers[0].path]))
    with pytest.raises(ValueError, match=r"^After video was not found\. Connect the Filenames output from a Video Combine node that has "
                                         r"already created a video\.$"):
        node.VRGDG_VideoCompareSlider().compare(*SETTINGS, before_video=legacy)
    with pytest.raises(ValueError, match=r"^Before video was not found\."):
        node.VRGDG_VideoCompareSlider().compare(*SETTINGS, after_images=after)


def test_compare_refuses_as_the_reference_does(stubbed, monkeypatch):
    node, writers, _ = stubbed
    for bad in (torch.zeros((0, 4, 4, 3)), torch.zeros((2, 4, 4, 2)), torch.zeros((4, 4)), torch.zeros((1, 2, 4, 4, 3))):
        with pytest.raises(ValueError, match=r"^before image input must be a non-empty IMAGE batch\.$"):
            node.VRGDG_VideoCompareSlider().compare(*SETTINGS, before_images=bad, after_images=torch.zeros((1, 4, 4, 3)))
    with pytest.raises(ValueError, match=r"^after image input must be a non-empty IMAGE batch\.$"):
        node.VRGDG_VideoCompareSlider().compare(*SETTINGS, before_images=torch.zeros((1, 4, 4, 3)), after_images=torch.zeros((0, 4, 4, 3)))
    # a sink that fails: the writer is abandoned, not closed, and the exception is the sink's own
    del writers[:]
    boom = OSError("broken pipe")
    monkeypatch.setattr(_Writer, "write", lambda self, buffer: (_ for _ in ()).throw(boom))
    with pytest.raises(OSError) as caught:
        node.VRGDG_VideoCompareSlider().compare(*SETTINGS, before_images=torch.zeros((1, 4, 4, 3)), after_images=torch.zeros((1, 4, 4, 3)))
    assert caught.value is boom and len(writers) == 1 and writers[0].aborted and not writers[0].closed


def test_the_default_writer_is_the_references_ffmpeg_pipe(node, tmp_path, monkeypatch):
    monkeypatch.setattr(node, "find_ffmpeg", lambda: None)
    with pytest.raises(RuntimeError, match=r"^The compare slider needs FFmpeg to convert IMAGE batches into a browser-playable video\.$"):
        node.video_writer(str(tmp_path / "x.mp4"), 8, 6, 24.0)
    # a stand-in executable that copies its stdin to the output path named last, then one that fails
    fake = tmp_path / "ffmpeg"
    fake.write_text("#!/bin/sh\nprintf '%s\\n' \"$@\" > \"$0.args\"\nfor last; do :; done\ncat > \"$last\"\n")
    fake.chmod(0o755)
    monkeypatch.setattr(node, "find_ffmpeg", lambda: str(fake))
    out = str(tmp_path / "y.mp4")
    writer = node.video_writer(out, 8, 6, 0.5)
    writer.write(memoryview(b"abc"))
    writer.write(memoryview(b"def"))
    writer.close()
    assert open(out, "rb").read() == b"abcdef"
    assert open(str(fake) + ".args").read().split("\n")[:-1] == ["-y", "-f", "rawvideo", "-vcodec", "rawvideo", "-pix_fmt", "rgb24", "-s", "8x6",
                                                                 "-r", "1.0", "-i", "-", "-an", "-c:v", "libx264", "-pix_fmt", "yuv420p",
                                                                 "-movflags", "+faststart", out]
    fake.write_text("#!/bin/sh\ncat > /dev/null\necho 'no such encoder' >&2\nexit 3\n")
    writer = node.video_writer(out, 8, 6, 24.0)
    writer.write(memoryview(b"abc"))
    with pytest.raises(RuntimeError, match=r"^FFmpeg could not create the compare video: no such encoder\n$"):
        writer.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# header, bindings, refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_agree_on_the_new_entry_point(ops):
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    header = open(os.path.join(ROOT, "include", "vrgdg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _hip.load_library()
    name = "vrg_rgb24_frames_u8"
    prototype = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
    assert prototype and name in _hip.EXPORTED_SYMBOLS and hasattr(lib._cdll, name)
    assert len(prototype.group(1).split(",")) == len(_hip._SIGNATURES[name][1]) == 5
    assert lib.vrg_abi_version() == 8 == _hip.ABI_VERSION and text.index(name) > text.index("vrg_guidance_rescale_f32")     # appended, nothing moved
    assert "vrg_compare.hip" in build_ext.SOURCES and "vrg_compare_math.hpp" in build_ext.HEADERS
    null, one, two = C.c_void_p(0), C.c_void_p(16), C.c_void_p(1 << 30)          # never dereferenced: validation fails or sizes are zero
    assert lib.vrg_rgb24_frames_u8(null, null, 0, 3, null) == 0                  # zero pixels: nothing to do
    assert lib.vrg_rgb24_frames_u8(null, two, 4, 3, null) == 1 and lib.vrg_rgb24_frames_u8(one, null, 4, 3, null) == 1
    assert lib.vrg_rgb24_frames_u8(one, two, 4, 2, null) == 1 and lib.vrg_rgb24_frames_u8(one, two, -1, 3, null) == 1
    assert lib.vrg_rgb24_frames_u8(C.c_void_p(18), two, 4, 3, null) == 1         # a source off the 4-byte grid
    assert lib.vrg_rgb24_frames_u8(one, one, 4, 3, null) == 1                    # overlapping operands
    assert lib.vrg_rgb24_frames_u8(one, C.c_void_p(16 + 4 * 3 * 4 - 1), 4, 3, null) == 1       # dst begins at the source's last byte
    assert lib.vrg_rgb24_frames_u8(one, two, 1 << 61, 4, null) == 2              # sizes that do not fit


def test_the_operators_refuse_on_the_host(ops):
    for name in ("rgb24_frames", "stream_rgb24"):
        args = () if name == "rgb24_frames" else (lambda view: None,)
        for bad in (torch.zeros((0, 4, 4, 3)), torch.zeros((2, 4, 4, 2)), torch.zeros((2, 0, 4, 3)), torch.zeros((4, 4))):
            with pytest.raises(ValueError, match=rf"^{name} image input must be a non-empty IMAGE batch\.$"):
                getattr(ops, name)(bad, *args)
    with pytest.raises(ValueError, match="float32"):
        ops.stream_rgb24(torch.zeros((1, 4, 4, 3), dtype=torch.float16), lambda view: None)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            ops.rgb24_frames(torch.zeros((1, 4, 4, 3)))

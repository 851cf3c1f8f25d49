"""The Video Folder Grid Plot on the MI355X: vrg_grid_tiles_f32 / _u8 through the ABI, ops.video_grid and the node against the numpy
restatement of tests/grid_support.py.  Every comparison is bit-equality of fp32; every output is allocated with a NaN fill and guard
floats before and after, the guards must be untouched and no NaN may remain."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import grid_support as G

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 64


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


@pytest.fixture(scope="module")
def node_module(pkg):
    from comfyui_vrgamedevgirl_amd import LTXLoraTrain
    return LTXLoraTrain


@pytest.fixture(scope="module")
def golden():
    with open(G.golden_paths()[0]) as fh:
        return json.load(fh), np.load(G.golden_paths()[1])


def guarded(shape, device="cuda"):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=device)
    flat[:GUARD] = 77.0
    flat[GUARD + n:] = 77.0
    return flat, flat[GUARD:GUARD + n].view(shape)


def check_guarded(flat, view):
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == 77.0).all()) and bool((flat[-GUARD:] == 77.0).all()), "a guard float was written"
    got = view.cpu().numpy()
    assert not np.isnan(got).any(), "a float of the output was never written"
    return got


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == F32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} floats differ"


def run_tiles(ops, sources, tile_hw, cell=None, offsets=None, byte_sources=False, columns=1, overlays=None, band=0):
    """sources: device tensors [n, H, W, C], one tile each, through the ABI entry with a hand-made plan: the tile is exactly tile_hw at
    `offsets` inside a cell of `cell` (default: the tile itself)."""
    from comfyui_vrgamedevgirl_amd import _hip
    h, w = tile_hw
    cell_h, cell_w = cell or tile_hw
    x_off, y_off = offsets or (0, 0)
    tiles = []
    for s in sources:
        H, W, Cn = (int(v) for v in s.shape[1:])
        mode, cps, inv = C.c_int32(), C.c_int32(), C.c_float()
        _hip.check(_hip.load_library().vrg_grid_plan(H, W, Cn, h, w, C.byref(mode), C.byref(cps), C.byref(inv)), "vrg_grid_plan")
        tiles.append(ops.GridTile(H, W, Cn, w, h, x_off, y_off, mode.value, cps.value, inv.value, ops.grid_taps(W, w, mode.value),
                                  ops.grid_taps(H, h, mode.value)))
    plan = ops.GridPlan(cell_w, cell_h, columns, -(-len(sources) // columns), band, tuple(tiles))
    frames = max(int(s.shape[0]) for s in sources)
    flat, out = guarded((frames, plan.grid_h, plan.grid_w, 3))
    dev_overlays, has = ops._grid_overlays(plan, overlays, out.device)
    jobs = [(None, cell_i, None, 0, np.full(frames, -1)) for cell_i in range(len(sources), plan.rows * columns)]
    jobs += [(i, i, s, 0, np.minimum(np.arange(frames), int(s.shape[0]) - 1)) for i, s in enumerate(sources)]
    ops._grid_launch(plan, out, jobs, dev_overlays, has, byte_sources)
    return check_guarded(flat, out), plan


def expected(plan, sources_np, frames, overlays=None):
    want = np.zeros((frames, plan.grid_h, plan.grid_w, 3), dtype=F32)
    for i, (s, t) in enumerate(zip(sources_np, plan.tiles)):
        y0, x0 = (i // plan.columns) * plan.cell_h, (i % plan.columns) * plan.cell_w
        for f in range(frames):
            tile = G.tile_floats(s[min(f, len(s) - 1)], (t.new_h, t.new_w))
            want[f, y0 + t.y_off:y0 + t.y_off + t.new_h, x0 + t.x_off:x0 + t.x_off + t.new_w] = tile
            if overlays is not None and overlays[i] is not None:
                want[f, y0:y0 + plan.band, x0:x0 + plan.cell_w] = overlays[i].astype(F32) / F32(255.0)
    return want


@pytest.mark.parametrize("src,tile,mode", G.GEOMETRIES)
@pytest.mark.parametrize("channels", (3, 4))
def test_geometry_sweep(ops, src, tile, mode, channels):
    """every rule, C = 3 and 4, uniform / smooth / special frames as three frames of one batch.  A wave stages at most 4096 source values
    (GRID_ROW_VALUES) at a time: 4 x 20000 -> 2 x 9000 needs about 430 per workgroup and is split across workgroups only, while
    4 x 4000 -> 2 x 64 and 8 x 3840 -> 4 x 120 need more and go through the row buffer in segments of columns (cps < 64)"""
    H, W = src
    x = np.concatenate([G.FRAME_KINDS[kind]((1, H, W, channels), 900 + H + W) for kind in ("uniform", "smooth", "special")])
    keep = x.copy()
    dev = torch.from_numpy(x).cuda()
    got, plan = run_tiles(ops, [dev], tile)
    assert plan.tiles[0].mode == mode and (plan.tiles[0].cps < 64) == ((src, tile) in G.SEGMENTED)
    same_bits(got, expected(plan, [x], 3))
    assert np.array_equal(dev.cpu().numpy(), keep, equal_nan=True)


@pytest.mark.parametrize("shift", (1, 2, 3))
def test_source_alignment_and_views(ops, shift):
    """the source base 4, 8 and 12 bytes off the 16-byte grid, as a view into a larger batch"""
    H, W = 70, 131
    big = torch.from_numpy(G.uniform_frames((1, 5 * H * W * 3 + 8), 41)[0]).cuda()
    view = big[shift:shift + 4 * H * W * 3].view(4, H, W, 3)[1:3]
    assert view.data_ptr() % 16 == (4 * (shift + H * W * 3)) % 16 and view.is_contiguous()
    got, plan = run_tiles(ops, [view], (30, 57))
    same_bits(got, expected(plan, [view.cpu().numpy()], 2))


def test_destination_phases_and_odd_offsets(ops):
    """cell_w = 35 with 3 columns: the tiles start off the 16-byte grid at every phase; x_off odd; bars, band rows and the empty cell are 0"""
    srcs = [G.uniform_frames((2, 40, 60, 3), 50 + i) for i in range(5)]
    overlays = [G.pattern_label(f"t{i}", 35, 30, 6)[:6] if i != 2 else None for i in range(5)]
    got, plan = run_tiles(ops, [torch.from_numpy(s).cuda() for s in srcs], (20, 30), cell=(30, 35), offsets=(3, 7), columns=3, overlays=overlays, band=6)
    assert (plan.grid_w, plan.grid_h) == (105, 60)
    want = expected(plan, srcs, 2, overlays)
    same_bits(got, want)
    assert not want[:, 30:, 70:].any() and not got[:, 30:, 70:].any()                       # the empty sixth cell
    assert want[:, :6, :35].any() and not got[:, :6, 70:105].any()                          # a label band, and the tile without one


def test_grid_rules_through_ops(ops):
    """5 tiles in 3 columns, batches of 3, 1 and 5 frames, mixed sizes, an [H, W, C] input, labels from a patterned renderer"""
    batches = [G.uniform_frames((3, 48, 64, 3), 1), G.smooth_frames((1, 30, 40, 3), 2), G.uniform_frames((5, 96, 128, 4), 3),
               G.uniform_frames((1, 70, 131, 3), 4)[0], G.special_frames((2, 12, 20, 3), 5)]
    band, cw, ch = 40, 64, 88
    overlays = [G.pattern_label(f"video{i + 1}", cw, ch, band)[:band] for i in range(5)]
    want = G.grid_frames(batches, cw, ch, 3, band, overlays)
    dev = [torch.from_numpy(b).cuda() for b in batches]
    flat, out = guarded(want.shape)
    assert ops.video_grid(dev, cw, ch, 3, band, overlays, out=out) is out
    got = check_guarded(flat, out)
    same_bits(got, want)
    assert not got[:, ch:, 2 * cw:].any()
    same_bits(got[4, :, :cw], got[2, :, :cw])                                               # the ended batch holds its last frame
    for b, d in zip(batches, dev):
        assert np.array_equal(d.cpu().numpy(), b, equal_nan=True)


def test_golden_cases_device_resident_and_host_fed(ops, golden, monkeypatch):
    """the reference's own grids: device-resident and host-fed give the same bits; inputs unchanged; PIPE_BYTES set so that a batch goes
    through the page-locked ring in pieces of two frames"""
    from comfyui_vrgamedevgirl_amd import _devices
    meta, grids = golden
    for case in meta["cases"]:
        batches = G.golden_inputs(case)
        cw, ch = case["resolved_cell"]
        band = G.LABEL_BAND if case["label_tiles"] else 0
        overlays = [G.pattern_label(t, cw, ch, band)[:band] for t in case["labels"]] if band else None
        cpu = [torch.from_numpy(b.copy()) for b in batches]
        if case.get("raises"):
            with pytest.raises(ValueError):
                ops.video_grid(cpu, cw, ch, case["columns"], band, overlays)
            continue
        want = grids[case["key"]].astype(F32) / F32(255.0)
        flat, out = guarded(want.shape)
        ops.video_grid([t.cuda() for t in cpu], cw, ch, case["columns"], band, overlays, out=out)
        same_bits(check_guarded(flat, out), want)
        largest = max(int(np.prod(b.shape[-3:])) * 4 for b in batches)
        monkeypatch.setattr(_devices, "PIPE_BYTES", 2 * largest)
        flat, out = guarded(want.shape)
        ops.video_grid(cpu, cw, ch, case["columns"], band, overlays, out=out)
        same_bits(check_guarded(flat, out), want)
        for t, b in zip(cpu, batches):
            assert np.array_equal(t.numpy(), b, equal_nan=True)


def test_node(node_module, monkeypatch):
    """the node under torch.inference_mode(): CPU inputs, labels through the seam, the four-tuple of the reference; a renderer that writes
    below the band raises"""
    monkeypatch.setattr(node_module, "render_label", G.pattern_label)
    node = node_module.VRGDG_VideoFolderGridPlot()
    batches = [G.uniform_frames((3, 48, 64, 3), 11), G.smooth_frames((2, 96, 128, 3), 12), G.uniform_frames((1, 30, 40, 3), 13)[0]]
    with torch.inference_mode():
        inputs = {"video1": torch.from_numpy(batches[0]), "video3": [torch.from_numpy(batches[1]), {"k": torch.from_numpy(batches[2])}], "label_2": "second"}
        images, prefix, fps, status = node.run("", "my grid", "", 3, 0, 0, True, 30, **inputs)
    labels = ["video1", "second", "video3"]
    want = G.grid_frames(batches, 64, 88, 2, 40, [G.pattern_label(t, 64, 88, 40)[:40, :, ::-1] for t in labels])     # the renderer draws in B,G,R
    assert images.device.type == "cpu" and (prefix, fps) == ("my_grid", 30)
    assert status == "Created grid image sequence from 3 connected video/image input(s)."
    same_bits(images.numpy(), want)
    monkeypatch.setattr(node_module, "render_label", lambda text, w, h, band: np.full((h, w, 3), 1, dtype=np.uint8))
    with pytest.raises(ValueError, match="leaves the 40-row band"):
        node.run("", "g", "", 1, 0, 0, True, 30, video1=torch.from_numpy(batches[0]))


class FakeCapture:
    def __init__(self, frames):
        self.frames, self.at, self.released = list(frames), 0, False

    def read(self):
        if self.at >= len(self.frames):
            return False, None
        self.at += 1
        return True, self.frames[self.at - 1]

    def release(self):
        self.released = True


def test_byte_input_and_the_folder_branch(ops, node_module, monkeypatch, tmp_path):
    """decoded B,G,R frames of unequal length, one video without a frame: equals vrg_grid_tiles_f32 on the same frames / 255 and the
    restatement; the loop ends where the reference's does (the longest video); pieces of 2 output frames"""
    videos = {"a.mp4": G.bytes_frames((5, 36, 52, 3), 21), "b.mov": G.bytes_frames((2, 70, 131, 3), 22), "c.mkv": np.zeros((0, 8, 8, 3), np.uint8),
              "d.avi": G.bytes_frames((3, 12, 20, 3), 23)}
    for name in list(videos) + ["skip_XYZ_COMPARE_1.mp4", "notes.txt"]:
        (tmp_path / name).write_text("x")
    captures = []

    def fake_open(path):
        captures.append(FakeCapture(videos[path.rsplit("/", 1)[-1]]))
        return captures[-1]

    monkeypatch.setattr(node_module, "open_capture", fake_open)
    monkeypatch.setattr(node_module, "render_label", G.pattern_label)
    monkeypatch.setattr(node_module, "FOLDER_PIECE_FRAMES", 2)
    node = node_module.VRGDG_VideoFolderGridPlot()
    images, prefix, fps, status = node.run(str(tmp_path), "", "", 4, 64, 88, True, 24)
    assert status == "Created grid image sequence from 4 videos." and all(c.released for c in captures) and tuple(images.shape) == (5, 176, 128, 3)
    names = ["a", "b", "c", "d"]
    overlays = [G.pattern_label(t, 64, 88, 40)[:40, :, ::-1] for t in names]                 # the renderer draws in B,G,R
    as_float = [v[..., ::-1].astype(F32) / F32(255.0) if len(v) else np.zeros((1, 48, 64, 3), F32) for v in videos.values()]
    same_bits(images.numpy(), G.grid_frames(as_float, 64, 88, 2, 40, overlays))
    same_bits(images.numpy(), ops.video_grid([torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in as_float], 64, 88, 2, 40, overlays).cpu().numpy())


def test_chunked_launch(ops):
    """more descriptors than one launch takes (32768): 8 x 8 sources, 4 x 4 tiles, 2 tiles x 16500 output frames"""
    frames = 16500
    a, b = G.uniform_frames((3, 8, 8, 3), 61), G.uniform_frames((2, 8, 8, 3), 62)
    dev = [torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()]
    tile = ops.GridTile(8, 8, 3, 4, 4, 0, 0, G.FAST_2X2, 64, 0.25, ops.grid_taps(8, 4, G.FAST_2X2), ops.grid_taps(8, 4, G.FAST_2X2))
    plan = ops.GridPlan(4, 4, 2, 1, 0, (tile, tile))                                        # the tile is the cell: a hand-made plan
    index = [np.arange(frames) % 3, np.arange(frames) % 2]
    flat, out = guarded((frames, 4, 8, 3))
    ops._grid_launch(plan, out, [(0, 0, dev[0], 0, index[0]), (1, 1, dev[1], 0, index[1])], None, [False, False], False)
    got = check_guarded(flat, out)
    ta = np.stack([G.tile_floats(f, (4, 4)) for f in a])
    tb = np.stack([G.tile_floats(f, (4, 4)) for f in b])
    same_bits(got[:, :, :4], ta[index[0]])
    same_bits(got[:, :, 4:], tb[index[1]])

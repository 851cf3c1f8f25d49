"""Host-side logic that needs no GPU: generator bookkeeping, .cube I/O, blend terms, staging groups,
statistics merging."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import philox as PH
from oracle import restated as R
from conftest import GOLDEN, ROOT


class FakeGen:
    def __init__(self, seed=1234, offset=0):
        self.seed, self.offset = seed, offset

    def initial_seed(self):
        return self.seed

    def get_offset(self):
        return self.offset

    def set_offset(self, v):
        self.offset = v


def test_rng_geometry_matches_oracle_restatement(pkg):
    from comfyui_vrgamedevgirl_amd import rng
    geom = rng.DeviceGeometry(256, 2048)
    assert geom.max_grid == 2048
    for numel in (1, 255, 256, 257, 3 * 512 * 512, 4 * 1080 * 1920 * 3, 4 * 2160 * 3840 * 3, 536870911):
        G = rng.grid_threads(numel, geom)
        assert G == PH.torch_grid_threads(numel, 256)
        assert rng.counter_offset(numel, G) == PH.torch_counter_offset(numel, G)
        plan, new_off = PH.torch_randn_plan(numel, 40, 256)
        assert plan == [(0, numel, G, 40)] and new_off == 40 + rng.counter_offset(numel, G)
    assert rng.grid_threads(4 * 2160 * 3840 * 3, geom) == 524288


def test_rng_reserve_advances_generator_like_successive_randn_calls(pkg):
    from comfyui_vrgamedevgirl_amd import rng
    geom = rng.DeviceGeometry(256, 2048)
    gen = FakeGen(seed=99, offset=12)
    numel = 4 * 64 * 64 * 3
    s = rng.reserve(numel, 5, torch.device("cpu"), generator=gen, geom=geom)
    G = PH.torch_grid_threads(numel, 256)
    step = PH.torch_counter_offset(numel, G)
    assert (s.seed, s.offset0, s.offset_stride, s.grid_threads, s.seed_stride) == (99, 12, step, G, 0)
    assert gen.offset == 12 + 5 * step
    with pytest.raises(ValueError):
        rng.reserve(rng.MAX_CHUNK_NUMEL + 1, 1, torch.device("cpu"), generator=gen, geom=geom)      # such chunks: reserve_split


def test_oversized_randn_is_split_like_aten(pkg):
    """A randn beyond 2^29 elements: the same leaves, grids and generator offsets as the oracle's restatement of
    TensorIterator::with_32bit_indexing + distribution_nullary_kernel (the outer call consumes an offset first)."""
    from comfyui_vrgamedevgirl_amd import ops, rng
    geom = rng.DeviceGeometry(256, 2048)
    for n in (2 ** 29 + 1, 22 * 2160 * 3840 * 3, 3 * 536870911, 500 * 1080 * 1920 * 3, 2 ** 31 + 5):
        parts = PH.split_32bit(n)
        assert rng.split_32bit(n) == parts
        assert sum(l for _, l in parts) == n and all(l <= 2 ** 29 for _, l in parts)
        assert [s for s, _ in parts] == sorted(s for s, _ in parts)
        plan, off = PH.torch_randn_plan(n, 40, 256)
        gen = FakeGen(seed=7, offset=40)
        sp = rng.reserve_split(n, torch.device("cpu"), generator=gen, geom=geom)
        assert sp.leaves == plan and gen.offset == off and plan[0][3] > 40
    assert rng.split_32bit(2 ** 29) == [(0, 2 ** 29)]
    fe = 2160 * 3840 * 3
    assert not ops.oversize_chunks(256, fe, 4) and not ops.oversize_chunks(21, fe, 0)
    assert ops.oversize_chunks(22, fe, 0) and ops.oversize_chunks(256, fe, 22) and ops.oversize_chunks(87, 1080 * 1920 * 3, 0)


def test_plan_noise_full_and_tail_chunks(pkg, monkeypatch):
    from comfyui_vrgamedevgirl_amd import ops, rng
    geom = rng.DeviceGeometry(256, 2048)
    monkeypatch.setattr(rng, "device_geometry", lambda device=None: geom)
    gen = FakeGen(seed=5, offset=0)
    fe = 12 * 16 * 3
    main, tail, n_full = ops.plan_noise(7, fe, 3, torch.device("cpu"), gen)
    assert n_full == 2 and main.chunk_frames == 3 and tail.chunk_frames == 1
    assert main.stream.offset0 == 0 and tail.stream.offset0 == 2 * main.stream.offset_stride
    assert gen.offset == tail.stream.offset0 + rng.counter_offset(fe, rng.grid_threads(fe, geom))
    main, tail, n_full = ops.plan_noise(4, fe, 0, torch.device("cpu"), FakeGen())
    assert n_full == 1 and main.chunk_frames == 4 and tail is None
    main, tail, n_full = ops.plan_noise(2, fe, 8, torch.device("cpu"), FakeGen())
    assert n_full == 1 and main.chunk_frames == 2 and tail is None      # batch_size > F: one chunk of F


def test_blend_terms(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    assert ops.blend_terms(0.0)[0] == 0 and ops.blend_terms(-3)[0] == 0
    assert ops.blend_terms(10.0) == (1, 1.0, 0.0) and ops.blend_terms(99)[0] == 1
    mode, B, omB = ops.blend_terms(3.3)
    assert mode == 2 and B == float(np.float32(0.33)) and omB == float(np.float32(1.0 - 0.33))
    assert R.lut_blend_factor(3.3) == 3.3 / 10.0 and B == float(np.float32(3.3 / 10.0)) and omB == float(np.float32(1.0 - 3.3 / 10.0))


@pytest.mark.parametrize("fname", ["synthetic_17.cube", "synthetic_domain_9.cube"])
def test_cube_parser_matches_oracle(pkg, fname):
    from comfyui_vrgamedevgirl_amd import cube
    a = cube.parse_cube_file(os.path.join(GOLDEN, fname))
    b = R.parse_cube_file(os.path.join(GOLDEN, fname))
    assert a["size"] == b["size"]
    for k in ("lut", "domain_min", "domain_max"):
        assert torch.equal(a[k], b[k]) and a[k].dtype == torch.float32


def test_cube_writer_roundtrip_and_errors(pkg, tmp_path):
    from comfyui_vrgamedevgirl_amd import cube
    table = cube.build_palette_lut("#0b1d51, #1f6aa5, #f3d27a", 9)
    assert table.shape == (9, 9, 9, 3) and table.dtype == torch.float32 and 0 <= table.min() and table.max() <= 1
    path = str(tmp_path / "sub" / "x.cube")
    cube.write_cube_file(table, path)
    back = cube.parse_cube_file(path)
    assert back["size"] == 9 and (back["lut"] - table).abs().max() <= 5.1e-7      # %.6f text
    assert torch.equal(back["lut"], R.parse_cube_file(path)["lut"])
    assert cube.next_available_lut_path(str(tmp_path / "sub"), "x").endswith("x_2.cube")
    assert cube.sanitize_filename_part("  #FF 88/00 ") == "ff_88_00" and cube.sanitize_filename_part("") == "custom"
    assert np.allclose(cube.parse_hex_color("teal"), [0, 128 / 255, 128 / 255]) and np.allclose(cube.parse_hex_color("#fff"), 1)
    for bad in ("#12345", "nope", "#gggggg"):
        with pytest.raises(ValueError):
            cube.parse_hex_color(bad)
    with pytest.raises(ValueError):
        cube.parse_color_list(" , ")
    p = tmp_path / "b.cube"
    for text in ("LUT_1D_SIZE 2\n", "0 0 0\n", "LUT_3D_SIZE 2\n0 0 0\n", "LUT_3D_SIZE 2 2\n", "LUT_3D_SIZE 2\nDOMAIN_MIN 0 0\n"):
        p.write_text(text)
        with pytest.raises(ValueError):
            cube.parse_cube_file(str(p))


def test_cube_parser_on_shipped_reference_assets(pkg, tmp_path):
    """The reference's 12 shipped cube files (tests/golden/reference_luts/, gzip of the files as shipped), parsed by the pack and the oracle."""
    import gzip
    from comfyui_vrgamedevgirl_amd import cube
    src = os.path.join(GOLDEN, "reference_luts")
    names = sorted(n[:-3] for n in os.listdir(src) if n.endswith(".cube.gz"))
    assert len(names) == 12
    for name in names:
        path = tmp_path / name
        with gzip.open(os.path.join(src, name + ".gz"), "rb") as fh:
            path.write_bytes(fh.read())
        a = cube.parse_cube_file(str(path))
        b = R.parse_cube_file(str(path))
        assert torch.equal(a["lut"], b["lut"]) and torch.equal(a["domain_min"], b["domain_min"]), name


def test_palette_lut_matches_reference_generator(pkg):
    """The reference's _build_palette_lut on three palettes, recorded from a live run of it (tests/golden/reference_nodes.*)."""
    import json
    from comfyui_vrgamedevgirl_amd import cube
    z = np.load(os.path.join(GOLDEN, "reference_nodes.npz"))
    with open(os.path.join(GOLDEN, "reference_nodes.json")) as fh:
        cases = json.load(fh)["palette"]
    assert [(c["colors"], c["n"]) for c in cases] == [("#0b1d51, #1f6aa5, #f3d27a", 8), ("red", 9), ("teal, orange", 11)]
    for i, c in enumerate(cases):
        assert torch.equal(cube.build_palette_lut(c["colors"], c["n"]), torch.from_numpy(z[f"palette.{i}"])), c


def test_frame_groups(pkg):
    from comfyui_vrgamedevgirl_amd import _devices as D
    fb = 2160 * 3840 * 3 * 4
    groups = list(D.frame_groups(37, fb, multiple_of=4))
    assert groups[0][0] == 0 and groups[-1][1] == 37
    assert all(a1 == b0 for (_, a1), (b0, _) in zip(groups, groups[1:]))
    assert all((e - s) % 4 == 0 for s, e in groups[:-1]) and all((e - s) * fb <= max(D.STAGE_BYTES, 4 * fb) for s, e in groups)
    assert list(D.frame_groups(0, fb)) == []


def test_merge_stats_is_chan(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    g = np.random.default_rng(0)
    data = g.normal(50, 20, size=(4, 1000))
    parts = torch.tensor([[len(d), d.mean(), ((d - d.mean()) ** 2).sum()] for d in data], dtype=torch.float64)
    merged = ops.merge_stats(parts)
    allv = data.reshape(-1)
    assert merged[0].item() == allv.size
    assert abs(merged[1].item() - allv.mean()) < 1e-10
    assert abs(merged[2].item() - ((allv - allv.mean()) ** 2).sum()) < 1e-6


def test_adjust_normalization_and_terms(pkg):
    """Host mirror of _normalize_adjust_settings (reference fixture) and the descriptor terms the kernels get."""
    import json
    from comfyui_vrgamedevgirl_amd import VRGDG_LUTVideoTools as LVT, ops
    with open(os.path.join(GOLDEN, "adjust_normalized.json")) as fh:
        want = json.load(fh)
    with open(os.path.join(GOLDEN, "adjust_cases.json")) as fh:
        cases = json.load(fh)["cases"]
    for name, settings in cases.items():
        assert LVT._normalize_adjust_settings(settings) == want[name], name
    assert LVT._normalize_adjust_settings("nope") == want["not_a_dict"]
    d = ops.adjust_terms(LVT._normalize_adjust_settings(cases["all"]))
    f32 = lambda v: float(np.float32(v))
    assert d.enabled == 1 and d.has_clarity == 1 and d.has_sharpen == 1 and d.has_fade == 1 and d.has_vignette == 1
    assert d.shift[0] == f32(-12.5 / 400.0 - 8.0 / 900.0) and d.shift[1] == f32(8.0 / 450.0)
    assert d.shift[2] == f32(12.5 / 400.0 - 8.0 / 900.0)
    assert d.exposure == f32(2.0 ** (-9.0 / 100.0)) and d.fade_mul == f32(1.0 - 0.09 * 0.35) and d.fade_add == f32(0.09 * 0.18)
    t = ops.adjust_terms(LVT._normalize_adjust_settings(cases["thresholds"]))   # the reference's > 0.001 / > 0 gates
    assert t.has_clarity == (1 if abs(0.1 / 100.0) > 0.001 else 0) and t.has_sharpen == (1 if 0.1 / 100.0 > 0.001 else 0)
    assert t.has_fade == 1 and t.has_vignette == 1
    off = ops.adjust_terms(LVT._normalize_adjust_settings(cases["disabled"]))
    assert off.enabled == 0


def test_opening_match_host_terms_cube_and_weight(pkg):
    """Host side of the opening colour match mirror against the reference fixtures (statistics need the GPU: -m gpu)."""
    import hashlib
    import json
    from comfyui_vrgamedevgirl_amd import VRGDG_WorkflowRunnerNodes as WR
    z = np.load(os.path.join(GOLDEN, "opening_match.npz"))
    with open(os.path.join(GOLDEN, "opening_match.json")) as fh:
        meta = json.load(fh)
    for name, m in meta.items():
        rs, ts = R.image_stat_rgb(z[f"{name}.ref"]), R.image_stat_rgb(z[f"{name}.tgt"])
        scales, offsets = WR._opening_color_match_terms(rs, ts)
        assert scales == m["scales"] and offsets == m["offsets"], name
        assert hashlib.sha256(WR._opening_color_match_cube_text(scales, offsets).encode()).hexdigest() == m["cube_sha256"], name
        for k in (0, 3, 29, 1000):
            got = WR._opening_color_match_weight(k, 30.0, m["strength"], m["fade_seconds"])
            assert got == R.opening_match_weight(k, 30.0, m["strength"], m["fade_seconds"])


def test_statistics_call_runs(pkg):
    """ops._chunk_runs: frames per reference statistics call (an int = the node's batch_size with a ragged last call, or the explicit
    list of call sizes) -> runs of equally sized calls, one library call each."""
    from comfyui_vrgamedevgirl_amd import ops
    assert ops._chunk_runs(10, 4) == [(0, 10, 4)]                 # the library takes the ragged tail itself
    assert ops._chunk_runs(0, 3) == []
    assert ops._chunk_runs(5, [2, 2, 1]) == [(0, 4, 2), (4, 1, 1)]
    assert ops._chunk_runs(7, [3, 1, 1, 1, 1]) == [(0, 3, 3), (3, 4, 1)]
    assert ops._chunk_runs(6, [1, 2, 2, 1]) == [(0, 1, 1), (1, 4, 2), (5, 1, 1)]
    for bad in ([2, 2], [3, 0, 2], 0):
        with pytest.raises(ValueError):
            ops._chunk_runs(5, bad)


def test_colour_match_node_hands_whole_statistics_calls_to_every_piece(pkg, monkeypatch):
    """ColorMatchToReference.match_color: the pieces streamed through the GPU consist of whole batch_size calls, and a one-frame
    chunk broadcast against n_ref references becomes n_ref one-frame calls (control flow only: the ops are stubbed)."""
    from comfyui_vrgamedevgirl_amd import nodes, ops
    seen = []
    monkeypatch.setattr(nodes, "compute_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "reference_stats_async", lambda ref, *a, **k: (torch.zeros((ref.shape[0], 3, 2)), None))

    def fake_color_match(frames, _ref, k, ref_ms=None, cm_chunk=1, ref_event=None, **kw):
        seen.append((int(frames.shape[0]), cm_chunk))
        return frames

    monkeypatch.setattr(ops, "color_match", fake_color_match)

    def grouped(images, fn, multiple_of=1, fn_for_device=None, kind=None, fuse=None, stage_for_device=None):            # pieces of at most 2 * multiple_of frames
        step = 2 * multiple_of
        return torch.cat([fn(images[s:s + step], s) for s in range(0, images.shape[0], step)], dim=0)

    monkeypatch.setattr(nodes, "_run_grouped", grouped)
    node = nodes.ColorMatchToReference()
    x = torch.zeros((7, 4, 4, 3))
    node.match_color(x, torch.zeros((1, 4, 4, 3)), 1.0, 3)
    assert seen == [(6, 3), (1, 3)]                                          # int batch_size per piece; the last piece holds the remainder
    seen.clear()
    (out,) = node.match_color(x, torch.zeros((3, 4, 4, 3)), 1.0, 3)           # chunks 3, 3, 1 -> the single frame is matched to 3 references
    assert out.shape[0] == 9 and seen == [(6, [3, 3]), (3, [1, 1, 1])]
    seen.clear()
    (out,) = node.match_color(x[:2], torch.zeros((3, 4, 4, 3)), 1.0, 1)       # one-frame chunks: 3 calls of one frame each, per frame
    assert out.shape[0] == 6 and seen == [(6, [1] * 6)]


def test_device_copy_cache_under_inference_mode_and_alias_writes(pkg, monkeypatch):
    """ComfyUI runs every node under torch.inference_mode(): such tensors track no version counter (reading `_version` raises), so the
    cache of device copies validates them by its content stamp instead; a write through a numpy alias that the version counter cannot
    see drops the copy where it touches a sampled page; the weak-reference callback may run while the (re-entrant) lock is held; a
    failure inside the bookkeeping never reaches the node (ADVICE round 4, high + medium + low)."""
    import gc
    from comfyui_vrgamedevgirl_amd import _devices as D
    cpu = torch.device("cpu")
    c = D._DeviceCopies()
    monkeypatch.setattr(c, "_budget", lambda device: 1 << 30)
    monkeypatch.setattr(D, "DEVICE_CACHE_SECONDS", 0.0)            # no timer thread in this test
    with torch.inference_mode():
        t = torch.rand(8, 64, 64, 3)
        with pytest.raises(RuntimeError):
            t._version
        assert D._version_of(t) is None
        c.remember(t, cpu, [(0, 8, torch.empty(16), None)])
        assert c.errors == 0 and id(t) in c.entries
        assert c.lookup(t, cpu) is not None and c.hits == 1
        t.numpy()[0, 0, 0, 0] += 1.0                               # alias write: no version counter anywhere
        assert c.lookup(t, cpu) is None and id(t) not in c.entries
    u = torch.rand(4, 32, 32, 3)
    c.remember(u, cpu, [(0, 4, torch.empty(16), None)])
    u[3, 31, 31, 2] += 1.0                                          # ordinary tensor: the version counter sees every in-place op
    assert c.lookup(u, cpu) is None
    # sampled stamp: first and last page always covered
    big = torch.rand(64, 256, 256, 3)
    s0 = D._content_stamp(big)
    big.numpy()[-1, -1, -1, -1] += 1.0
    assert D._content_stamp(big) != s0
    # the weak-reference callback takes the lock remember() / lookup() hold: re-entrant
    v = torch.rand(2, 8, 8, 3)
    c.remember(v, cpu, [(0, 2, torch.empty(4), None)])
    key = id(v)
    with c.lock:
        del v
        gc.collect()
    assert key not in c.entries
    # expiry: copies older than DEVICE_CACHE_SECONDS are not handed out
    monkeypatch.setattr(D, "DEVICE_CACHE_SECONDS", 1e-9)
    monkeypatch.setattr(c, "_arm_timer", lambda: None)
    w = torch.rand(2, 8, 8, 3)
    c.remember(w, cpu, [(0, 2, torch.empty(4), None)])
    assert c.lookup(w, cpu) is None
    # a failing stamp never fails the caller
    monkeypatch.setattr(D, "_content_stamp", lambda t: (_ for _ in ()).throw(ValueError("boom")))
    c.remember(w, cpu, [(0, 2, torch.empty(4), None)])
    assert c.errors >= 1 and c.lookup(w, cpu) is None
    assert D.release_device_copies() >= 0


def test_product_sources_have_no_command_line_switches(pkg):
    """the A/B and ablation switches (among them VRG_MARCH_ABLATE: wrong pixels) are not build options of the
    product sources -- no `#ifndef VRG_*` knob is left in the kernels, and a -D of one of the old names stops the build."""
    import glob
    import shutil
    import subprocess
    from conftest import PKG_DIR, ROOT
    csrc = os.path.join(PKG_DIR, "csrc")
    knobs = 0
    for path in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")):
        with open(path) as fh:
            knobs += sum(1 for line in fh if line.startswith("#ifndef VRG_") and "VRG_HW_LOG2" not in line)
    assert knobs == 0
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    for macro in ("VRG_MARCH_ABLATE=1", "VRG_APPLY_FORCE_GENERAL", "VRG_TILE_H=16"):
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-D" + macro, "-fsyntax-only",
                            os.path.join(csrc, "vrg_api.hip")], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "not build options of the product sources" in r.stderr, macro


def test_lazy_frames_download_once_at_first_use(pkg, monkeypatch):
    """_devices.LazyFrames without a GPU (the download replaced by a host copy): shape questions do not download; any torch / numpy use
    downloads exactly once, on the calling thread, without re-entering itself (the cache's content stamp reads the tensor through torch);
    afterwards the object is an ordinary tensor known to the device-copy cache; a result dropped unread leaves the registry at once."""
    import gc
    import weakref
    from comfyui_vrgamedevgirl_amd import _devices as D
    monkeypatch.setattr(D, "LAZY_SECONDS", 0.0)                   # no timer thread here
    monkeypatch.setattr(D._DEVICE_COPIES, "_budget", lambda device: 1 << 30)
    truth = torch.arange(2 * 3 * 4 * 3, dtype=torch.float32).reshape(2, 3, 4, 3)
    calls = []

    def make():
        host = torch.zeros_like(truth)
        p = D._Pending(host, torch.device("cpu"), [(0, 2, truth, None)], truth.numel() * 4)
        monkeypatch.setattr(p, "_download", lambda p=p: (calls.append(1), p.host.copy_(p.pieces[0][2])))
        res = D.LazyFrames(host, p)
        p.owner = weakref.ref(res, lambda _r, pr=weakref.ref(p): D._LAZY.forget(pr()) if pr() is not None else None)
        D._LAZY.add(p, 1 << 30)
        return res, p

    t, p = make()
    assert isinstance(t, torch.Tensor) and t.shape == truth.shape and t.dtype == torch.float32 and t.device.type == "cpu" and len(t) == 2
    assert t.numel() == truth.numel() and t.is_contiguous() and t.stride() == truth.stride() and not calls and D.pending_of(t) is p
    assert torch.equal(t, truth) and len(calls) == 1 and D.pending_of(t) is None and p.done       # (first use: one download)
    assert torch.equal(t + 1, truth + 1) and len(calls) == 1
    assert id(t) in D._DEVICE_COPIES.entries and p not in D._LAZY.pending
    t.mul_(2)                                                                                       # an ordinary tensor now: in-place ops, version counter
    assert D._DEVICE_COPIES.lookup(t, torch.device("cpu")) is None
    for use in (lambda x: x.numpy(), lambda x: x[1], lambda x: list(x), lambda x: x.clone(), lambda x: x.to(torch.float16), lambda x: x.data_ptr(),
                lambda x: torch.cat([x, x]), lambda x: x.permute(0, 3, 1, 2), lambda x: repr(x), lambda x: x.sum().item(), lambda x: np.asarray(x)):
        n = len(calls)
        u, pu = make()
        use(u)
        assert len(calls) == n + 1 and pu.done and D.pending_of(u) is None
    u, pu = make()
    n_pending = len(D._LAZY.pending)
    assert pu in D._LAZY.pending
    del u
    gc.collect()
    assert pu not in D._LAZY.pending and len(D._LAZY.pending) == n_pending - 1 and not pu.done
    D._DEVICE_COPIES.clear()


def test_bench_issue_cost_roofline_and_clock_sampler_without_a_gpu(pkg):
    """bench.py's round-6 additions are host logic: the VALU roofline of a kernel's own instruction mix from the committed ISA price
    (profiles/r06_isa_cost_*.json) and a PMC record, and the clock sampler on a box without amdgpu hwmon files."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_bench_for_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(bench)
    finally:
        sys.argv = argv
    rec = {"valu_lane_instr": 687.3}
    r = bench.issue_cost_roofline("chain4_4k", "stats", rec, 70.0e9)
    assert r is not None and r["isa_profile"].endswith("r06_isa_cost_produce_lab.json")
    units = r["units_per_valu_instruction"]
    assert 3.0 < units < 3.7                                                      # pass 1: 44 % full-rate arithmetic, the rest 4.4 ... 8.4 cycles
    assert abs(r["issue_bound_Mpix_s"] - 1024 * 64 * 2.4e9 / (687.3 * units) / 1e6) < 20.0        # (units is printed rounded to 3 places)
    assert abs(r["frac"] - 70.0e9 / (r["issue_bound_Mpix_s"] * 1e6)) < 1e-3 and 0.9 < r["frac"] < 1.15
    assert abs(sum(r["by_class_share"].values()) - 1.0) < 0.02
    assert bench.issue_cost_roofline("grain_lut_1080p", "apply", rec, 1e9) is None      # no ISA price committed for that kernel
    assert bench.issue_cost_roofline("chain4_4k", "stats", {}, 1e9) is None
    with bench.ClockSampler() as cs:
        pass
    assert cs.summary() is None or "sclk_mhz_median" in cs.summary()


def test_bench_dump_outputs_and_step_counts_without_a_gpu(pkg, tmp_path):
    """bench.py --dump-outputs writes float32 .npy files whose sample indices depend on the batch size only (equal runs, equal files), within
    64 MB at the headline's 4K x 256 frames; --steps below 1 and a negative --warmup are refused."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_bench_for_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(bench)
        assert (bench.DUMP_SAMPLE + 2 * bench.DUMP_ROWS * 3840 * 3) * 4 <= 64 << 20
        bench.DUMP_SAMPLE = 1000                  # (this test's own copy of the module) the sampled form on a small batch
        out = torch.rand(3, 70, 40, 3, generator=torch.Generator().manual_seed(1))
        dumps = []
        for d in ("a", "b"):
            bench.dump_outputs(out, str(tmp_path / d))
            dumps.append({n: np.load(tmp_path / d / f"{n}.npy") for n in ("output_sample", "output_first_rows", "output_last_rows")})
        for n, a in dumps[0].items():
            assert a.dtype == np.float32 and np.array_equal(a, dumps[1][n]), n
        assert np.array_equal(dumps[0]["output_first_rows"], out[0, :bench.DUMP_ROWS].numpy())
        assert np.array_equal(dumps[0]["output_last_rows"], out[-1, -bench.DUMP_ROWS:].numpy())
        assert dumps[0]["output_sample"].shape == (1000,) and np.isin(dumps[0]["output_sample"], out.numpy()).all()
        sys.argv = ["bench.py", "--steps", "7", "--warmup", "0"]
        args = bench.parse_args()
        assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 0, False, None)
        for bad in (["--steps", "0"], ["--warmup", "-1"]):
            sys.argv = ["bench.py", *bad]
            with pytest.raises(SystemExit):
                bench.parse_args()
    finally:
        sys.argv = argv

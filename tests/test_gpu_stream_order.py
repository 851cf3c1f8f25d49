"""Every operator under a stream that is not the default one (tests/stream_support.py): launches on the caller's stream, results that
cross streams through _devices, cold and evicted table caches under two streams."""
import sys
import threading
import types

import numpy as np
import pytest
import torch

import stream_support as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def spin(ops):
    s = S.Spin()
    print(f"\n[stream order] {torch.cuda.get_device_name(0)}: {s}")
    return s


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_launches_go_to_the_callers_stream(ops, dev, spin, case):
    inputs, call = case.build(ops, dev)
    torch.cuda.synchronize()
    r = S.probe(ops, case, inputs, call, spin)
    print(f"\n[stream order] {case.name}: host {r['host_ms']:.3f} ms, spins {r['early_ms']:.1f} / {r['late_ms']:.1f} ms, "
          f"armed early {r['armed_early']} late {r['armed_late']}")
    assert r["armed_late"], f"{case.name}: the spin on the default stream had ended when the call returned (host {r['host_ms']:.3f} ms)"
    if case.name not in S.HOST_SYNCING:
        assert r["armed_early"], f"{case.name}: the call waited for the caller's stream on the host and is not listed in HOST_SYNCING"
    assert r["outputs"] and all(r["outputs"]), f"{case.name}: outputs differ from the default-stream run: {r['outputs']}"
    assert all(r["inputs_kept"]), f"{case.name}: an input was written"


# ---- a result crosses streams through _devices --------------------------------------------------------------------------------------------------

def _device_graph(monkeypatch, dev):
    from comfyui_vrgamedevgirl_amd import _devices as D
    mm = types.ModuleType("comfy.model_management")
    mm.get_torch_device = lambda: dev
    mm.intermediate_device = lambda: dev
    comfy = types.ModuleType("comfy")
    comfy.model_management = mm
    monkeypatch.setitem(sys.modules, "comfy", comfy)
    monkeypatch.setitem(sys.modules, "comfy.model_management", mm)
    monkeypatch.setattr(D, "LAZY_SECONDS", 60.0)
    monkeypatch.setattr(D, "LAZY_DOWNLOAD", True)
    return D, mm


def _in_thread(fn):
    box = []

    def body():
        try:
            box.append(("ok", fn()))
        except BaseException as exc:             # reported by the caller
            box.append(("error", exc))
    th = threading.Thread(target=body)
    th.start()
    th.join()
    assert box and box[0][0] == "ok", box
    return box[0][1]


@pytest.mark.parametrize("consumer", ["materialise", "on_device"])
def test_a_device_result_whose_recipe_ran_on_another_threads_stream(pkg, ops, dev, spin, monkeypatch, consumer):
    """The recipe of a deferred device-resident result runs from a second host thread under that thread's stream, behind a spin; the main
    thread then uses the result under a stream of its own.  It has to wait for the recipe's event."""
    from comfyui_vrgamedevgirl_amd import nodes
    D, _mm = _device_graph(monkeypatch, dev)
    x = S._rand((4, 72, 128, 3), 90).to(dev)
    monkeypatch.setattr(D, "DEFER_GRAPH", False)
    want = nodes.FastUnsharpSharpen().apply_unsharp(x, 0.6, False)[0].clone()
    torch.cuda.synchronize()
    monkeypatch.setattr(D, "DEFER_GRAPH", True)
    got = nodes.FastUnsharpSharpen().apply_unsharp(x, 0.6, False)[0]
    pending = D.pending_of(got)
    assert got.is_cuda and pending is not None and pending.recipe is not None
    t, s = spin.streams(2)                  # streams that run beside one another: on one hardware queue nothing could go wrong
    late = torch.cuda.Event()

    def run_recipe():
        torch.cuda.set_device(dev)
        with torch.cuda.stream(t):
            spin.queue(0.05)
            pieces = pending.device_pieces()
            late.record()
        return pieces
    assert _in_thread(run_recipe)
    with torch.cuda.stream(s):
        plain = D.materialise(got) if consumer == "materialise" else D.on_device(got, dev)
        seen = plain * 1.0
        armed = not late.query()
    s.synchronize()
    torch.cuda.synchronize()
    assert armed, "the recipe had finished before the consumer was queued: nothing was tested"
    assert S.same_bits(seen, want)


def test_a_host_result_whose_recipe_ran_on_another_threads_stream(pkg, ops, dev, spin, monkeypatch):
    """device frames in, host frames out: the recipe runs on the second thread's stream behind a spin, the download is triggered from the
    main thread under another stream"""
    from comfyui_vrgamedevgirl_amd import nodes
    D, mm = _device_graph(monkeypatch, dev)
    mm.intermediate_device = lambda: torch.device("cpu")
    x = S._rand((4, 72, 128, 3), 91).to(dev)
    monkeypatch.setattr(D, "DEFER_GRAPH", False)
    want = nodes.FastUnsharpSharpen().apply_unsharp(x, 0.6, False)[0].clone()
    torch.cuda.synchronize()
    monkeypatch.setattr(D, "DEFER_GRAPH", True)
    got = nodes.FastUnsharpSharpen().apply_unsharp(x, 0.6, False)[0]
    pending = D.pending_of(got)
    assert got.device.type == "cpu" and pending is not None and pending.recipe is not None
    t, s = spin.streams(2)                  # streams that run beside one another: on one hardware queue nothing could go wrong
    late = torch.cuda.Event()

    def run_recipe():
        torch.cuda.set_device(dev)
        with torch.cuda.stream(t):
            spin.queue(0.05)
            pieces = pending.device_pieces()
            late.record()
        return pieces
    try:
        assert _in_thread(run_recipe)
        with torch.cuda.stream(s):
            armed = not late.query()
            seen = (got * 1.0).clone()
        torch.cuda.synchronize()
        assert armed, "the recipe had finished before the download was triggered: nothing was tested"
        assert S.same_bits(seen, want.cpu() if want.is_cuda else want)
    finally:
        torch.cuda.synchronize()
        D._DEVICE_COPIES.clear()             # the download remembers a device copy: not for later tests, whatever happened here


# ---- table caches under two streams ---------------------------------------------------------------------------------------------------------------

def test_two_host_threads_two_streams_one_cold_cache(ops, dev):
    x = S._bytes((2, 54, 96, 3), 92).to(dev)
    f = S._rand((3, 70, 90, 3), 93).to(dev)
    g = [S._rand((2, 40, 64, 3), 94).to(dev)]
    want = (ops.resize_frames_u8(x, 192, 108), ops.cut_thumbnails(f), ops.video_grid(g, 32, 24, 1))
    torch.cuda.synchronize()
    S._forget_tables(ops)
    barrier = threading.Barrier(2)
    results, errors = {}, []

    def worker(k):
        try:
            torch.cuda.set_device(dev)
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                barrier.wait(timeout=30)
                results[k] = (ops.resize_frames_u8(x, 192, 108), ops.cut_thumbnails(f), ops.video_grid(g, 32, 24, 1))
            st.synchronize()
        except BaseException as exc:
            errors.append(exc)
    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for k in range(2):
        assert all(S.same_bits(a, b) for a, b in zip(results[k], want)), k


def test_a_table_evicted_under_another_stream_outlives_its_reader(ops, dev, spin):
    """Table K is uploaded under stream b, then read by a launch queued on stream a behind a spin; meanwhile calls under b overflow the
    cache, which drops K, and b allocates blocks of K's size and fills them with ANOTHER valid table (of a smaller source: every tap it
    names lies inside the frames).  a's launch must still read K."""
    x = S._bytes((2, 54, 96, 3), 95).to(dev)
    want = ops.resize_frames_u8(x, 192, 108)
    torch.cuda.synchronize()
    other = torch.from_numpy(ops.lanczos4_taps(27, 48, 108, 192).view(np.uint8).copy()).to(dev)         # same size, smaller source
    a, b = spin.streams(2)
    ops._lanczos_tables.clear()
    with torch.cuda.stream(b):
        ops.resize_frames_u8(x, 192, 108)                  # K is made here: its block belongs to b's pool
    b.synchronize()
    (key,) = ops._lanczos_tables
    table = ops._lanczos_tables.pop(key)
    assert table.numel() == other.numel()
    for i in range(62):
        ops._lanczos_tables[("filler", i)] = torch.empty(1, dtype=torch.uint8, device=dev)
    ops._lanczos_tables[key] = table                       # 63 entries, K among them
    del table
    late = torch.cuda.Event()
    with torch.cuda.stream(a):
        spin.queue(0.05)
        got = ops.resize_frames_u8(x, 192, 108)
        late.record()
    with torch.cuda.stream(b):
        small = S._bytes((1, 9, 9, 3), 96).to(dev)
        ops.resize_frames_u8(small, 10, 10)                # the 64th entry
        ops.resize_frames_u8(small, 11, 11)                # clears the cache: K is dropped
        assert key not in ops._lanczos_tables
        blocks = [torch.empty_like(other) for _ in range(64)]
        for blk in blocks:
            blk.copy_(other)
        armed = not late.query()
    a.synchronize()
    torch.cuda.synchronize()
    ops._lanczos_tables.clear()
    assert armed, "stream a had finished before the table was dropped: nothing was tested"
    assert S.same_bits(got, want)

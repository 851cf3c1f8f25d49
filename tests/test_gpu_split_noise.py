"""Split noise on the GPU: an RNG chunk of more than rng.MAX_CHUNK_NUMEL elements (one torch.randn that ATen runs as several kernels over
"leaves") drawn in registers by the fused kernels -- no noise buffer, any piece of whole frames, inside the fused chain.  The limit is
lowered for every test, so a few MB stand for the 2 GB of the real thing (which tests/test_gpu_parity.py compares against ATen's own split
at 91 x 1080p).

Shape A: 3 frames of 541 x 959 x 3 = 4,669,371 elements under a limit of 3,000,000: two leaves of 2,334,685 and 2,334,686 elements, the
boundary at element 778,228 of frame 1, inside a pixel (778228 % 3 == 1); each leaf is larger than 4 G = 2,097,152, so the second Philox
round is used with the saturated G = 524,288.  Shape B: the same frames under 1,200,000: four leaves.  Smallest: 2 frames of 5 x 7 x 3 under
60: G unsaturated, each frame meets two leaves, a 3 x 3 stencil crosses a leaf boundary in both directions."""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

A_SHAPE, A_LIMIT, B_LIMIT = (3, 541, 959, 3), 3_000_000, 1_200_000
S_SHAPE, S_LIMIT = (2, 5, 7, 3), 60
CASES = [pytest.param(A_SHAPE, A_LIMIT, id="A"), pytest.param(A_SHAPE, B_LIMIT, id="B"), pytest.param(S_SHAPE, S_LIMIT, id="smallest")]
I, SAT = 0.07, 0.4
SEED = 1234


class _Generator:
    """seed and Philox offset of a generator, for reserving on the host what the device generator would hand out (rng.py uses these
    three methods)"""

    def __init__(self, seed, offset=0):
        self.seed, self.offset = seed, offset

    def initial_seed(self):
        return self.seed

    def get_offset(self):
        return self.offset

    def set_offset(self, v):
        self.offset = v


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def mods(pkg):
    from comfyui_vrgamedevgirl_amd import ops, rng
    return ops, rng


@functools.lru_cache(maxsize=None)
def _frames(shape, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g)


def _plans(ops, rng, shape, dev, chunk_frames=0, seed=SEED):
    """the whole batch reserved on the host from (seed, offset 0) with this device's geometry, and the generator afterwards"""
    gen = _Generator(seed)
    fe = shape[1] * shape[2] * 3
    return ops.plan_noise(shape[0], fe, chunk_frames, dev, gen, geom=rng.device_geometry(dev)), gen


def _torch_noise(plans, shape, dev, seed=SEED):
    """torch's own values: for every leaf a generator set to the leaf's offset draws torch.randn(size) -- torch picks G from `size` itself"""
    main = plans[0]
    parts = []
    for start, size, _G, off in main.stream.leaves:
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        g.set_offset(off)
        parts.append(torch.randn(size, device=dev, generator=g))
    return torch.cat(parts).reshape(shape)


def test_shape_a_is_the_shape_described(mods, dev, monkeypatch):
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", A_LIMIT)
    plans, _ = _plans(ops, rng, A_SHAPE, dev)
    leaves = plans[0].stream.leaves
    assert [(s, n) for s, n, _G, _o in leaves] == [(0, 2334685), (2334685, 2334686)]
    fe = 541 * 959 * 3
    assert leaves[1][0] - fe == 778228 and 778228 % 3 == 1
    assert all(G == 524288 and n > 4 * G for _s, n, G, _o in leaves)
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", B_LIMIT)
    assert len(_plans(ops, rng, A_SHAPE, dev)[0][0].stream.leaves) == 4
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", S_LIMIT)
    small = _plans(ops, rng, S_SHAPE, dev)[0][0].stream
    assert all(G < 524288 for _s, _n, G, _o in small.leaves)
    assert all(len(small.leaves_of(0, f * 105, (f + 1) * 105)) == 2 for f in range(2))


@pytest.mark.parametrize("shape,limit", CASES)
def test_the_noise_is_torchs_own(mods, dev, monkeypatch, shape, limit):
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", limit)
    x = _frames(shape).to(dev)
    plans, after = _plans(ops, rng, shape, dev)
    want = ops.film_grain_injected(x, _torch_noise(plans, shape, dev), I, SAT)
    torch.manual_seed(SEED)
    gen = torch.cuda.default_generators[dev.index]
    assert gen.get_offset() == 0
    got = ops.film_grain(x, I, SAT, chunk_frames=0)
    assert torch.equal(got, want)
    assert gen.get_offset() == after.get_offset()               # the generator moved as the host predicted: outer reservation + leaves
    assert not torch.equal(got, x)
    assert torch.equal(ops.film_grain(x, I, SAT, plans=plans), want)


RANGES = [[(0, 1), (1, 3)], [(0, 2), (2, 3)], [(0, 1), (1, 2), (2, 3)]]


@pytest.mark.parametrize("shape,limit", CASES)
def test_pieces_equal_the_whole_call(mods, dev, monkeypatch, shape, limit):
    """film_grain and fused_chain (grain -> unsharp, fp32 and uint8) over frame ranges that cut through a leaf, in and out of order"""
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", limit)
    x = _frames(shape).to(dev)
    xb = (_frames(shape) * 255).to(torch.uint8).to(dev)
    F = shape[0]
    plans, _ = _plans(ops, rng, shape, dev)
    spec = ops.ChainSpec(grain=(I, SAT, 0), sharpen=("unsharp", 0.6, False))
    whole = {"grain": ops.film_grain(x, I, SAT, plans=plans), "chain": ops.fused_chain(x, spec, plans=plans),
             "bytes": ops.fused_chain(xb, spec, plans=plans)}
    for ranges in RANGES:
        ranges = [(a, min(b, F)) for a, b in ranges if a < F]
        got = {k: [None] * len(ranges) for k in whole}
        for i in reversed(range(len(ranges))):                  # last piece first: a piece depends on nothing but its plan
            a, b = ranges[i]
            sub = ops.slice_plans(plans, a, b - a)
            got["grain"][i] = ops.film_grain(x[a:b], I, SAT, plans=sub)
            got["chain"][i] = ops.fused_chain(x[a:b], spec, plans=sub)
            got["bytes"][i] = ops.fused_chain(xb[a:b], spec, plans=sub)
        for k in whole:
            assert torch.equal(torch.cat(got[k]), whole[k]), (k, ranges)


@functools.lru_cache(maxsize=None)
def _lut17(device_index):
    from comfyui_vrgamedevgirl_amd import VRGDG_IV_Adjustments as iv, cube, ops
    return ops.upload_lut(cube.parse_cube_file(os.path.join(iv.LUTS_DIR, "AMD_Identity_17.cube")), torch.device("cuda", device_index))


@pytest.mark.parametrize("shape,limit", CASES)
def test_chains_equal_the_operators_in_order(mods, dev, monkeypatch, shape, limit):
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", limit)
    x = _frames(shape).to(dev)
    lut = _lut17(dev.index)
    plans, _ = _plans(ops, rng, shape, dev)
    grained = ops.film_grain(x, I, SAT, plans=plans)
    lutted = ops.lut3d(grained, lut, 10.0)
    grain = (I, SAT, 0)
    for zero in (False, True):                                  # grain -> LUT 17^3 -> unsharp, both borders
        got = ops.fused_chain(x, ops.ChainSpec(grain=grain, lut=(lut, 10.0), sharpen=("unsharp", 0.6, zero)), plans=plans)
        assert torch.equal(got, ops.stencil3x3(lutted, "unsharp", 0.6, zero)), zero
    got = ops.fused_chain(x, ops.ChainSpec(grain=grain, sharpen=("laplacian", 0.5, False)), plans=plans)
    assert torch.equal(got, ops.stencil3x3(grained, "laplacian", 0.5, False))
    assert torch.equal(ops.fused_chain(x, ops.ChainSpec(grain=grain, lut=(lut, 10.0)), plans=plans), lutted)
    assert torch.equal(ops.fused_chain(x, ops.ChainSpec(grain=grain), plans=plans), grained)
    # uint8 grain -> LUT: the byte kernels equal convert -> fp32 operators -> convert
    xb = (_frames(shape) * 255).to(torch.uint8).to(dev)
    want = ops.f32_to_frames_u8(ops.lut3d(ops.film_grain(ops.frames_u8_to_f32(xb), I, SAT, plans=plans), lut, 10.0))
    assert torch.equal(ops.fused_chain(xb, ops.ChainSpec(grain=grain, lut=(lut, 10.0)), plans=plans), want)
    # the generator route gives the same as the plans
    torch.manual_seed(SEED)
    assert torch.equal(ops.fused_chain(x, ops.ChainSpec(grain=grain, lut=(lut, 10.0))), lutted)


@pytest.mark.parametrize("cm_stats", ["fp64", "device"])
@pytest.mark.parametrize("shape,limit", CASES)
def test_chain_with_colour_match(mods, dev, monkeypatch, shape, limit, cm_stats):
    """grain -> LUT -> colour match -> unsharp: pass 1 draws the split noise, pass 2 starts from its Lab image"""
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", limit)
    x = _frames(shape).to(dev)
    ref = _frames((1, 30, 40, 3), 9).to(dev)
    lut = _lut17(dev.index)
    plans, _ = _plans(ops, rng, shape, dev)
    ref_ms = ops.reference_stats(ref, cm_stats=cm_stats)
    y = ops.lut3d(ops.film_grain(x, I, SAT, plans=plans), lut, 10.0)
    y = ops.color_match(y, None, 0.9, ref_ms=ref_ms, cm_chunk=2, cm_stats=cm_stats)
    want = ops.stencil3x3(y, "unsharp", 0.6, False)
    spec = ops.ChainSpec(grain=(I, SAT, 0), lut=(lut, 10.0), colormatch=(ref_ms, 0.9), sharpen=("unsharp", 0.6, False), cm_stats=cm_stats, cm_chunk=2)
    got = ops.fused_chain(x, spec, plans=plans)
    assert torch.equal(got, want)
    assert torch.equal(ops.fused_chain(x, spec, plans=plans, cache_lab=False), want)       # (the recomputing form is not taken for split noise: same bits)
    # the statistics pass on its own, whole and in pieces
    st = ops.chain_stats(x, spec, plans=plans)
    parts = torch.cat([ops.chain_stats(x[a:b], spec, plans=ops.slice_plans(plans, a, b - a)) for a, b in ((0, 1), (1, shape[0]))])
    assert torch.equal(st, parts)


def test_split_launches_past_32768_frames(mods, dev, monkeypatch):
    """32771 frames of 2 x 2 (393,252 elements, four leaves under a limit of 100,000) in ONE record: the point-wise route and the
    statistics pass cut the call at frame 32768 (blockIdx.y) and move the table's starts with the second launch.  Against torch's noise,
    and against the same call in two pieces cut at another frame."""
    ops, rng = mods
    shape = (32771, 2, 2, 3)
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", 100_000)
    x = _frames(shape).to(dev)
    plans, _ = _plans(ops, rng, shape, dev)
    assert len(plans[0].stream.leaves) == 4 and len(ops.split_launches(plans[0], 12)) == 1
    want = ops.film_grain_injected(x, _torch_noise(plans, shape, dev), I, SAT)
    assert not torch.equal(want[32768:], want[:3])
    assert torch.equal(ops.film_grain(x, I, SAT, plans=plans), want)
    lut = _lut17(dev.index)
    spec = ops.ChainSpec(grain=(I, SAT, 0), lut=(lut, 10.0))
    assert torch.equal(ops.fused_chain(x, spec, plans=plans), ops.lut3d(want, lut, 10.0))
    cut = 32766
    lab = torch.empty_like(x)
    st = ops.chain_stats(x, spec, plans=plans, lab_out=lab)
    lab2 = torch.empty_like(x)
    parts = torch.cat([ops.chain_stats(x[a:b], spec, plans=ops.slice_plans(plans, a, b - a), lab_out=lab2[a:b]) for a, b in ((0, cut), (cut, shape[0]))])
    assert torch.equal(st, parts) and torch.equal(lab, lab2)
    assert torch.equal(st, ops.chain_stats(ops.film_grain(x, I, SAT, plans=plans), ops.ChainSpec(lut=(lut, 10.0))))


def test_a_frame_of_more_than_eight_leaves_still_gets_torchs_noise(mods, dev, monkeypatch):
    """2 frames of 5 x 7 x 3 under a limit of 11: every frame meets more than eight leaves and takes the materialising branch, alone and
    inside a chain"""
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", 11)
    x = _frames(S_SHAPE).to(dev)
    plans, after = _plans(ops, rng, S_SHAPE, dev)
    assert ops._split_records(plans[0], 105) is None
    want = ops.film_grain_injected(x, _torch_noise(plans, S_SHAPE, dev), I, SAT)
    torch.manual_seed(SEED)
    assert torch.equal(ops.film_grain(x, I, SAT, chunk_frames=0), want)
    assert torch.cuda.default_generators[dev.index].get_offset() == after.get_offset()
    assert torch.equal(torch.cat([ops.film_grain(x[i:i + 1], I, SAT, plans=ops.slice_plans(plans, i, 1)) for i in (0, 1)]), want)
    got = ops.fused_chain(x, ops.ChainSpec(grain=(I, SAT, 0), sharpen=("unsharp", 0.6, True)), plans=plans)
    assert torch.equal(got, ops.stencil3x3(want, "unsharp", 0.6, True))


def test_no_noise_buffer(mods, dev, monkeypatch):
    """film_grain(..., out=preallocated) under shape A allocates less than the chunk's bytes (it used to allocate exactly the chunk's noise)"""
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", A_LIMIT)
    x = _frames(A_SHAPE).to(dev)
    out = torch.empty_like(x)
    torch.manual_seed(SEED)
    ops.film_grain(x[:1], I, SAT, chunk_frames=0, out=out[:1])          # library loaded, geometry cached
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.max_memory_allocated(dev)
    ops.film_grain(x, I, SAT, chunk_frames=0, out=out)
    torch.cuda.synchronize(dev)
    rise = torch.cuda.max_memory_allocated(dev) - before
    print(f"film_grain, shape A, out= given: peak allocation rose by {rise} bytes (the chunk is {x.numel() * 4})")
    assert rise < x.numel() * 4


def _node_settings(monkeypatch, D, defer):
    monkeypatch.setattr(D, "LAZY_SECONDS", 60.0)
    monkeypatch.setattr(D, "DEFER_GRAPH", defer)
    monkeypatch.setattr(D, "LAZY_DOWNLOAD", defer)
    D._DEVICE_COPIES.clear()


#: the nodes' batch: 5 frames of 25 x 41 x 3 = 15,375 elements under a limit of 4,000: leaves of 3,843 / 3,844 / 3,844 / 3,844, their
#: boundaries inside frames 1, 2 and 3 (elements 768, 1,537 and 2,306 of them: on a pixel, one and two elements into a pixel)
N_SHAPE, N_LIMIT = (5, 25, 41, 3), 4000


def test_node_streams_a_long_batch_in_pieces(mods, dev, monkeypatch):
    """FastFilmGrain(batch_size 0) on host frames beyond the (lowered) limit: several bounded pieces, the bits and the generator of the
    device-resident call"""
    ops, rng = mods
    from comfyui_vrgamedevgirl_amd import nodes, _devices as D
    shape = N_SHAPE
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", N_LIMIT)
    x = _frames(shape)
    fe = x[0].numel()
    plans, _ = _plans(ops, rng, shape, dev)
    assert [(s // fe, s % fe) for s, _n, _G, _o in plans[0].stream.leaves[1:]] == [(1, 768), (2, 1537), (3, 2306)]
    torch.manual_seed(SEED)
    want = ops.film_grain(x.to(dev), I, SAT, chunk_frames=0).cpu()
    state = torch.cuda.get_rng_state(dev)
    _node_settings(monkeypatch, D, defer=False)
    monkeypatch.setattr(D, "PIPE_BYTES", 2 * fe * 4)
    monkeypatch.setattr(D, "STAGE_BYTES", 2 * fe * 4)
    pieces = []
    real = ops.film_grain
    monkeypatch.setattr(ops, "film_grain", lambda images, *a, **k: (pieces.append(int(images.shape[0])), real(images, *a, **k))[1])
    torch.manual_seed(SEED)
    got = nodes.FastFilmGrain().apply_grain(x, I, SAT, 0)[0]
    assert torch.equal(torch.as_tensor(got).cpu(), want)
    assert len(pieces) > 1 and sum(pieces) == shape[0] and max(pieces) <= 2, pieces
    assert torch.equal(torch.cuda.get_rng_state(dev), state)
    D._DEVICE_COPIES.clear()


def test_node_fuses_with_the_node_behind_it(mods, dev, monkeypatch):
    """FastFilmGrain(batch_size 0) -> FastUnsharpSharpen on a long batch: deferred, ONE fused launch of both stages (counted the way
    tests/test_deferred_graph.py counts), the bits and the generator state of the two eager nodes"""
    ops, rng = mods
    from comfyui_vrgamedevgirl_amd import nodes, _devices as D
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", N_LIMIT)
    x = _frames(N_SHAPE)
    ops.toolchain_selfcheck(dev)                 # (its probes launch fused chains themselves: before the count)
    calls = []
    real_chain, real_grain, real_stencil = ops.fused_chain, ops.film_grain, ops.stencil3x3

    def fused_chain(images, spec, *a, **k):
        calls.append(("fused_chain", sum(v is not None for v in (spec.grain, spec.lut, spec.colormatch, spec.sharpen))))
        return real_chain(images, spec, *a, **k)

    monkeypatch.setattr(ops, "fused_chain", fused_chain)
    monkeypatch.setattr(ops, "film_grain", lambda *a, **k: (calls.append(("film_grain", 1)), real_grain(*a, **k))[1])
    monkeypatch.setattr(ops, "stencil3x3", lambda *a, **k: (calls.append(("stencil3x3", 1)), real_stencil(*a, **k))[1])

    def graph():
        g = nodes.FastFilmGrain().apply_grain(x, I, SAT, 0)[0]
        return g, nodes.FastUnsharpSharpen().apply_unsharp(g, 0.6, False)[0]

    _node_settings(monkeypatch, D, defer=False)
    torch.manual_seed(SEED)
    want = [w.clone() for w in graph()]
    state = torch.cuda.get_rng_state(dev)
    assert calls and all(n == 1 for _name, n in calls)          # two nodes, single-stage launches
    _node_settings(monkeypatch, D, defer=True)
    calls.clear()
    torch.manual_seed(SEED)
    got = graph()
    assert torch.equal(torch.cuda.get_rng_state(dev), state)    # the grain node reserved its noise when it was called
    assert not calls                                            # nothing has run
    assert torch.equal(got[1], want[1])
    assert calls == [("fused_chain", 2)]                        # one launch of both stages, nothing else
    assert torch.equal(got[0], want[0])
    D._DEVICE_COPIES.clear()

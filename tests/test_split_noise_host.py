"""Split noise on the host: RNG chunks of more than rng.MAX_CHUNK_NUMEL elements, which torch draws as several kernels over "leaves"
(rng.split_32bit / rng.reserve_split).  ops.plan_noise reserves them as ATen does, ops.slice_plans cuts them at any frame,
ops.split_launches groups frames into launches of at most eight leaves, and the kernels' leaf lookup (csrc/vrg_common.hpp) is checked
against a bisect by a stand-alone program.  No GPU is needed: the limit is lowered, the geometry and the generator are passed in."""
import bisect
import os
import random
import subprocess

import pytest
import torch

from conftest import PKG_DIR, ROOT

HOST_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse"]
HOST_SOURCE = os.path.join(ROOT, "tests", "host_math", "split_noise_check.cpp")


@pytest.fixture()
def mods(pkg):
    from comfyui_vrgamedevgirl_amd import ops, rng
    return ops, rng


def _geom(rng):
    return rng.DeviceGeometry(cu_count=256, max_threads_per_cu=2048)      # an MI355X: 2048 blocks of 256, G saturates at 524,288


class _Generator:
    """The three methods rng.py uses of a device generator.  (torch's CPU generator keeps no Philox offset -- set_offset raises "CPU
    Generator does not use offset" -- so the host tests carry seed and offset in this stand-in, as tests/test_deferred_graph.py does.)"""

    def __init__(self, seed, offset):
        self.seed, self.offset = seed, offset

    def initial_seed(self):
        return self.seed

    def get_offset(self):
        return self.offset

    def set_offset(self, v):
        self.offset = v


def _gen(seed=77, offset=40):
    return _Generator(seed, offset)


#: (frames, frame elements, chunk_frames, limit): several full oversize chunks + an oversize tail, + a small tail, one draw for all,
#: a limit that makes a chunk many leaves, a chunk exactly at the limit (not split) and one element above it
SHAPES = [(11, 3 * 35, 4, 300), (9, 3 * 35, 4, 300), (10, 3 * 35, 4, 300), (7, 3 * 1000, 0, 5000), (3, 541 * 959 * 3, 0, 3_000_000), (3, 541 * 959 * 3, 0, 1_200_000),
          (2, 105, 0, 60), (6, 100, 3, 300), (6, 100, 3, 299), (5, 3 * 7, 2, 11)]
SPLIT_SHAPES = [s for s in SHAPES if min(s[2] or s[0], s[0]) * s[1] > s[3]]          # (all but the chunk of exactly `limit` elements)


def _reference_loop(rng, frames, fe, chunk_frames, geom, gen):
    """the generator as the chunk loop of ops._film_grain_oversize moved it before split plans existed: per chunk reserve_split, or
    reserve for a chunk at or below the limit; returns the element parameters (start, size, G, off) of every chunk"""
    step = min(chunk_frames if chunk_frames > 0 else frames, frames)
    chunks = []
    for f0 in range(0, frames, step):
        numel = min(step, frames - f0) * fe
        if numel > rng.MAX_CHUNK_NUMEL:
            chunks.append(rng.reserve_split(numel, None, gen, geom).leaves)
        else:
            st = rng.reserve(numel, 1, None, gen, geom)
            chunks.append([(0, numel, st.grid_threads, st.offset0)])
    return chunks


def _leaf_at(leaves, e):
    i = bisect.bisect_right([l[0] for l in leaves], e) - 1
    start, size, G, off = leaves[i]
    assert start <= e < start + size
    return (e - start, size, G, off)


def _plan_params(ops, rng, plans, fe, frame, elems):
    """(element inside its leaf, leaf size, G, offset) of elements `elems` of frame `frame` of `plans`, through the launches a kernel sees"""
    out = []
    for f0, nf, plan in ops._plan_segments(plans, _frames_of(ops, plans), "test"):
        if not f0 <= frame < f0 + nf:
            continue
        if isinstance(plan, ops.SplitNoisePlan):
            for g0, n, _seed, leaves in ops.split_launches(plan, fe):
                if g0 <= frame - f0 < g0 + n:
                    assert leaves is not None
                    return [_leaf_at(leaves, (frame - f0 - g0) * fe + e) for e in elems]
        else:
            s = plan.stream
            chunk, fl = divmod(frame - f0, plan.chunk_frames)
            off = s.offset0 + (plan.chunk0 + chunk) * s.offset_stride
            return [(fl * fe + e, s.chunk_numel, s.grid_threads, off) for e in elems]
    raise AssertionError("frame outside the plans")


def _frames_of(ops, plans):
    main, tail, n_full = plans
    return sum(ops._plan_frames(p, n) for p, n in ((main, n_full), (tail, 1)) if p is not None)


@pytest.mark.parametrize("frames,fe,chunk_frames,limit", SHAPES)
def test_plan_noise_moves_the_generator_as_the_chunk_loop_does(mods, monkeypatch, frames, fe, chunk_frames, limit):
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", limit)
    geom = _geom(rng)
    a, b = _gen(), _gen()
    want = _reference_loop(rng, frames, fe, chunk_frames, geom, a)
    plans = ops.plan_noise(frames, fe, chunk_frames, torch.device("cpu"), b, geom=geom)
    assert b.get_offset() == a.get_offset() and b.initial_seed() == a.initial_seed()
    step = min(chunk_frames if chunk_frames > 0 else frames, frames)
    main, tail, n_full = plans
    assert n_full == frames // step and _frames_of(ops, plans) == frames
    assert isinstance(main, ops.SplitNoisePlan) == (step * fe > limit)
    if frames % step:
        assert isinstance(tail, ops.SplitNoisePlan) == ((frames % step) * fe > limit)
    # every chunk's leaves are the loop's: same starts, sizes, grids and offsets
    for c, leaves in enumerate(want):
        plan = main if c < n_full else tail
        if isinstance(plan, ops.SplitNoisePlan):
            numel = plan.chunk_frames * fe
            assert plan.stream.leaves_of(c if c < n_full else 0, 0, numel) == leaves


@pytest.mark.parametrize("frames,fe,chunk_frames,limit", SHAPES)
def test_leaves_cover_every_chunk_exactly_and_in_order(mods, monkeypatch, frames, fe, chunk_frames, limit):
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", limit)
    plans = ops.plan_noise(frames, fe, chunk_frames, torch.device("cpu"), _gen(), geom=_geom(rng))
    for plan in plans[:2]:
        if not isinstance(plan, ops.SplitNoisePlan):
            continue
        numel = plan.chunk_frames * fe
        for chunk in range(plan.frames // plan.chunk_frames):
            leaves = plan.stream.leaves_of(chunk, 0, numel)
            at = 0
            for start, size, G, off in leaves:
                assert start == at and 0 < size <= limit and size >= (limit + 1) // 2 and G % 256 == 0 and G > 0 and off % 4 == 0
                at += size
            assert at == numel and len(leaves) >= 2
            offs = [l[3] for l in leaves]
            assert offs == sorted(offs) and len(set(offs)) == len(offs)


@pytest.mark.parametrize("frames,fe,chunk_frames,limit", SPLIT_SHAPES)
def test_slices_reproduce_every_elements_parameters(mods, monkeypatch, frames, fe, chunk_frames, limit):
    """slice_plans over random frame ranges -- across chunk and leaf boundaries, taken in order or not -- gives every element the
    (position in its leaf, leaf size, G, offset) of the whole plan, and moves no generator"""
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", limit)
    gen = _gen()
    plans = ops.plan_noise(frames, fe, chunk_frames, torch.device("cpu"), gen, geom=_geom(rng))
    assert isinstance(plans[0], ops.SplitNoisePlan)
    after = gen.get_offset()
    tail_is_plain = plans[1] is not None and not isinstance(plans[1], ops.SplitNoisePlan)
    split_frames = frames - (plans[1].chunk_frames if tail_is_plain else 0)
    rnd = random.Random(frames * 1000 + limit)
    probe = sorted({0, 1, 2, fe // 2, fe - 3, fe - 2, fe - 1} & set(range(fe)))
    whole = {f: _plan_params(ops, rng, plans, fe, f, probe) for f in range(frames)}
    cuts = sorted(rnd.sample(range(1, split_frames), min(3, split_frames - 1))) if split_frames > 1 else []
    ranges = [(a, b) for a, b in zip([0] + cuts, cuts + [split_frames])]
    if tail_is_plain:
        ranges[-1] = (ranges[-1][0], frames)                   # the ordinary tail chunk stays whole, behind a split range
    ranges += [(f, f + 1) for f in range(split_frames)]        # single frames
    for order in (ranges, ranges[::-1]):
        for a, b in order:
            sub = ops.slice_plans(plans, a, b - a)
            assert _frames_of(ops, sub) == b - a
            for f in range(a, b):
                assert _plan_params(ops, rng, sub, fe, f - a, probe) == whole[f], (a, b, f)
            if b - a > 1 and b <= split_frames:                 # a slice of a slice
                again = ops.slice_plans(sub, 1, b - a - 1)
                assert _plan_params(ops, rng, again, fe, 0, probe) == whole[a + 1]
    assert gen.get_offset() == after
    if tail_is_plain and plans[1].chunk_frames > 1:             # the rules for ordinary chunks stay: a plain tail chunk is not cut
        with pytest.raises(ValueError):
            ops.slice_plans(plans, split_frames, plans[1].chunk_frames - 1)
        with pytest.raises(ValueError):
            ops.slice_plans(plans, split_frames - 1, 2)
    with pytest.raises(ValueError):
        ops.slice_plans(plans, frames - 1, 2)


def test_ordinary_plans_slice_as_before(mods):
    ops, rng = mods
    plans = ops.plan_noise(10, 300, 4, torch.device("cpu"), _gen(), geom=_geom(rng))
    assert all(isinstance(p, ops.NoisePlan) for p in plans[:2])
    with pytest.raises(ValueError):
        ops.slice_plans(plans, 2, 4)
    with pytest.raises(ValueError):
        ops.slice_plans(plans, 8, 1)
    main, tail, n = ops.slice_plans(plans, 4, 6)
    assert main.chunk0 == 1 and n == 1 and tail is plans[1]


@pytest.mark.parametrize("frames,fe,chunk_frames,limit", SHAPES)
def test_no_launch_meets_more_than_eight_leaves(mods, monkeypatch, frames, fe, chunk_frames, limit):
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", limit)
    plans = ops.plan_noise(frames, fe, chunk_frames, torch.device("cpu"), _gen(), geom=_geom(rng))
    for plan in plans[:2]:
        if not isinstance(plan, ops.SplitNoisePlan):
            continue
        for a, n in ((0, plan.frames), (1, plan.frames - 1), (plan.frames - 1, 1)):
            if n < 1:
                continue
            piece = ops.SplitNoisePlan(plan.chunk_frames, plan.stream, plan.first + a, n)
            at = 0
            for g0, nf, seed, leaves in ops.split_launches(piece, fe):
                assert g0 == at and nf >= 1 and seed == plan.stream.seed
                at += nf
                chunk, lo = divmod(piece.first + g0, plan.chunk_frames)
                assert lo + nf <= plan.chunk_frames                                # a launch stays inside one chunk
                met = plan.stream.leaves_of(chunk, lo * fe, (lo + nf) * fe)
                if leaves is None:
                    assert nf == 1 and len(met) > rng.NOISE_LEAVES_MAX
                else:
                    assert leaves == met and 1 <= len(leaves) <= rng.NOISE_LEAVES_MAX
                    assert leaves[0][0] <= 0 and leaves[-1][0] + leaves[-1][1] >= nf * fe
                    # greedy: one more frame of the chunk would not have fitted
                    if lo + nf < plan.chunk_frames and g0 + nf < n:
                        assert len(plan.stream.leaves_of(chunk, lo * fe, (lo + nf + 1) * fe)) > rng.NOISE_LEAVES_MAX
            assert at == n


def test_a_frame_of_more_than_eight_leaves_takes_the_materialising_branch(mods, monkeypatch):
    """A frame of fewer than `limit` elements meets at most 3 leaves; one of more than 8 leaves needs 7 * (limit + 1) // 2 elements and more:
    1.8 G at the real limit, 3 * 35 elements under a limit of 11"""
    ops, rng = mods
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", 11)
    fe = 3 * 35
    plans = ops.plan_noise(2, fe, 0, torch.device("cpu"), _gen(), geom=_geom(rng))
    launches = ops.split_launches(plans[0], fe)
    assert [(g0, n, leaves) for g0, n, _s, leaves in launches] == [(0, 1, None), (1, 1, None)]
    assert ops._split_records(plans[0], fe) is None             # what ops.film_grain / fused_chain / chain_stats branch on
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", 60)
    plans = ops.plan_noise(2, fe, 0, torch.device("cpu"), _gen(), geom=_geom(rng))
    records = ops._split_records(plans[0], fe)
    assert records and all(1 <= rec.count <= 8 for _g0, _n, rec in records)
    for limit in (2 ** 29, 3_000_000, 60):                      # a frame below the limit: at most 3 leaves
        for numel in (limit + 1, 3 * limit + 7, 9 * limit - 1):
            monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", limit)
            leaves = rng.split_32bit(numel)
            sizes = [s for _a, s in leaves]
            assert min(sizes) >= (limit + 1) // 2 and max(sizes) <= limit
            starts = [a for a, _s in leaves]
            for lo in (0, numel // 3, numel - limit):
                hi = min(numel, lo + limit - 1)
                assert bisect.bisect_left(starts, hi) - (bisect.bisect_right(starts, lo) - 1) <= 3


def test_records_hold_the_leaves_by_value(mods):
    ops, rng = mods
    from comfyui_vrgamedevgirl_amd import _hip
    assert _hip.NOISE_LEAVES_MAX == rng.NOISE_LEAVES_MAX == 8
    leaves = [(-5, 40, 512, 8), (35, 41, 256, 12)]
    rec = _hip.NoiseSplit.of(123, leaves)
    assert rec.seed == 123 and rec.count == 2
    assert [(l.start, l.size, l.grid_threads, l.offset) for l in rec.leaves[:2]] == leaves
    with pytest.raises(ValueError):
        _hip.NoiseSplit.of(1, [])
    with pytest.raises(ValueError):
        _hip.NoiseSplit.of(1, leaves * 5)


def test_the_split_entry_points_refuse_bad_tables(mods):
    """argument validation of the split entry points without a device: null table, counts outside 1 .. 8, overlap, gap, a grid that is
    no multiple of 256, a table that does not reach the launch's last element"""
    import ctypes as C
    from comfyui_vrgamedevgirl_amd import _hip, build_ext
    if not os.path.exists(_hip.LIB_PATH):
        build_ext.build(verbose=False)
    lib = _hip.load_library()
    one, two, null = C.c_void_p(16), C.c_void_p(1 << 30), C.c_void_p(0)
    fe = 4 * 4 * 3

    def grain(rec, frames=2):
        return lib.vrg_grain_split_f32(one, two, frames, 4, 4, 0.1, 0.5, 0.5, C.byref(rec) if rec is not None else None, null)

    good = [(-10, 40, 256, 8), (30, 100, 512, 12)]
    assert grain(None) == 1
    assert grain(_hip.NoiseSplit.of(1, good), frames=0) == 0                                  # zero frames: no launch
    for bad in ([(-10, 40, 256, 8), (31, 100, 512, 12)],         # gap
                [(-10, 40, 256, 8), (29, 100, 512, 12)],         # overlap
                [(-10, 40, 256, 8), (30, 100, 500, 12)],         # grid
                [(-10, 40, 256, 8), (30, 100, 0, 12)],
                [(-10, 40, 256, 8), (30, 2 * fe - 31, 512, 12)],  # ends one element before the launch does
                [(1, 2 * fe, 256, 8)]):                            # begins behind the launch's first element
        assert grain(_hip.NoiseSplit.of(1, bad)) == 1, bad
    rec = _hip.NoiseSplit.of(1, good)
    for count in (0, -1, 9):
        rec.count = count
        assert grain(rec) == 1
    cd = _hip.ChainDesc(stages=_hip.STAGE_GRAIN | _hip.STAGE_SHARPEN, stencil_op=0, border=0)
    bad = _hip.NoiseSplit.of(1, [(-10, 40, 256, 8), (31, 100, 512, 12)])
    ok = _hip.NoiseSplit.of(1, good)
    for fn in (lib.vrg_fused_chain_split_f32, lib.vrg_fused_chain_split_u8):
        assert fn(one, two, 2, 4, 4, C.byref(cd), C.byref(bad), null) == 1
        assert fn(one, two, 2, 4, 4, C.byref(cd), None, null) == 1
        assert fn(one, one, 2, 4, 4, C.byref(cd), C.byref(ok), null) == 1                      # in == out under a stencil
        no_grain = _hip.ChainDesc(stages=_hip.STAGE_SHARPEN, stencil_op=0, border=0)
        assert fn(one, two, 2, 4, 4, C.byref(no_grain), C.byref(ok), null) == 1                # a split table without a grain stage
        with_cm = _hip.ChainDesc(stages=_hip.STAGE_GRAIN | _hip.STAGE_COLORMATCH)
        assert fn(one, two, 2, 4, 4, C.byref(with_cm), C.byref(ok), null) == 2                 # pass 2 has no grain stage: unsupported
    st = _hip.ChainDesc(stages=_hip.STAGE_GRAIN)
    assert lib.vrg_chain_stats_lab_split_f32(one, two, 2, 4, 4, C.byref(st), C.byref(bad), one, one, null) == 1
    assert lib.vrg_chain_stats_lab_split_f32(one, two, 2, 4, 4, C.byref(st), None, one, one, null) == 1


def test_leaf_lookup_against_a_bisect_under_the_sanitizers(tmp_path):
    """split_leaf_of / split_covers / split_shifted / make_split of csrc/vrg_common.hpp, compiled by g++ as a stand-alone program with the
    address and undefined-behaviour sanitizers: random tables, every boundary element and its two neighbours (tests/host_math/split_noise_check.cpp)"""
    exe = str(tmp_path / "split_noise_check")
    cmd = ["g++", *HOST_FLAGS, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(PKG_DIR, "csrc"),
           HOST_SOURCE, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr + built.stdout and ("cannot find" in built.stderr or "unrecognized" in built.stderr):
        built = subprocess.run([c for c in cmd if not c.startswith(("-fsanitize", "-fno-sanitize"))], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and ran.stdout.startswith("split_noise_check:") and not ran.stderr, ran.stderr
    assert int(ran.stdout.split()[1]) > 100000


def test_the_node_takes_the_deferred_branch_for_long_batches(mods, monkeypatch):
    """FastFilmGrain.apply_grain with batch_size 0 on a batch beyond the limit: whole-batch reservation, pieces of any frame count
    (multiple_of 1), kind and fuse handed on -- seen through a stand-in for _run_grouped, no device involved"""
    ops, rng = mods
    from comfyui_vrgamedevgirl_amd import nodes
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", 60)
    monkeypatch.setattr(rng, "device_geometry", lambda device=None: _geom(rng))
    monkeypatch.setattr(nodes, "compute_device", lambda: torch.device("cpu"))
    want = _gen()
    rng.reserve_split(2 * 105, None, want, _geom(rng))
    gen = _gen()
    monkeypatch.setattr(rng, "_generator_for", lambda device, generator: gen)          # "the primary device's global generator"
    seen = {}

    def run_grouped(images, fn, multiple_of=1, fn_for_device=None, kind=None, fuse=None, stage_for_device=None):
        seen.update(multiple_of=multiple_of, kind=kind, fuse=fuse)
        return images

    monkeypatch.setattr(nodes, "_run_grouped", run_grouped)
    x = torch.zeros((2, 5, 7, 3))
    nodes.FastFilmGrain().apply_grain(x, 0.05, 0.4, 0)
    assert seen["multiple_of"] == 1 and seen["kind"] == "grain"
    assert isinstance(seen["fuse"]["plans"][0], ops.SplitNoisePlan) and seen["fuse"]["step"] == 2
    assert gen.get_offset() == want.get_offset()                # reserved once, when the node is called
    # an ordinary batch keeps whole-chunk pieces
    nodes.FastFilmGrain().apply_grain(torch.zeros((4, 2, 2, 3)), 0.05, 0.4, 2)
    assert seen["multiple_of"] == 2 and isinstance(seen["fuse"]["plans"][0], ops.NoisePlan)
    # a split chunk followed by an ordinary tail chunk: the immediate route, whole chunks
    nodes.FastFilmGrain().apply_grain(torch.zeros((5, 5, 7, 3)), 0.05, 0.4, 4)      # 4 * 105 > 60, tail 105 > 60 too -> still deferred
    assert seen["kind"] == "grain" and seen["multiple_of"] == 1
    monkeypatch.setattr(rng, "MAX_CHUNK_NUMEL", 110)
    seen.clear()
    nodes.FastFilmGrain().apply_grain(torch.zeros((5, 5, 7, 3)), 0.05, 0.4, 4)      # tail of 105 <= 110: one ordinary draw
    assert seen["kind"] is None and seen["multiple_of"] == 4

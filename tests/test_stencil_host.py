"""The stand-alone stencil's sweep on the host: tests/stencil_support.SWEEP must reach every class of the flat march's launch geometry
and the other two routes, and the oracle that tests/test_gpu_stencil.py holds the kernels to bit for bit must itself stay within a
measured distance of the float64 operators at these shapes -- channel counts other than 3 and frames of several strips included, for
which the reference left no fixture."""
import numpy as np

import stencil_support as S


def test_route_restates_the_entry_point():
    """The decisions the sweep was classified with, on shapes whose route is known from the kernel's text."""
    assert S.FLAT_ROWS % 3 == 0
    assert S.route(1, 1080, 1920, 3).route == "flat" and not S.route(1, 1080, 1920, 3).general
    assert S.route(1, 1080, 1920, 3)[2:5] == (1440, 23, 1080 // S.FLAT_ROWS + (1080 % S.FLAT_ROWS != 0))
    assert S.route(1, 6, 8, 4)[:5] == ("flat", True, 8, 1, 1)                 # the `c4` fixture of stencil.npz
    assert S.route(1, 6, 7, 3).route == "tile" and S.route(1, 6, 8, 3, aligned=False).route == "tile"
    assert S.route(1, 6, 8, 4, aligned=False).route == "generic" and S.route(1, 6, 7, 4).route == "flat"      # W * 4 floats: always whole vectors
    assert [S.route(1, 6, 8, c).route for c in (1, 2, 5)] == ["generic"] * 3
    r = S.route(2, S.FLAT_ROWS * 2 + 1, 172, 3)
    assert (r.n4, r.strips, r.segments, r.strip_overlap, r.segment_overlap, r.straddles) == (129, 3, 3, True, True, True)
    assert (r.waves_mod4, r.groups_mod8) == (18 % 4, 5 % 8)


def test_sweep_reaches_every_class():
    """A condition on the sweep, not a measurement: it fails when someone shrinks the sweep (or moves VRG_FLAT_ROWS without re-deriving
    the shapes)."""
    routed = [(c, S.case_route(c)) for c in S.SWEEP]
    assert {r.route for _, r in routed} == {"flat", "tile", "generic"}
    for C in (3, 4):
        flat = [r for c, r in routed if r.route == "flat" and c.shape[3] == C]
        have = lambda pred: any(pred(r) for r in flat)
        missing = [name for name, pred in [
            ("GENERAL", lambda r: r.general), ("steady", lambda r: not r.general),
            ("one strip", lambda r: r.strips == 1), ("two strips", lambda r: r.strips == 2), ("three or more strips", lambda r: r.strips >= 3),
            ("overlapped last strip", lambda r: r.strip_overlap), ("exact last strip", lambda r: not r.general and not r.strip_overlap),
            ("overlapped last segment", lambda r: r.segment_overlap), ("exact last segment", lambda r: not r.general and not r.segment_overlap),
            ("ragged last strip", lambda r: r.strip_ragged),
            ("ragged last segment, rows % 3 == 0", lambda r: r.segment_ragged and r.last_rows % 3 == 0),
            ("ragged last segment, rows % 3 == 1", lambda r: r.segment_ragged and r.last_rows % 3 == 1),
            ("ragged last segment, rows % 3 == 2", lambda r: r.segment_ragged and r.last_rows % 3 == 2),
            ("total_waves % 4 != 0", lambda r: r.waves_mod4 != 0), ("groups % 8 != 0", lambda r: r.groups_mod8 != 0),
            ("a workgroup straddling two frames", lambda r: r.straddles),
            ("several segments", lambda r: r.segments >= 3),
        ] if not have(pred)]
        assert not missing, (C, missing)
    generic = [c.shape[3] for c, r in routed if r.route == "generic" and c.arrangement == "aligned"]
    assert min(generic) < 3 and max(generic) > 4
    misaligned = {(c.shape[3], c.arrangement): r.route for c, r in routed if c.arrangement != "aligned"}
    assert misaligned == {**{(4, a): "generic" for a in S.ARRANGEMENTS}, **{(3, a): "tile" for a in S.ARRANGEMENTS}}
    for shape in S.MISALIGNED_SHAPES:                                        # the same frames on 16-byte bases would take the flat march
        assert S.route(*shape).route == "flat"
    assert all(int(np.prod(c.shape)) * 4 <= 400_000 for c in S.SWEEP)        # a few hundred kilobytes a case


#: (op, zero_border) -> the bound in ulp(1.0): the measured distance rounded up to the next half ulp
ORACLE_ULP = {("unsharp", False): 5.0, ("unsharp", True): 5.0, ("laplacian", False): 3.0, ("laplacian", True): 2.0,
              ("sobel", False): 4.0, ("sobel", True): 3.5}


def test_oracle_against_float64_at_the_sweep_shapes():
    """Largest distance of the fp32 oracle (stencil_support.expected) from the float64 operators (stencil_support.truth64) over every sweep
    shape, in ulp(1.0) = 2^-23; unsharp at strengths 0.5 and 3.75, laplacian and sobel at 0.8.  Measured on the CPU with the seeded inputs
    (deterministic: no further margin), asserted against the measured value rounded up to the next half ulp:

        unsharp    replicate 4.6875   zero 4.6875      (both at strength 3.75; 0.5 stays below 1)
        laplacian  replicate 2.6728   zero 1.7345
        sobel      replicate 3.6148   zero 3.4040
    """
    worst = {k: 0.0 for k in ORACLE_ULP}
    for shape in S.SHAPES:
        x = S.frames(shape)
        for op, strength, zero in S.RUNS:
            d = S.ulps(S.expected_of(shape, op, strength, zero).numpy(), S.truth64(x.numpy(), op, strength, zero))
            worst[(op, zero)] = max(worst[(op, zero)], d)
    print("\nstencil oracle vs float64, ulp(1.0): " + ", ".join(f"{op} {'zero' if z else 'replicate'} {d:.4f}" for (op, z), d in worst.items()))
    for key, bound in ORACLE_ULP.items():
        assert worst[key] <= bound, (key, worst[key], bound)

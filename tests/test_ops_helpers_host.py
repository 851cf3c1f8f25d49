"""The host helpers every operator of ops.py shares -- _placement, _checked_out, _byte_picture / _as_tensor, _uploaded, _refuse -- without a
GPU: a torch.device can be named without being there, and the table cache takes device="cpu"."""
import numpy as np
import pytest
import torch

CPU, GPU0, GPU1 = torch.device("cpu"), torch.device("cuda", 0), torch.device("cuda", 1)


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------------------------
# _placement.  HOME is the compute device, AWAY the other GPU; every row is what the code of the named site chose before the helper
# (`dev = first resident device`, then the site's own ifs), worked through by hand.
# ---------------------------------------------------------------------------------------------------------------------------------
HOME, AWAY, REFUSED = "home", "away", "refused"
RING = [
    # _grid_run, reference_sheet, msr_reference_frames, flf_guide_frames: `if dev is None or any(not cuda): ... dev = compute_device()`
    (["cpu", "cpu"], HOME),
    ([], HOME),                                     # _grid_run alone: every batch None (`elif dev is None: dev = compute_device()`)
    (["home", "home"], HOME),                       # everything resident: `dev` stays the first resident device
    (["away", "away"], AWAY),                       # ... also off the compute device (no CPU input, so the ring is not used)
    (["cpu", "home"], HOME),
    (["home", "cpu", "cpu"], HOME),
    (["cpu", "away"], REFUSED),                     # `dev != compute_device()`: "... move them there"
    (["away", "cpu"], REFUSED),
    (["home", "away"], REFUSED),                    # `any(s.is_cuda and s.device != dev)`; _grid_run: "batch i lives on ..., the grid on ..."
    (["cpu", "home", "away"], REFUSED),
    (["cpu", "away", "home"], REFUSED),
]
FOLLOW = [
    # _refbatch_place, _assemble_prepare, anchor_frames: `dev = on[0] if on else compute_device()`, `if any(d != dev for d in on): raise`
    (["cpu", "cpu"], HOME),
    ([], HOME),
    (["home", "home"], HOME),
    (["away", "away"], AWAY),
    (["cpu", "home"], HOME),
    (["cpu", "away"], AWAY),                        # the CPU inputs follow the resident one
    (["away", "cpu", "cpu"], AWAY),
    (["home", "away"], REFUSED),
    (["cpu", "away", "home"], REFUSED),
]
PREFER = [
    # anchor_frames: `on[0] if on else (out.device if out is a CUDA tensor else compute_device())` -- (inputs, device of out, expected)
    (["cpu", "cpu"], "away", AWAY),
    (["cpu"], "home", HOME),
    (["cpu"], None, HOME),
    (["cpu", "home"], "away", HOME),                # a resident input wins over `out` (whose device _checked_out then refuses)
    (["away"], "home", AWAY),
    (["home", "away"], "home", REFUSED),
]


@pytest.mark.parametrize("home", (GPU0, GPU1), ids=str)
def test_placement_chooses_and_refuses_as_the_seven_sites_did(ops, monkeypatch, home):
    from comfyui_vrgamedevgirl_amd import _devices
    monkeypatch.setattr(_devices, "compute_device", lambda: home)
    name = {"cpu": CPU, "home": home, "away": GPU1 if home == GPU0 else GPU0, None: None}
    rows = [(d, True, None, w) for d, w in RING] + [(d, False, None, w) for d, w in FOLLOW] + [(d, False, p, w) for d, p, w in PREFER]
    for devices, ring, prefer, want in rows:
        args = ([name[d] for d in devices], "some operator", "clips")
        if want == REFUSED:
            with pytest.raises(RuntimeError, match="^some operator: .*clips") as caught:
                ops._placement(*args, ring=ring, prefer=name[prefer])
            assert type(caught.value) is RuntimeError, (devices, ring)
        else:
            got = ops._placement(*args, ring=ring, prefer=name[prefer])
            assert isinstance(got, torch.device) and got == name[want], (devices, ring, prefer, got)


def test_placement_asks_for_the_compute_device_only_when_it_decides(ops, monkeypatch):
    from comfyui_vrgamedevgirl_amd import _devices

    def nowhere():
        raise AssertionError("compute_device() was asked")
    monkeypatch.setattr(_devices, "compute_device", nowhere)
    assert ops._placement([GPU1, GPU1], "w", "n", ring=True) == GPU1
    assert ops._placement([CPU, GPU1], "w", "n", ring=False) == GPU1
    assert ops._placement([CPU], "w", "n", ring=False, prefer=GPU1) == GPU1


# ---------------------------------------------------------------------------------------------------------------------------------
# _checked_out
# ---------------------------------------------------------------------------------------------------------------------------------
def test_checked_out_allocates_or_hands_the_callers_tensor_back(ops):
    made = ops._checked_out(None, (2, 3, 5), torch.uint8, CPU, "op")
    assert tuple(made.shape) == (2, 3, 5) and made.dtype == torch.uint8 and made.device == CPU and made.is_contiguous()
    made = ops._checked_out(None, torch.Size((4, 0, 3)), torch.float32, CPU, "op")             # a shape as tensors carry it; an empty one
    assert tuple(made.shape) == (4, 0, 3) and made.dtype == torch.float32
    mine = torch.empty((2, 3, 5), dtype=torch.float32)
    assert ops._checked_out(mine, (2, 3, 5), torch.float32, CPU, "op") is mine
    assert ops._checked_out(mine, mine.shape, torch.float32, CPU, "op", "mask_out") is mine
    piece = torch.empty((6, 3, 5))[2:4]                                                          # a contiguous slice is taken as it is
    assert ops._checked_out(piece, (2, 3, 5), torch.float32, CPU, "op") is piece


@pytest.mark.parametrize("bad", ("shape", "dtype", "view", "device", "list", "array"))
def test_checked_out_refuses_with_a_value_error_that_names_the_operator_and_the_argument(ops, bad):
    out = {"shape": torch.empty((2, 3, 4)), "dtype": torch.empty((2, 3, 5), dtype=torch.float64),
           "view": torch.empty((2, 5, 3)).transpose(1, 2), "device": torch.empty((2, 3, 5), device="meta"),
           "list": [[0.0] * 5] * 6, "array": np.zeros((2, 3, 5), np.float32)}[bad]
    for name in ("out", "clean_out"):
        with pytest.raises(ValueError, match=rf"^some operator: {name} must be a contiguous float32 \[2, 3, 5\] tensor on cpu$"):
            ops._checked_out(out, (2, 3, 5), torch.float32, CPU, "some operator", name)


def test_out_like_is_checked_out_plus_the_alias_refusal(ops):
    x = torch.zeros((2, 3, 4, 3))
    fresh = ops._out_like(x, None, "op")
    assert fresh.shape == x.shape and fresh.dtype == x.dtype and fresh.data_ptr() != x.data_ptr()
    other = torch.empty_like(x)
    assert ops._out_like(x, other, "op") is other
    with pytest.raises(ValueError, match="^op: out must not alias"):
        ops._out_like(x, x, "op")
    with pytest.raises(ValueError, match="^op: out must be a contiguous float32"):
        ops._out_like(x, "nothing", "op")
    empty = torch.zeros((0, 3, 4, 3))
    assert ops._out_like(empty, empty, "op") is empty                  # nothing is read or written: not an alias
    # two views of one allocation: any shared byte is refused, ranges that only touch are taken
    buf = torch.zeros((5, 3, 4, 3))
    flat = buf.view(-1)
    n = x.numel()
    for start in (1, n - 1):                                           # out one element after the input's start; out's first element the input's last
        with pytest.raises(ValueError, match="^op: out must not alias"):
            ops._out_like(flat[:n].view(x.shape), flat[start:start + n].view(x.shape), "op")
    with pytest.raises(ValueError, match="^op: out must not alias"):
        ops._out_like(buf[1:3], buf[:2], "op")                         # out's last frame is the input's first
    assert ops._out_like(buf[:2], buf[2:4], "op").data_ptr() == buf[2:4].data_ptr()            # out starts exactly where the input ends
    assert ops._out_like(buf[2:4], buf[:2], "op").data_ptr() == buf.data_ptr()                 # out ends exactly where the input starts


# ---------------------------------------------------------------------------------------------------------------------------------
# _byte_picture / _as_tensor
# ---------------------------------------------------------------------------------------------------------------------------------
def test_byte_picture_takes_arrays_read_only_arrays_and_tensors(ops):
    a = np.random.default_rng(1).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    locked = a.copy()
    locked.flags.writeable = False
    grad_free = torch.from_numpy(a.copy())
    got = [ops._byte_picture(p, "picture 0", allow_empty=False) for p in (a, locked, grad_free, a[:, ::-1])]
    for g, want in zip(got, (a, a, a, a[:, ::-1])):
        assert isinstance(g, torch.Tensor) and g.dtype == torch.uint8 and tuple(g.shape) == (5, 7, 3) and not g.requires_grad
        assert np.array_equal(g.numpy(), want)
    assert got[0].data_ptr() == a.ctypes.data                           # a writable contiguous array is used where it lies
    assert got[1].data_ptr() != locked.ctypes.data                      # the read-only one is copied: not aliased ...
    got[1].fill_(0)
    assert np.array_equal(locked, a) and not locked.flags.writeable     # ... and not written
    assert got[2].data_ptr() == grad_free.data_ptr()


def test_as_tensor_is_the_conversion_alone(ops):
    f = np.linspace(0, 1, 24, dtype=np.float32).reshape(2, 3, 4)
    f.flags.writeable = False
    t = ops._as_tensor(f)
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 3, 4) and np.array_equal(t.numpy(), f)     # any type and rank
    weights = torch.ones(3, requires_grad=True)
    assert not ops._as_tensor(weights * 2).requires_grad
    assert ops._as_tensor("a path") == "a path" and ops._as_tensor(None) is None                         # left for the caller's refusal


@pytest.mark.parametrize("allow_empty", (True, False))
def test_byte_picture_refusals(ops, allow_empty):
    for bad in (np.zeros((5, 7, 3), np.float32), torch.zeros((5, 7, 3)), np.zeros((5, 7), np.uint8), np.zeros((5, 7, 4), np.uint8),
                torch.zeros((1, 5, 7, 3), dtype=torch.uint8), [[1, 2, 3]], None):
        with pytest.raises(ValueError, match=r"^node: picture 3 must be a (non-empty )?\[height, width, 3\] uint8 tensor or array$"):
            ops._byte_picture(bad, "node: picture 3", allow_empty=allow_empty)
    for empty in (np.zeros((0, 5, 3), np.uint8), torch.zeros((5, 0, 3), dtype=torch.uint8)):
        if allow_empty:
            assert tuple(ops._byte_picture(empty, "p", allow_empty=True).shape) == tuple(empty.shape)
        else:
            with pytest.raises(ValueError, match="^p must be a non-empty"):
                ops._byte_picture(empty, "p", allow_empty=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# _uploaded
# ---------------------------------------------------------------------------------------------------------------------------------
def _counting(ops, cache, limit=None):
    built = []

    def get(key):
        def build():
            built.append(key)
            return np.full(3, key, dtype=np.int16)
        return ops._uploaded(cache, key, build, "cpu") if limit is None else ops._uploaded(cache, key, build, "cpu", limit=limit)
    return built, get


def test_uploaded_builds_once_per_key_and_returns_the_records_as_bytes(ops):
    cache = {}
    built, get = _counting(ops, cache)
    first = get(7)
    assert first.dtype == torch.uint8 and np.array_equal(first.numpy().view(np.int16), [7, 7, 7])
    assert get(7) is first and get(8) is not first and get(7) is first
    assert built == [7, 8] and set(cache) == {7, 8}


@pytest.mark.parametrize("limit", (None, 256, 3))
def test_uploaded_clears_a_full_cache_before_the_next_entry(ops, limit):
    cache = {}
    built, get = _counting(ops, cache, limit)
    n = 64 if limit is None else limit
    for key in range(n):
        get(key)
    assert len(cache) == n and built == list(range(n))
    get(0)
    assert len(cache) == n and len(built) == n                           # a hit at the limit evicts nothing
    get(n)
    assert set(cache) == {n}                                             # entry limit + 1: everything else is gone
    get(0)
    assert set(cache) == {n, 0} and built[-2:] == [n, 0]


def test_the_five_table_caches_are_plain_dicts_behind_the_one_lock(ops):
    for name in ("_lanczos_tables", "_area_tables", "_msr_tables", "_grid_tables", "_warp_tables"):
        assert type(getattr(ops, name)) is dict, name
    assert not hasattr(ops, "_grid_lock") and not hasattr(ops, "_warp_lock")
    table = np.arange(6, dtype=np.int32)
    ops._grid_tables.clear()
    try:
        t = ops._grid_table(5, 6, 3, table, "cpu")
        assert ops._grid_table(5, 6, 3, table, "cpu") is t and list(ops._grid_tables) == [(5, 6, 3, "cpu")]
        assert np.array_equal(t.numpy().view(np.int32), table)
    finally:
        ops._grid_tables.clear()


# ---------------------------------------------------------------------------------------------------------------------------------
# _refuse
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refuse_maps_the_three_outcomes(ops):
    from comfyui_vrgamedevgirl_amd import _hip
    assert ops._refuse(_hip.VRG_OK, "op", "bad records", "too large") is None
    with pytest.raises(ValueError, match="^op: bad records$"):
        ops._refuse(_hip.VRG_ERR_BAD_ARG, "op", "bad records", "too large")
    for rc in (_hip.VRG_ERR_UNSUPPORTED, 3, -1):
        with pytest.raises(RuntimeError, match="^op: too large$") as caught:
            ops._refuse(rc, "op", "bad records", "too large")
        assert type(caught.value) is RuntimeError

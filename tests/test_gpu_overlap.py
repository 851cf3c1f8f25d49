"""Every operator of tests/overlap_support.ROWS on the GPU: a call whose written operand shares a byte with another operand is refused
before anything is launched (every byte of the shared allocation, inputs, would-be outputs and guard bands, is unchanged); operands
that only touch -- carved back to back from one allocation, reads then writes and writes then reads -- are accepted and give the bits of
the same call on separate allocations, with the inputs and the guard bands intact.  adjust and fused_chain, where overlapping calls used
to return wrong pixels silently, are also held to their device oracles in the back-to-back arrangement."""
import functools

import pytest
import torch

import overlap_support as S
from oracle import restated as R

pytestmark = pytest.mark.gpu

ROW_IDS = [S.row_id(row) for row in S.ROWS]


@pytest.fixture(scope="module")
def ops(pkg):
    from comfyui_vrgamedevgirl_amd import ops
    return ops


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def up16(n):
    return (n + 15) // 16 * 16


def operands_of(call):
    """name -> (shape, dtype) of every operand of a call, reads first"""
    both = {name: (tuple(t.shape), t.dtype) for name, t in call.reads.items()}
    both.update(call.writes)
    return both


def fill(call, tensors):
    for name, value in call.reads.items():
        tensors[name].copy_(value)


@functools.lru_cache(maxsize=None)
def separate(index):
    """the results of ROWS[index] on separately allocated operands, as raw bytes on the CPU: computed once, never written"""
    from comfyui_vrgamedevgirl_amd import ops
    call = S.call_of(index)
    tensors = {name: torch.empty(shape, dtype=dtype, device=dev()) for name, (shape, dtype) in operands_of(call).items()}
    fill(call, tensors)
    results = call.run(ops, tensors)
    torch.cuda.synchronize()
    for name, value in call.reads.items():
        assert torch.equal(tensors[name].cpu(), value), name
    return [raw(r) for r in results if r is not None]


def raw(t):
    return t.detach().contiguous().cpu().view(-1).view(torch.uint8).clone()


@pytest.mark.parametrize("index", range(len(S.ROWS)), ids=ROW_IDS)
def test_overlapping_operands_are_refused_and_nothing_is_launched(ops, index):
    row, call = S.ROWS[index], S.call_of(index)
    operands = operands_of(call)
    assert list(call.reads) == list(row.reads) and list(call.writes) == list(row.writes)
    tried = 0
    for w, other in S.pairs(row):
        (w_shape, w_dtype), (r_shape, r_dtype) = operands[w], operands[other]
        w_bytes, r_bytes = S.nbytes_of(w_shape, w_dtype), S.nbytes_of(r_shape, r_dtype)
        w_item = torch.empty((), dtype=w_dtype).element_size()
        for arrangement in S.REFUSED:
            offset = S.placement(arrangement, w_bytes, w_item, r_bytes)
            if offset is None:
                continue
            base = S.GUARD + up16(w_bytes)
            at = {other: base, w: base + offset}
            end = up16(base + r_bytes + w_bytes)
            for name, (shape, dtype) in operands.items():
                if name not in at:
                    at[name] = end
                    end = up16(end + S.nbytes_of(shape, dtype))
            total = end + S.GUARD
            buffer = S.sentinel(total, dev())
            assert all(S.GUARD <= at[n] and at[n] + S.nbytes_of(*operands[n]) <= total - S.GUARD for n in operands)
            tensors = {name: S.carve(buffer, at[name], shape, dtype) for name, (shape, dtype) in operands.items()}
            for name, value in call.reads.items():
                if name != w:
                    tensors[name].copy_(value)
            torch.cuda.synchronize()
            before = buffer.clone()
            with pytest.raises(ValueError, match=rf"^({S.MESSAGE_NAME.get(row.op, row.op)}): ({w}|{other}) must not alias ({other}|{w})"):
                call.run(ops, tensors)
            torch.cuda.synchronize()
            assert torch.equal(buffer, before), (w, other, arrangement)
            tried += 1
    assert tried >= 3 * len(S.pairs(row))                                       # (a), (b), (c) at the least, for every pair


@pytest.mark.parametrize("order", ("reads-then-writes", "writes-then-reads"))
@pytest.mark.parametrize("index", range(len(S.ROWS)), ids=ROW_IDS)
def test_operands_back_to_back_give_the_bits_of_separate_allocations(ops, index, order):
    """no gap between the operands (an operand whose length is no multiple of 16 puts the next one off the 16-byte grid), 256 sentinel
    bytes before the first and after the last"""
    call = S.call_of(index)
    operands = operands_of(call)
    names = list(operands) if order == "reads-then-writes" else list(call.writes) + list(call.reads)
    at, end = {}, S.GUARD
    for name in names:
        item = torch.empty((), dtype=operands[name][1]).element_size()
        end = (end + item - 1) // item * item                                  # an element starts on its own grid, nothing more
        at[name] = end
        end += S.nbytes_of(*operands[name])
    total = end + S.GUARD
    buffer = S.sentinel(total, dev())
    guards = buffer.clone()
    tensors = {name: S.carve(buffer, at[name], shape, dtype) for name, (shape, dtype) in operands.items()}
    fill(call, tensors)
    results = call.run(ops, tensors)
    torch.cuda.synchronize()
    want = separate(index)
    got = [raw(r) for r in results if r is not None]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), f"result {k} differs in {int((g != w).sum())} of {g.numel()} bytes"
    for name, value in call.reads.items():
        assert torch.equal(tensors[name].cpu(), value), f"{name} was written"
    assert torch.equal(buffer[:S.GUARD], guards[:S.GUARD]) and torch.equal(buffer[-S.GUARD:], guards[-S.GUARD:])
    gaps = sorted((at[n], at[n] + S.nbytes_of(*operands[n])) for n in names)
    for (_, stop), (start, _) in zip(gaps, gaps[1:]):
        assert torch.equal(buffer[stop:start], guards[stop:start])             # at most 3 bytes, where a float follows bytes


def test_an_empty_batch_may_point_anywhere(ops):
    """(h): nothing is read or written by a zero-frame call, so its operands overlap nothing"""
    x = torch.rand((2, 5, 7, 3), device=dev())
    assert ops.stencil3x3(x[:0], "unsharp", 0.5, out=x[:0]).shape == (0, 5, 7, 3)
    assert ops.film_grain(x[1:1], 0.1, 0.5, out=x[:0]).shape == (0, 5, 7, 3)
    assert ops.fused_chain(x[:0], ops.ChainSpec(sharpen=("unsharp", 0.5, False)), out=x[2:]).shape == (0, 5, 7, 3)
    assert ops.adjust(x[:0], S.adjust_terms(ops), out=x[:0], workspace=x[:0]).shape == (0, 5, 7, 3)
    big, thumbs = torch.rand((1, 70, 66, 3), device=dev()), torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=dev())
    assert ops.cut_thumbnails(big[:0], out=thumbs[:0]).shape == (0, 64, 64, 3) and not thumbs.any()


def test_a_view_that_is_copied_is_judged_by_the_copy(ops):
    """a non-contiguous input reaches the kernel as _check_frames' contiguous copy: `out` inside the view's own storage is accepted"""
    storage = torch.rand((2, 9, 13, 6), device=dev())
    view = storage[..., :3]
    want = ops.stencil3x3(view.contiguous(), "unsharp", 0.5)
    out = storage.view(-1)[:view.numel()].view(view.shape)
    assert torch.equal(ops.stencil3x3(view, "unsharp", 0.5, out=out), want)


def back_to_back(names, shapes, dtype=torch.float32):
    buffer = S.sentinel(2 * S.GUARD + sum(S.nbytes_of(s, dtype) for s in shapes), dev())
    at, tensors = S.GUARD, {}
    for name, shape in zip(names, shapes):
        tensors[name] = S.carve(buffer, at, shape, dtype)
        at += S.nbytes_of(shape, dtype)
    return buffer, tensors


@pytest.mark.parametrize("shape", [(2, 24, 40, 3), (2, 6, 7, 3)], ids=["boxes", "small-box"])
def test_adjust_back_to_back_equals_the_device_oracle(ops, shape):
    """out, workspace and images in one allocation without a gap, clarity and sharpen both on (the 9-box or the small box, the 3-box and
    the fp32 ring): the oracle of test_adjust_device_arithmetic_bit_equal_device_oracle, torch's own operators on this GPU"""
    x = S._rand(shape, 301, -0.1, 1.1)
    buffer, t = back_to_back(("out", "workspace", "images"), [shape] * 3)
    guards = buffer.clone()
    t["images"].copy_(x)
    got = ops.adjust(t["images"], S.adjust_terms(ops), out=t["out"], workspace=t["workspace"])
    want = R.adjust_tensor(x.to(dev()), S.ADJUST_BOTH)
    torch.cuda.synchronize()
    assert got.data_ptr() == t["out"].data_ptr() and torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    assert torch.equal(t["images"].cpu(), x)
    assert torch.equal(buffer[:S.GUARD], guards[:S.GUARD]) and torch.equal(buffer[-S.GUARD:], guards[-S.GUARD:])


@pytest.mark.parametrize("colormatch", (False, True), ids=["grain-lut-sharpen", "lut-colormatch-sharpen"])
@pytest.mark.parametrize("shape,variant", [((2, 33, 62, 3), 1), ((2, 73, 344, 3), 0), ((2, 37, 88, 3), 2)], ids=["tile", "auto-march", "march"])
def test_fused_chain_back_to_back_equals_the_sequential_operators(ops, shape, variant, colormatch):
    """out, lab_workspace and images in one allocation without a gap: the pairing of
    test_fused_chain_equals_sequential_operators_and_oracle -- the stand-alone operators in order, which tests/test_gpu_parity.py and
    tests/test_gpu_stencil.py hold to the CPU oracle bit for bit"""
    x = S._rand(shape, 51)
    buffer, t = back_to_back(("out", "lab_workspace", "images"), [shape] * 3)
    guards = buffer.clone()
    t["images"].copy_(x)
    spec = S.chain_spec(ops, dev(), colormatch, variant)
    torch.manual_seed(77)
    got = ops.fused_chain(t["images"], spec, out=t["out"], lab_workspace=t["lab_workspace"])
    torch.manual_seed(77)
    y = x.to(dev())
    if spec.grain:
        y = ops.film_grain(y, spec.grain[0], spec.grain[1], chunk_frames=spec.grain[2])
    y = ops.lut3d(y, *spec.lut)
    if colormatch:
        y = ops.color_match(y, None, spec.colormatch[1], ref_ms=spec.colormatch[0])
    y = ops.stencil3x3(y, *spec.sharpen)
    torch.cuda.synchronize()
    assert got.data_ptr() == t["out"].data_ptr() and torch.equal(got.view(torch.int32), y.view(torch.int32))
    assert torch.equal(t["images"].cpu(), x)
    assert torch.equal(buffer[:S.GUARD], guards[:S.GUARD]) and torch.equal(buffer[-S.GUARD:], guards[-S.GUARD:])

"""Self-test of tests/guardband.py on CPU tensors: a harness that cannot fail is worth nothing, this file is the proof that it can.

Four fake operators stand for the four things a kernel wrapper can do; the guard check, bit-invariance across the fills and
finiteness must tell them apart exactly like this:

    fake operator                                  guard check   bit-equal across fills   all finite
    writes everything, reads only its input        ok            yes                      yes
    leaves its last output element unwritten       ok            no                       no
    reads one element before its input, times 0    ok            no                       no
    writes one element past its output             FAILS         yes                      yes
"""
import pytest
import torch

from guardband import FILLS, GUARD, GuardArena, GuardViolation

CPU = torch.device("cpu")
N = 37


def _before(x):
    """The element in front of x[0] (what a kernel that starts one element early reads)."""
    return torch.as_strided(x, (1,), (1,), x.storage_offset() - 1)


def _past(y, n):
    """y with n more elements than it has (what a kernel that runs one element too far writes)."""
    return torch.as_strided(y, (y.numel() + n,), (1,), y.storage_offset())


def op_good(x):
    y = torch.empty_like(x)
    y.copy_(2 * x)
    return y


def op_unwritten_tail(x):
    y = torch.empty_like(x)
    y[:-1] = 2 * x[:-1]
    return y


def op_reads_before_times_zero(x):
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    y.copy_(2 * x)
    y[0] += 0.0 * _before(x)[0]
    return y


def op_writes_past(x):
    y = torch.empty_like(x)
    _past(y, 1).copy_(torch.cat([2 * x, x[:1]]))
    return y


def _run(op):
    """(guard check ok, outputs bit-equal across the fills, all outputs finite)"""
    x = torch.randn(N, generator=torch.Generator().manual_seed(0))
    guards_ok, outs = True, []
    for fill in FILLS:
        arena = GuardArena(CPU, fill, 1 << 19)
        xp = arena.place(x)
        with arena.allocations():
            y = op(xp)
        try:
            arena.check()
        except GuardViolation:
            guards_ok = False
        outs.append(y.clone())
    bits = [o.view(torch.int32) for o in outs]
    return guards_ok, all(torch.equal(bits[0], b) for b in bits[1:]), all(bool(torch.isfinite(o).all()) for o in outs)


@pytest.mark.parametrize("op,expect", [
    (op_good, (True, True, True)),
    (op_unwritten_tail, (True, False, False)),
    (op_reads_before_times_zero, (True, False, False)),
    (op_writes_past, (False, True, True)),
])
def test_four_fake_operators_give_the_table(op, expect):
    assert _run(op) == expect


def test_fills_are_what_the_docstring_says():
    for dtype in (torch.float64, torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn):
        a = GuardArena(CPU, 0xFF, 1 << 18)
        with a.allocations():
            t = torch.empty(8, dtype=dtype)
        assert bool(torch.isnan(t.float()).all()), dtype
    a = GuardArena(CPU, 0x7B, 1 << 19)
    with a.allocations():
        f32, b16, f16 = torch.empty(4), torch.empty(4, dtype=torch.bfloat16), torch.empty(4, dtype=torch.float16)
    assert abs(float(f32[0]) / 1.3058e36 - 1) < 1e-4 and abs(float(b16[0]) / 1.3033e36 - 1) < 1e-4 and float(f16[0]) == 61280.0


@pytest.mark.parametrize("skew", [0, 4, 16, 36])
def test_place_preserves_values_shape_strides_and_skew(skew):
    arena = GuardArena(CPU, 0xFF, 1 << 20)
    wide = torch.randn(9, 24)
    for t in (torch.randn(5, 7), wide[:, :16], wide[:, 2:18], torch.randn(2, 8, 3, 5).permute(0, 2, 3, 1), torch.randn(1),
              torch.arange(12, dtype=torch.int32).view(3, 4).t()):
        p = arena.place(t, skew)
        assert p.shape == t.shape and p.stride() == t.stride() and p.dtype == t.dtype and torch.equal(p, t)
        assert p.data_ptr() % 256 == skew
        assert p.untyped_storage().data_ptr() == arena.buf.untyped_storage().data_ptr()
    # the padding columns of a strided view are poison, not the zeros or values of the buffer it was cut from
    p = arena.place(wide[:, :16])
    pad = torch.as_strided(p, (8, 8), (24, 1), p.storage_offset() + 16)
    assert bool(torch.isnan(pad).all())
    arena.check()


def test_placements_keep_clear_of_both_ends_and_of_each_other():
    arena = GuardArena(CPU, 0x7B, 1 << 20)
    with arena.allocations():
        ts = [torch.empty(100), torch.empty_like(torch.ones(3, 5)), torch.zeros(7, dtype=torch.float16), torch.full((4,), 2.5),
              torch.empty_strided((4, 4), (8, 1)), torch.zeros_like(torch.ones(6))]
    ts.append(arena.place(torch.ones(1000)))
    assert len(arena.ranges) == len(ts)
    assert float(ts[2].sum()) == 0.0 and float(ts[3].sum()) == 10.0 and float(ts[5].sum()) == 0.0 and ts[4].stride() == (8, 1)
    prev_end = -GUARD
    for (a, b, _), t in zip(arena.ranges, ts):
        assert a >= GUARD and b <= arena.nbytes - GUARD and a - prev_end >= GUARD
        assert t.data_ptr() - arena.buf.data_ptr() == a
        prev_end = b
    arena.check()
    # an arena too small for the request and its guard refuses; it never hands out memory flush against its end
    with pytest.raises(RuntimeError, match="exhausted"):
        arena.place(torch.ones((1 << 20) // 4 - 1100 - 2 * GUARD // 4))
    # the check names the bytes: one float written 8 bytes past the end of ts[0]
    torch.as_strided(ts[0], (1,), (1,), ts[0].storage_offset() + 102).fill_(1.0)
    with pytest.raises(GuardViolation) as e:
        arena.check()
    a0 = arena.ranges[0][1] + 8
    assert f"[{a0}, {a0 + 4})" in str(e.value) and "0x7B" in str(e.value)


def test_allocators_are_restored_after_an_exception_and_foreign_requests_fall_through():
    names = ("empty", "empty_like", "empty_strided", "zeros", "zeros_like", "full")
    before = {n: getattr(torch, n) for n in names}
    arena = GuardArena(CPU, 0xFF, 1 << 18)
    with pytest.raises(ZeroDivisionError):
        with arena.allocations():
            assert torch.empty is not before["empty"]
            m = torch.empty(3, device="meta")                    # another device: the real function
            s = torch.empty((2, 2), layout=torch.sparse_coo)     # something the patch does not understand
            1 / 0
    assert m.device.type == "meta" and s.layout is torch.sparse_coo and len(arena.ranges) == 0
    assert all(getattr(torch, n) is before[n] for n in names)
    # a tensor from the arena has a version counter of its own: writing to a neighbour does not invalidate what autograd saved
    with arena.allocations():
        a, b = torch.empty(4), torch.empty(4)
    v = a._version
    b.fill_(1.0)
    assert a._version == v

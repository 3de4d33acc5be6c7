"""params.derived / params.refresh on CPU tensors: the two kinds of cached copy and the one path that invalidates them.
A copy WITH a refill view is re-filled in place by refresh() and is part of the set's refresh plan; a copy WITHOUT one stands
until the parameter's version counter or address moves or a set holding the parameter is refreshed, and is in no plan."""
import pytest
import torch

from refign_amd import params

BF16 = torch.bfloat16


def _set(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(8 + i, 16, generator=g)) for i in range(n)]


@pytest.fixture
def plan_key():
    key = ("test_params_cpu", object())
    yield key
    params.forget(key)


def _doubled(p):
    return params.derived(p, "doubled", lambda t: t * 2.0)


def test_refresh_invalidates_entries_without_refill_and_keeps_the_plan(monkeypatch, plan_key):
    ps = _set(6, 1)
    lo = [params.as_dtype(p, BF16) for p in ps]
    tr = [params.transposed(p, BF16) for p in ps]
    builds = []
    build = params._build_plan
    monkeypatch.setattr(params, "_build_plan", lambda pl: builds.append(1) or build(pl))
    prev = None
    for step in range(4):
        with torch.no_grad():
            for p in ps:
                p.data.add_(0.25 * (step + 1))                     # through .data: no version counter moves
        d = _doubled(ps[2])                                         # first use since the refresh: re-made
        assert d is not prev and torch.equal(d, ps[2].detach() * 2.0), f"step {step}: the entry survived the refresh of its set"
        assert _doubled(ps[2]) is d                                 # ... and is kept until the next one
        prev = d
        params.refresh(ps, plan_key)
        for p, a, b in zip(ps, lo, tr):
            assert params.as_dtype(p, BF16) is a and params.transposed(p, BF16) is b
            assert torch.equal(a, p.detach().to(BF16)) and torch.equal(b, p.detach().to(BF16).t())
    assert _doubled(ps[2]) is not prev
    assert len(builds) == 1, f"{len(builds)} plan builds in 4 steps"


def test_refresh_of_one_set_leaves_other_parameters_alone(plan_key):
    set_a, set_b, (loner,) = _set(3, 2), _set(3, 3), _set(1, 4)
    key_b = plan_key + ("b",)
    try:
        for _ in range(2):                                          # once on the rebuild path, once on the planned path
            params.refresh(set_b, key_b)
            kept = [_doubled(set_b[1]), _doubled(loner)]
            params.refresh(set_a, plan_key)
            assert _doubled(set_b[1]) is kept[0] and _doubled(loner) is kept[1]
            assert _doubled(set_a[0]) is _doubled(set_a[0])
    finally:
        params.forget(key_b)


def test_version_reallocation_and_unplanned_refresh_invalidate():
    (p,) = _set(1, 5)
    d = _doubled(p)
    with torch.no_grad():
        p.mul_(3.0)                                                 # moves _version
    d2 = _doubled(p)
    assert d2 is not d and torch.equal(d2, p.detach() * 2.0)
    p.data = p.data.clone() + 1.0                                   # re-allocation: _version stands, the address moves
    d3 = _doubled(p)
    assert d3 is not d2 and torch.equal(d3, p.detach() * 2.0)
    p.data.sub_(0.5)
    assert _doubled(p) is d3                                        # nobody said so yet
    params.refresh([p])
    d4 = _doubled(p)
    assert d4 is not d3 and torch.equal(d4, p.detach() * 2.0)


def test_value_and_fill_target_entries(plan_key):
    ps = _set(4, 6)

    def make(t):
        base = torch.zeros(t.shape[0] + 3, t.shape[1] + 5, dtype=BF16)
        view = base[:t.shape[0], :t.shape[1]]
        view.copy_(t)
        return base, view

    def padded(p):
        return params.derived(p, "padded", make, lambda t: t)

    bases = [padded(p) for p in ps]
    addr = [b.data_ptr() for b in bases]
    for step in range(2):                                           # rebuild path, then planned path
        for p in ps:
            p.data.mul_(-1.5)
        params.refresh(ps, plan_key)
        for p, b, a in zip(ps, bases, addr):
            n, k = p.shape
            assert padded(p) is b and b.data_ptr() == a and tuple(b.shape) == (n + 3, k + 5)
            assert torch.equal(b[:n, :k], p.detach().to(BF16))
            assert not b[n:].any() and not b[:, k:].any()


def test_entries_and_forget(monkeypatch, plan_key):
    """(That forget() drops the EMA chunk table too shows on the GPU only, where ema_update builds one:
    tests/test_split32_gpu.py::test_conv2d_follows_every_kind_of_parameter_update.)"""
    ps = _set(2, 7)
    lo, d = params.as_dtype(ps[0], BF16), _doubled(ps[0])
    got = {key: (t, refill) for key, t, refill in params.entries(ps[0])}
    assert set(got) == {BF16, "doubled"}
    assert got[BF16][0] is lo and got[BF16][1] is not None
    assert got["doubled"][0] is d and got["doubled"][1] is None
    assert list(params.entries(ps[1])) == []
    builds = []
    build = params._build_plan
    monkeypatch.setattr(params, "_build_plan", lambda pl: builds.append(1) or build(pl))
    live = _set(2, 8)
    params.ema_update(ps, live, 0.5, plan_key)
    assert [key for key, _, _ in params.entries(ps[0])] == [BF16]   # the refreshed set's entry without a refill is gone
    assert torch.equal(lo, ps[0].detach().to(BF16))
    params.ema_update(ps, live, 0.5, plan_key)
    assert len(builds) == 1                                         # the plan is there ...
    params.forget(plan_key)
    params.forget(plan_key)                                         # (forgetting twice is fine)
    params.ema_update(ps, live, 0.5, plan_key)
    assert len(builds) == 2                                         # ... until it is forgotten
    assert params.as_dtype(ps[0], BF16) is lo and torch.equal(lo, ps[0].detach().to(BF16))

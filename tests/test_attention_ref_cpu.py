"""CPU: the attention reference, the rounding model of the kernels and the bound built on them (tests/attention_ref.py).

test_attention_gpu.py holds csrc/attn.hip to `M x E + floor`, E being the error of the rounding model on the very input.
Before anyone trusts that bound, this file shows that it has teeth: each of the defects an attention kernel typically has
(attention_ref.FAULTS), injected into the model, lands outside the bound by a factor of 2 or more on its designated cases.
"""
import math

import pytest
import torch

import attention_ref as ar

NAME = ar.DT_NAME


def _faults():
    for fault, (builder, cases, dtypes) in ar.FAULTS.items():
        for case in cases:
            for dtype in dtypes:
                yield pytest.param(fault, builder, case, dtype, id=f"{fault}-{case}-{NAME[dtype]}")


def test_case_table():
    """The table has the edges it is about, within the size limit, and every designated builder is one its case runs."""
    assert len({c[0] for c in ar.CASES}) == len(ar.CASES) == len(ar.KEY_EDGES) + len(ar.QUERY_EDGES) + 1
    for name, B, heads, Nq, Nkv, builders in ar.CASES:
        assert Nq <= 160 and Nkv <= 257 and heads <= 5 and builders, name
    assert {c[4] for c in ar.CASES if c[0] in ar.KEY_CASES} == set(ar.KEY_EDGES)
    assert {c[3] for c in ar.CASES if c[0] in ar.QUERY_CASES} == set(ar.QUERY_EDGES)
    assert (1, 5) in {(c[1], c[2]) for c in ar.CASES}
    for fault, (builder, cases, dtypes) in ar.FAULTS.items():
        assert fault in ar.FAULT_NAMES and dtypes
        for case in cases:
            assert builder in ar.CASE[case][5], (fault, case)
    assert set(ar.FAULTS) == set(ar.FAULT_NAMES)
    assert 1.0 <= ar.M <= 4.0 and math.log2(ar.M) == int(math.log2(ar.M))


def test_reference_is_autograd_of_the_textbook_formulation():
    """reference() against fp64 autograd of softmax(scale q k^T) v, and lse2 / delta against their definitions."""
    B, heads, Nq, Nkv = 2, 2, 37, 45
    q, kv, dO = (t.double() for t in ar.build_random(7, B, heads, Nq, Nkv))
    q.requires_grad_(True), kv.requires_grad_(True)
    qh = q.view(B, Nq, heads, 64).transpose(1, 2)
    k, v = kv.view(B, Nkv, 2, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
    s = (qh @ k.transpose(-2, -1)) * ar.SCALE
    want = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, Nq, heads * 64)
    want.backward(dO)
    o, lse2, delta, dq, dkv = ar.reference(q.detach(), kv.detach(), dO, heads, ar.SCALE)
    for got, ref in ((o, want.detach()), (dq, q.grad), (dkv, kv.grad)):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    lse_want = torch.logsumexp(s.detach(), -1).reshape(B * heads, Nq) * ar.LOG2E
    assert float((lse2 - lse_want).abs().max()) <= 1e-12 * float(lse_want.abs().max())
    d_want = (dO * o).view(B, Nq, heads, 64).sum(-1).transpose(1, 2).reshape(B * heads, Nq)
    assert float((delta - d_want).abs().max()) <= 1e-12 * float(d_want.abs().max())
    # delta on a stored output that is not the fp64 one
    o2 = o.bfloat16().double()
    d2 = ar.reference(q.detach(), kv.detach(), dO, heads, ar.SCALE, o=o2)[2]
    assert torch.equal(d2, (dO * o2).view(B, Nq, heads, 64).sum(-1).transpose(1, 2).reshape(B * heads, Nq))


@pytest.mark.parametrize("builder", ["random", "neg_tail", "last_spike"])
def test_builders(builder):
    """Values are exact in both 16-bit types (one reference serves both); each builder has the property it is named for."""
    B, heads, Nq, Nkv = 2, 2, 33, 95
    q, kv, dO = ar.BUILDERS[builder](3, B, heads, Nq, Nkv)
    for t in (q, kv, dO):
        assert torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t)
    Q, (K, _) = ar._heads_first(q, heads), ar._split_kv(kv, heads)
    s = ar.SCALE * (Q @ K.transpose(-2, -1))
    if builder == "neg_tail":
        assert float(s.max()) < -10 and abs(float(s.mean()) + 18) < 1
    if builder == "last_spike":
        p = s.softmax(-1)
        assert float(p[:, :, Nq // 2, Nkv - 1].min()) > 0.999
    # same seed, same tensors; another seed, other tensors
    assert torch.equal(ar.BUILDERS[builder](3, B, heads, Nq, Nkv)[0], q)
    assert not torch.equal(ar.BUILDERS[builder](4, B, heads, Nq, Nkv)[0], q)


@pytest.mark.parametrize("dtype", ar.DTYPES, ids=NAME.get)
def test_clean_emulation_is_rounding_noise(dtype):
    """With no fault the model is within a few 16-bit ulp of the reference on every case and builder of the table (and inside
    M x E by construction: its ratio to itself is 1)."""
    worst = {}
    for name, B, heads, Nq, Nkv, builders in ar.CASES:
        for builder in builders:
            ref, emu = ar.case_reference(name, builder), ar.case_emulation(name, builder, dtype)
            for t, (ek, ee, bound) in ar.compare(emu, emu, ref, heads, dtype).items():
                assert ek == ee and ee[0] <= bound[0] and ee[1] <= bound[1]
                if Nkv == 1 and t in ("dq", "dk"):
                    continue                               # mathematically zero: see test_one_key_gradients_are_zero
                assert math.isfinite(ee[0]) and math.isfinite(ee[1]), (name, builder, t)
                worst[t] = tuple(max(a, b) for a, b in zip(worst.get(t, (0, 0)), ee))
            # the statistics of the model are the reference's, to fp32 and the 16-bit o under delta
            assert float((emu[1] - ref[1]).abs().max()) <= 4 * ar.U24 * float(ref[1].abs().max().clamp(min=1))
    for t, (ef, em) in worst.items():
        assert ef <= 6 * ar.EPS[dtype] and em <= 6 * ar.EPS[dtype], (t, ef, em)


@pytest.mark.parametrize("dtype", ar.DTYPES, ids=NAME.get)
def test_one_key_gradients_are_zero(dtype):
    """Nkv = 1: P = 1, o = v bit for bit, and dq and dk vanish -- the relative metrics have no denominator there, the GPU
    test bounds the kernel's dq and dk absolutely."""
    _, B, heads, Nq, Nkv, _ = ar.CASE["k1"]
    q, kv, dO = ar.inputs("k1", "random")
    o, lse2, delta, dq, dkv = ar.case_emulation("k1", "random", dtype)
    v = ar.split_dkv(kv, heads)[1]
    assert torch.equal(o, v.double().expand(B, Nq, heads * 64))
    dk, dv = ar.split_dkv(dkv, heads)
    # (the model keeps delta in fp32 as the kernel does, so its dq and dk are fp32 dust, inside the bound the GPU test uses)
    dq_bound, dk_bound = ar.one_key_bounds(q, kv, dO, heads, ar.SCALE)
    assert bool((dq.abs() <= dq_bound).all()) and bool((dk.abs() <= dk_bound).all())
    # (the bounds are small against real gradients: dq elsewhere is of order 0.1, dk, a sum over the queries, of order 1)
    assert float(dq_bound.max()) <= 1e-3 and float(dk_bound.max()) <= 1e-2
    ref =ar.case_reference("k1", "random")
    assert float(ref[3].abs().max()) <= 1e-12 and float(ar.split_dkv(ref[4], heads)[0].abs().max()) <= 1e-12
    assert float((dv - dO.double().sum(1, keepdim=True)).abs().max()) <= 2 * ar.EPS[dtype] * float(dv.abs().max())


@pytest.mark.parametrize("fault,builder,case,dtype", list(_faults()))
def test_fault_is_outside_the_bound(fault, builder, case, dtype):
    """A kernel with this defect fails the GPU test on this case: in at least one metric of one tensor its error is 2 x the
    bound `M x E + floor` or more."""
    heads = ar.CASE[case][2]
    ref = ar.case_reference(case, builder)
    clean = ar.case_emulation(case, builder, dtype)
    bad = ar.case_emulation(case, builder, dtype, fault)
    margin = 0.0
    for t, (ek, ee, bound) in ar.compare(bad, clean, ref, heads, dtype).items():
        for err, b in zip(ek, bound):
            if err > 0:
                margin = max(margin, err / b if b > 0 else math.inf)
    assert margin >= 2.0, (fault, case, NAME[dtype], margin)


@pytest.mark.parametrize("Nkv", [1, 33, 95, 257])
@pytest.mark.parametrize("dtype", ar.DTYPES, ids=NAME.get)
def test_exact_case_on_the_model(dtype, Nkv):
    """all_equal: the claims the GPU test makes of the kernels hold for the model -- o = v0 bit for bit, dq = dK = 0,
    lse2 = log2 Nkv -- and a leaked padded key breaks the first of them."""
    B, heads, Nq = 2, 2, 33
    q, kv, dO = ar.build_all_equal(5, B, heads, Nq, Nkv)
    assert float(kv[..., :heads * 64].abs().max()) == 0 and float(q.abs().max()) <= 2 and float(dO.abs().max()) <= 2
    assert torch.equal(q, q.round()) and torch.equal(kv, kv.round()) and torch.equal(dO, dO.round())
    v0 = ar.split_dkv(kv, heads)[1][:, :1].double()
    assert torch.equal(ar.split_dkv(kv, heads)[1].double(), v0.expand(B, Nkv, heads * 64))
    o, lse2, delta, dq, dkv = ar.emulate(q, kv, dO, heads, ar.SCALE, dtype)
    assert torch.equal(o, v0.expand(B, Nq, heads * 64))
    assert float(dq.abs().max()) == 0 and float(ar.split_dkv(dkv, heads)[0].abs().max()) == 0
    assert float((lse2 - math.log2(Nkv)).abs().max()) <= 8 * ar.U24 * max(1.0, math.log2(Nkv))
    leaked = ar.emulate(q, kv, dO, heads, ar.SCALE, dtype, "extra_zero_key")[0]
    want = (v0 * Nkv / (Nkv + 1)).to(dtype).double().expand(B, Nq, heads * 64)
    assert torch.equal(leaked, want) and not torch.equal(leaked, o)

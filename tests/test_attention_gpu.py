"""GPU: the 16-bit attention kernels (csrc/attn.hip) at their edges, against fp64, under a bound that a leaked padded key or
a 1 % scale error does not pass (tests/attention_ref.py; test_attention_ref_cpu.py shows that on the CPU).

  edges       every case of attention_ref.CASES (1 ... 257 keys, 1 ... 160 queries), both types, both dK/dV forms: o, dq, dk,
              dv within `M x E + floor` of fp64, E the error of the rounding model on the same input
  statistics  lse2 and delta against fp64 under their fp32 bounds; their padded rows exactly 0
  exact       K = 0, equal V rows, small integers: o = v0 bit for bit, dq = dK = 0, lse2 = log2 Nkv
  ABI         strided operands, K / V packed by separate calls, every chunking of the dK/dV queries, nqpad > 32 nqblk,
              launch-to-launch bit equality of everything that has no atomics

Every test prints its figures before it asserts (`pytest -s`); profiles/attention_bounds.txt is such a run.
"""
import math

import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu

NAME = ar.DT_NAME
EDGES = [pytest.param(c[0], b, id=f"{c[0]}-{b}") for c in ar.CASES for b in c[5]]
ABI_CASE = "q129"                                    # (2, 2, 129, 70): five query blocks, three key blocks padded to four
_RUNS = {}


def _run(dev, case, builder, dtype, launch=0, **kw):
    """run_kernels on a case of the table, contiguous operands unless `kw` says otherwise; CPU tensors, computed once per
    distinct call (`launch` tells two launches of the same call apart)."""
    key = (case, builder, dtype, launch, tuple(sorted(kw.items())))
    if key not in _RUNS:
        q, kv, dO = (t.to(dev, dtype) for t in ar.inputs(case, builder))
        res = ar.run_kernels(q, kv, dO, ar.CASE[case][2], ar.SCALE, **kw)
        _RUNS[key] = tuple(t.cpu() for t in res)
    return _RUNS[key]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b, names):
    for x, y, n in zip(a, b, ("o", "lse2", "delta", "dq", "dkv")):
        if n in names:
            assert torch.equal(_bits(x), _bits(y)), n


def _hold(got, case, builder, dtype, label):
    """o, dq, dk, dv of a kernel run within M x E + floor of the fp64 reference, in both metrics."""
    _, B, heads, Nq, Nkv, _ = ar.CASE[case]
    ref, emu = ar.case_reference(case, builder), ar.case_emulation(case, builder, dtype)
    bad = []
    for t, (ek, ee, bound) in ar.compare(got, emu, ref, heads, dtype).items():
        if Nkv == 1 and t in ("dq", "dk"):
            # mathematically zero, no range to divide by: the absolute fp32 bound of attention_ref.one_key_bounds
            dq_bound, dk_bound = ar.one_key_bounds(*ar.inputs(case, builder), heads, ar.SCALE)
            x, b = (got[3], dq_bound) if t == "dq" else (ar.split_dkv(got[4], heads)[0], dk_bound)
            worst = float((x.double().abs() - b).max())
            print(f"ATTN_ZERO {case} {builder} {NAME[dtype]} {label} {t} max|x| {float(x.abs().max()):.3e} bound {float(b.max()):.3e}")
            if not worst <= 0:
                bad.append((t, "absolute", worst))
            continue
        ratio = [k / e if e > 0 else (0.0 if k == 0 else math.inf) for k, e in zip(ek, ee)]
        print(f"ATTN_BOUND {case} {builder} {NAME[dtype]} {label} {t} E_F kernel {ek[0]:.3e} model {ee[0]:.3e} ratio {ratio[0]:.3f} "
              f"E_max kernel {ek[1]:.3e} model {ee[1]:.3e} ratio {ratio[1]:.3f} floor {bound[1] - ar.M * ee[1]:.3e}")
        if not (ek[0] <= bound[0] and ek[1] <= bound[1]):
            bad.append((t, ek, ee, bound))
    assert not bad, (case, builder, NAME[dtype], label, bad)


def _check_statistics(got, case, builder, dtype, nqpad):
    _, B, heads, Nq, Nkv, _ = ar.CASE[case]
    q, kv, dO = ar.inputs(case, builder)
    o, lse2, delta = got[0], got[1].double(), got[2].double()
    assert lse2.shape == delta.shape == (B * heads, nqpad)
    ref = ar.reference(q, kv, dO, heads, ar.SCALE, o=o)
    lb, db = ar.lse2_bound(q, kv, heads, ar.SCALE, ref[1]), ar.delta_bound(dO, o, heads)
    le, de = (lse2[:, :Nq] - ref[1]).abs(), (delta[:, :Nq] - ref[2]).abs()
    print(f"ATTN_STAT {case} {builder} {NAME[dtype]} nqpad {nqpad} lse2 worst err/bound {float((le / lb).max()):.3f} "
          f"delta worst err/bound {float((de / db.clamp(min=1e-300)).max()):.3f}")
    assert bool((le <= lb).all()), ("lse2", float((le / lb).max()))
    assert bool((de <= db).all()), ("delta", float((de - db).max()))
    # the rows dK/dV streams in beside its zero packs: exp2(0 - garbage) * (0 - garbage) is not zero
    assert torch.equal(lse2[:, Nq:], torch.zeros(B * heads, nqpad - Nq, dtype=torch.float64)), "padded rows of lse2"
    assert torch.equal(delta[:, Nq:], torch.zeros(B * heads, nqpad - Nq, dtype=torch.float64)), "padded rows of delta"


# ---------------------------------------------------------------------------------------------------------------------
# 1. edges against the bound, in the layout mfma.attention uses
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ar.DTYPES, ids=NAME.get)
@pytest.mark.parametrize("case,builder", EDGES)
def test_edges_within_rounding_model_bound(dev, case, builder, dtype):
    """Contiguous operands, nqpad = 32 nqblk, one pack call of 2 x heads, the atomic and the deterministic dK/dV."""
    for det in (False, True):
        _hold(_run(dev, case, builder, dtype, det=det), case, builder, dtype, "det" if det else "atomic")
    # the forward and dQ of the two runs are the same launches on the same data
    _same_bits(_run(dev, case, builder, dtype, det=False), _run(dev, case, builder, dtype, det=True),
               ("o", "lse2", "delta", "dq"))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the statistics the forward and dQ hand to dK/dV
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ar.DTYPES, ids=NAME.get)
@pytest.mark.parametrize("case,builder", EDGES)
def test_statistics(dev, case, builder, dtype):
    nqpad = 32 * -(-ar.CASE[case][3] // 32)
    _check_statistics(_run(dev, case, builder, dtype, det=False), case, builder, dtype, nqpad)


@pytest.mark.parametrize("dtype", ar.DTYPES, ids=NAME.get)
@pytest.mark.parametrize("case", ["q1", "q128", "q129", "q160", "k257"])
def test_statistics_rows_beyond_the_packs(dev, case, dtype):
    """nqpad = 32 nqblk + 64: at 128 queries that is 64 rows past the last query tile of the forward's grid.  The outputs do
    not depend on nqpad."""
    nqpad = 32 * -(-ar.CASE[case][3] // 32) + 64
    got = _run(dev, case, "random", dtype, det=True, nqpad=nqpad)
    _check_statistics(got, case, "random", dtype, nqpad)
    _hold(got, case, "random", dtype, f"det-nqpad{nqpad}")
    _same_bits(got, _run(dev, case, "random", dtype, det=True), ("o", "dq", "dkv"))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the exact case
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ar.DTYPES, ids=NAME.get)
@pytest.mark.parametrize("Nkv", [1, 33, 95, 257])
def test_all_equal_keys_are_exact(dev, Nkv, dtype):
    """K = 0, every V row v0, integers of magnitude <= 2: every score is exactly 0 (so fma(s, c, -mrun) is exact), every dot
    product is exact in fp32 in any order.  o = v0 bit for bit -- one leaked padded key makes it v0 Nkv / (Nkv + 1) -- and
    dq = dK = 0 exactly (dP = delta = dO . v0); lse2 = log2 Nkv to log2f's accuracy."""
    B, heads, Nq = 2, 2, 33
    q, kv, dO = ar.build_all_equal(5, B, heads, Nq, Nkv)
    v0 = ar.split_dkv(kv, heads)[1][:, :1]
    for det in (False, True):
        o, lse2, delta, dq, dkv = (t.cpu() for t in ar.run_kernels(q.to(dev, dtype), kv.to(dev, dtype), dO.to(dev, dtype), heads,
                                                                  ar.SCALE, det=det))
        lerr = float((lse2[:, :Nq].double() - math.log2(Nkv)).abs().max())
        print(f"ATTN_EXACT Nkv {Nkv} {NAME[dtype]} {'det' if det else 'atomic'} o-v0 {float((o.float() - v0).abs().max()):.3e} "
              f"|dq| {float(dq.float().abs().max()):.3e} |dk| {float(ar.split_dkv(dkv, heads)[0].float().abs().max()):.3e} "
              f"lse2 err {lerr:.3e}")
        assert torch.equal(_bits(o), _bits(v0.expand(B, Nq, heads * 64).to(dtype))), "o != v0"
        assert float(dq.float().abs().max()) == 0.0, "dq"
        assert float(ar.split_dkv(dkv, heads)[0].float().abs().max()) == 0.0, "dK"
        assert lerr <= 8 * ar.U24 * max(1.0, math.log2(Nkv)), ("lse2", lerr)
        want_delta = (dO * v0).view(B, Nq, heads, 64).sum(-1).transpose(1, 2).reshape(B * heads, Nq)
        assert torch.equal(delta[:, :Nq], want_delta), "delta"


# ---------------------------------------------------------------------------------------------------------------------
# 4. the freedoms of the ABI that mfma.attention never uses
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ar.DTYPES, ids=NAME.get)
def test_strided_operands(dev, dtype):
    """Q, O (and dO, which shares O's strides) and dQ as column slices of wider tensors with three different row strides and
    batch strides that are not Nq x row stride; KV as a slice of a wider tensor.  Nothing outside the slices is touched,
    and everything without atomics is bit-equal to the contiguous run."""
    _, B, heads, Nq, Nkv, _ = ar.CASE[ABI_CASE]
    C = heads * 64
    q, kv, dO = (t.to(dev, dtype) for t in ar.inputs(ABI_CASE, "random"))
    wide = lambda rows, width: torch.full((B, rows, width), ar.POISON, dtype=dtype, device=dev)   # noqa: E731
    q_w, o_w, g_w, dq_w, kv_w = wide(Nq + 3, C + 8), wide(Nq + 1, C + 16), wide(Nq + 1, C + 16), wide(Nq + 2, C + 24), \
        wide(Nkv + 2, 2 * C + 8)
    q_v, o_v, g_v, dq_v, kv_v = q_w[:, :Nq, 8:], o_w[:, :Nq, 8:8 + C], g_w[:, :Nq, :C], dq_w[:, :Nq, 16:16 + C], kv_w[:, :Nkv, 8:]
    q_v.copy_(q), g_v.copy_(dO), kv_v.copy_(kv)
    assert len({q_v.stride(1), o_v.stride(1), dq_v.stride(1)}) == 3
    for t in (q_v, o_v, dq_v):
        assert t.stride(0) != Nq * t.stride(1) and not t.is_contiguous()
    for det in (False, True):
        o_w.fill_(ar.POISON), dq_w.fill_(ar.POISON)
        got = tuple(t.cpu() for t in ar.run_kernels(q_v, kv_v, g_v, heads, ar.SCALE, o=o_v, dq=dq_v, det=det))
        _hold(got, ABI_CASE, "random", dtype, "strided-" + ("det" if det else "atomic"))
        _same_bits(got, _run(dev, ABI_CASE, "random", dtype, det=det),
                   ("o", "lse2", "delta", "dq") + (("dkv",) if det else ()))
        for w, v in ((o_w, o_v), (dq_w, dq_v)):
            outside = torch.ones_like(w, dtype=torch.bool)
            outside[:, :Nq, v.storage_offset() % w.stride(1):v.storage_offset() % w.stride(1) + C] = False
            assert bool((w[outside] == ar.POISON).all()), "a store outside the slice"
    # the operands were read only
    assert torch.equal(q_v, q) and torch.equal(g_v, dO) and torch.equal(kv_v, kv)


@pytest.mark.parametrize("dtype", ar.DTYPES, ids=NAME.get)
def test_separate_k_and_v_packs(dev, dtype):
    """K and V packed by two rfn_attn_pack calls with kv_pack_heads = heads: the forward and dQ read the same blocks at other
    addresses, so o, the statistics and dq are bit-equal to the one-call 2 x heads layout."""
    for det in (False, True):
        got = _run(dev, ABI_CASE, "random", dtype, det=det, split_kv_pack=True)
        _hold(got, ABI_CASE, "random", dtype, "splitpack-" + ("det" if det else "atomic"))
        _same_bits(got, _run(dev, ABI_CASE, "random", dtype, det=det), ("o", "lse2", "delta", "dq") + (("dkv",) if det else ()))


@pytest.mark.parametrize("dtype", ar.DTYPES, ids=NAME.get)
@pytest.mark.parametrize("chunk", [1, 2, 4, 5, 7])
def test_query_chunking(dev, chunk, dtype):
    """blocks_per_chunk at nqblk = 5: one block per chunk, a ragged last chunk (2, 4), exactly one chunk (5), more than nqblk
    (7).  Both dK/dV forms stay inside the bound; the deterministic form is bit-equal from launch to launch."""
    assert -(-ar.CASE[ABI_CASE][3] // 32) == 5
    for det in (False, True):
        got = _run(dev, ABI_CASE, "random", dtype, det=det, blocks_per_chunk=chunk)
        _hold(got, ABI_CASE, "random", dtype, f"chunk{chunk}-" + ("det" if det else "atomic"))
    _same_bits(_run(dev, ABI_CASE, "random", dtype, det=True, blocks_per_chunk=chunk),
               _run(dev, ABI_CASE, "random", dtype, launch=1, det=True, blocks_per_chunk=chunk),
               ("o", "lse2", "delta", "dq", "dkv"))


@pytest.mark.parametrize("dtype", ar.DTYPES, ids=NAME.get)
@pytest.mark.parametrize("case", [ABI_CASE, "k257", "h5"])
def test_forward_and_dq_are_deterministic(dev, case, dtype):
    """The forward and dQ have no atomics: two launches agree bit for bit (and so does the deterministic dK/dV)."""
    _same_bits(_run(dev, case, "random", dtype, det=True), _run(dev, case, "random", dtype, launch=1, det=True),
               ("o", "lse2", "delta", "dq", "dkv"))

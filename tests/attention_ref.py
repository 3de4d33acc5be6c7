"""Reference, rounding model and raw-ABI driver for the 16-bit attention kernels (refign_amd/csrc/attn.hip).

Used by test_attention_ref_cpu.py (which shows that the bounds below have teeth) and test_attention_gpu.py (which holds the
kernels to them).  Everything except run_kernels is plain torch on the CPU.

  reference   fp64 attention and its gradients on the 16-bit values as given
  emulate     the same mathematics with a rounding wherever the kernels round (and, optionally, one injected fault)
  run_kernels rfn_attn_pack / _fwd / _bwd_dq / _bwd_dkv[_det] through the C ABI with every argument explicit
  builders    random, neg_tail, last_spike, all_equal
  CASES       the table of shapes every test walks; FAULTS the designated (fault, builder, cases, types)

Tensor layout is the kernels': q, dO, o, dq (B, Nq, heads * 64); kv, dkv (B, Nkv, 2 * heads * 64), K then V per token;
lse2, delta (B * heads, rows).

The bound of the GPU tests is `M * E + floor`: E is the error of `emulate` against `reference` on the very same input, in
two metrics (relative Frobenius norm; largest error over the reference's range), floor is one 16-bit ulp of the range
(largest-error metric only).  M is measured, not chosen: profiles/attention_bounds.txt holds the kernel / emulation ratios
of a run on an MI355X; M is the next power of two above 1.5 x the worst of them (the two errors are different draws of
the same rounding noise), and never more than 4.
"""
import functools
import math

import torch

LOG2E = 1.4426950408889634
M = 4.0                                       # profiles/attention_bounds.txt
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}       # one ulp of a value in [1, 2) is 2 eps; see floor()
DTYPES = (torch.bfloat16, torch.float16)
DT_CODE = {torch.bfloat16: 1, torch.float16: 2}
DT_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
PACK_BLOCK = 4096
SCALE = 0.125
U24 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# layout helpers
# ---------------------------------------------------------------------------------------------------------------------
def _heads_first(x, heads):
    B, N, _ = x.shape
    return x.double().reshape(B, N, heads, 64).transpose(1, 2)                         # (B, heads, N, 64)


def _split_kv(kv, heads):
    B, Nkv, _ = kv.shape
    k, v = kv.double().reshape(B, Nkv, 2, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)   # (B, heads, Nkv, 64) each
    return k, v


def _rows(x):
    B, heads, N, _ = x.shape
    return x.transpose(1, 2).reshape(B, N, heads * 64)


def _join_kv(dk, dv):
    B, heads, Nkv, _ = dk.shape
    return torch.stack([dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B, Nkv, 2 * heads * 64)


def split_dkv(dkv, heads):
    """(dk, dv) halves of a (B, Nkv, 2 * heads * 64) tensor, each (B, Nkv, heads * 64)."""
    C = heads * 64
    return dkv[..., :C], dkv[..., C:]


def _stat(x):
    return x.reshape(-1, x.shape[-1])                                                  # (B, heads, Nq) -> (B * heads, Nq)


# ---------------------------------------------------------------------------------------------------------------------
# fp64 reference
# ---------------------------------------------------------------------------------------------------------------------
def reference(q, kv, dO, heads, scale, o=None):
    """fp64 attention on the values as given: (o, lse2, delta, dq, dkv).  lse2 = log2 sum_j 2^(scale log2(e) s_j);
    delta = rowsum(dO o O), on `o` if it is given (the kernel's own stored output), else on the fp64 output."""
    Q, G = _heads_first(q, heads), _heads_first(dO, heads)
    K, V = _split_kv(kv, heads)
    z = (scale * LOG2E) * (Q @ K.transpose(-2, -1))
    lse2 = torch.logsumexp(z * math.log(2.0), -1) / math.log(2.0)
    P = torch.exp2(z - lse2[..., None])
    O = P @ V
    delta = (G * (O if o is None else _heads_first(o, heads))).sum(-1)
    dS = P * (G @ V.transpose(-2, -1) - delta[..., None])
    dq = scale * (dS @ K)
    dk = scale * (dS.transpose(-2, -1) @ Q)
    dv = P.transpose(-2, -1) @ G
    return _rows(O), _stat(lse2), _stat(delta), _rows(dq), _join_kv(dk, dv)


def lse2_bound(q, kv, heads, scale, lse2):
    """Per-row bound of the kernel's lse2 against fp64: the fp32 dot-product bound of the scores (64 terms) plus a few ulp
    for v_exp / log2f:  scale log2(e) 64 2^-24 max_j sum_d |q_d k_jd|  +  8 2^-24 max(1, |lse2|)."""
    Q, (K, _) = _heads_first(q, heads), _split_kv(kv, heads)
    absdot = (Q.abs() @ K.abs().transpose(-2, -1)).amax(-1)
    return _stat(scale * LOG2E * 64 * U24 * absdot) + 8 * U24 * lse2.abs().clamp(min=1.0)


def delta_bound(dO, o, heads):
    """Per-row bound of the kernel's delta against fp64 rowsum(dO o O) on the same o: 64 2^-24 sum_d |dO_d O_d|."""
    return _stat(64 * U24 * (_heads_first(dO, heads) * _heads_first(o, heads)).abs().sum(-1))


def one_key_bounds(q, kv, dO, heads, scale):
    """Nkv = 1: P = 1 and o = v, so dP - delta, dq and dk are mathematically zero and the relative metrics have no
    denominator.  What fp32 leaves: dP and delta are two fp32 sums of the same 64 products dO_d v_d in different orders,
    each within 64 2^-24 sum_d |dO_d v_d| of the exact value, so |dS_i| <= e_i = 2 * 64 2^-24 sum_d |dO_id v_d| (P <= 1), and
      |dq_id| <= scale |k_d| e_i,   |dk_d| <= scale sum_i |q_id| e_i,
    times 1.02 for the 16-bit roundings of dS and of the result.  Returns (dq bound (B, Nq, C), dk bound (B, 1, C))."""
    Q, G = _heads_first(q, heads), _heads_first(dO, heads)
    K, V = _split_kv(kv, heads)
    assert K.shape[2] == 1
    e = 2 * 64 * U24 * (G.abs() @ V.abs().transpose(-2, -1))                           # (B, heads, Nq, 1)
    return _rows(1.02 * scale * e * K.abs()), _rows(1.02 * scale * (e * Q.abs()).sum(2, keepdim=True))


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic: fp64 with a rounding where attn.hip rounds
# ---------------------------------------------------------------------------------------------------------------------
FAULT_NAMES = ("extra_zero_key", "drop_last_key", "no_delta", "p_scale_1pct", "stale_last_row")


def emulate(q, kv, dO, heads, scale, dtype, fault=None):
    """(o, lse2, delta, dq, dkv) as attn.hip computes them, in fp64 with the kernels' rounding points:
      forward  stages of 64 keys with a running maximum (attn_fwd_kernel's loop); P = exp2(c s - mrun) is rounded to
               `dtype` for the PV product (to_operands) while l sums the unrounded p (`ps += p`); o is rounded on store
               (store_rows64); lse2 = mrun + log2 l is stored as fp32
      dQ       delta = rowsum(dO o O) on the ROUNDED o, stored as fp32; dS = P o (dP - delta) is rounded (to_operands) for
               K^T dS; dq = round(scale * sum) (store_rows64's `mul`)
      dK / dV  P and dS are both rounded (to_operands) for dO^T P and Q^T dS; dK is scaled after the sum
               (`dk[db][r] * scale`); both are rounded by the finishing kernel
    The fp32 roundings of the accumulators themselves are not modelled: they are 2^-13 or less of a 16-bit ulp.
    `fault`: one of FAULT_NAMES -- what a kernel with that defect would compute."""
    assert fault is None or fault in FAULT_NAMES, fault
    rnd = lambda x: x.to(dtype).double()                   # noqa: E731
    f32 = lambda x: x.float().double()                     # noqa: E731
    Q, G = _heads_first(q, heads), _heads_first(dO, heads)
    K, V = _split_kv(kv, heads)
    Nkv = K.shape[2]
    if fault == "extra_zero_key":                          # the tail mask lets one padded key (zero K, zero V) through
        pad = torch.zeros_like(K[:, :, :1])
        K, V = torch.cat([K, pad], 2), torch.cat([V, pad], 2)
    elif fault == "drop_last_key":                         # the tail mask hides the last real key
        K, V = K[:, :, :-1], V[:, :, :-1]
    c = scale * LOG2E
    z = c * (Q @ K.transpose(-2, -1))
    n = K.shape[2]
    # forward
    mrun = torch.full(z.shape[:-1], -1e30, dtype=torch.float64)
    lrun = torch.zeros_like(mrun)
    oacc = torch.zeros_like(Q)
    for k0 in range(0, n, 64):
        zs = z[..., k0:k0 + 64]
        mnew = torch.maximum(mrun, zs.amax(-1))
        alpha = torch.exp2(mrun - mnew)
        p = torch.exp2(zs - mnew[..., None])
        lrun = lrun * alpha + p.sum(-1)
        oacc = oacc * alpha[..., None] + rnd(p) @ V[:, :, k0:k0 + 64]
        mrun = mnew
    o = rnd(oacc / lrun[..., None])
    if fault == "stale_last_row":                          # the last query row is not stored: it keeps its neighbour's
        o = o.clone()
        o[:, :, -1] = o[:, :, -2]
    lse2 = f32(mrun + torch.log2(lrun))
    # backward
    delta = f32((G * o).sum(-1))
    P = torch.exp2(z - lse2[..., None])
    if fault == "p_scale_1pct":
        P = P * 1.01
    dS = P * (G @ V.transpose(-2, -1) - (0.0 if fault == "no_delta" else delta[..., None]))
    dq = rnd(scale * (rnd(dS) @ K))
    dk = rnd(scale * (rnd(dS).transpose(-2, -1) @ Q))
    dv = rnd(rnd(P).transpose(-2, -1) @ G)
    if n > Nkv:
        dk, dv = dk[:, :, :Nkv], dv[:, :, :Nkv]
    elif n < Nkv:
        zero = torch.zeros_like(dk[:, :, :1])
        dk, dv = torch.cat([dk, zero], 2), torch.cat([dv, zero], 2)
    return _rows(o), _stat(lse2), _stat(delta), _rows(dq), _join_kv(dk, dv)


# ---------------------------------------------------------------------------------------------------------------------
# metrics and the bound
# ---------------------------------------------------------------------------------------------------------------------
def errors(got, ref):
    """(E_F, E_max): relative Frobenius norm of the error; largest error over the reference's range."""
    got, ref = got.double(), ref.double()
    d = got - ref
    norm, rng = float(ref.norm()), float(ref.max() - ref.min())
    ef = float(d.norm()) / norm if norm > 0 else (0.0 if float(d.norm()) == 0 else math.inf)
    em = float(d.abs().max()) / rng if rng > 0 else (0.0 if float(d.abs().max()) == 0 else math.inf)
    return ef, em


def floor(ref, dtype):
    """One 16-bit ulp of the tensor's range R, over R: the ulp of R in [2^e, 2^(e+1)) is 2 eps 2^e."""
    rng = float(ref.max() - ref.min())
    return 2 * EPS[dtype] * 2.0 ** math.floor(math.log2(rng)) / rng if rng > 0 else 0.0


def tensors(res, heads):
    """{name: tensor} of the four tensors the bound is about, from a (o, lse2, delta, dq, dkv) tuple."""
    o, _, _, dq, dkv = res
    dk, dv = split_dkv(dkv, heads)
    return {"o": o, "dq": dq, "dk": dk, "dv": dv}


def compare(got, emu, ref, heads, dtype):
    """Per tensor: (kernel errors, emulation errors, bounds), each an (E_F, E_max) pair."""
    g, e, r = tensors(got, heads), tensors(emu, heads), tensors(ref, heads)
    out = {}
    for name in g:
        ek, ee = errors(g[name], r[name]), errors(e[name], r[name])
        out[name] = (ek, ee, (M * ee[0], M * ee[1] + floor(r[name], dtype)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs: fp32 tensors whose values are representable in BOTH 16-bit types, so that one reference serves both
# ---------------------------------------------------------------------------------------------------------------------
def _both(x):
    return x.bfloat16().half().bfloat16().float()


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float32)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def build_random(seed, B, heads, Nq, Nkv):
    """q, kv ~ 1.5 N(0, 1), dO ~ N(0, 1)."""
    g = _gen(seed)
    C = heads * 64
    return _both(1.5 * _randn(g, B, Nq, C)), _both(1.5 * _randn(g, B, Nkv, 2 * C)), _both(_randn(g, B, Nq, C))


def build_neg_tail(seed, B, heads, Nq, Nkv):
    """q = 1.5 u + 0.5 n, k = -1.5 u + 0.5 n with u a random sign vector per head: every real score is near
    -1.5 * 1.5 * 64 * scale = -18 at scale 0.125, so a padded key of score 0 would take the whole row."""
    g = _gen(seed)
    C = heads * 64
    u = (torch.randint(0, 2, (1, 1, C), generator=g).float() * 2 - 1)
    q = 1.5 * u + 0.5 * _randn(g, B, Nq, C)
    k = -1.5 * u + 0.5 * _randn(g, B, Nkv, C)
    v = 1.5 * _randn(g, B, Nkv, C)
    return _both(q), _both(torch.cat([k, v], -1)), _both(_randn(g, B, Nq, C))


def build_last_spike(seed, B, heads, Nq, Nkv):
    """random, with k[Nkv - 1] = 4 q[Nq // 2] per (batch, head): the last real key dominates that query's row."""
    q, kv, dO = build_random(seed, B, heads, Nq, Nkv)
    C = heads * 64
    kv[:, Nkv - 1, :C] = 4 * q[:, Nq // 2, :]
    return q, _both(kv), dO


def build_all_equal(seed, B, heads, Nq, Nkv):
    """K = 0, every V row equal to v0 (per batch and head), integer entries of magnitude <= 2 in q, v0 and dO: every
    score is exactly 0 and every dot product is exact in fp32 in any order."""
    g = _gen(seed)
    C = heads * 64
    ints = lambda *shape: torch.randint(-2, 3, shape, generator=g).float()   # noqa: E731
    q, dO, v0 = ints(B, Nq, C), ints(B, Nq, C), ints(B, 1, C)
    kv = torch.cat([torch.zeros(B, Nkv, C), v0.expand(B, Nkv, C)], -1).contiguous()
    return q, kv, dO


BUILDERS = {"random": build_random, "neg_tail": build_neg_tail, "last_spike": build_last_spike,
            "all_equal": build_all_equal}


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
KEY_EDGES = (1, 31, 32, 33, 63, 64, 65, 95, 96, 255, 256, 257)     # 95 / 96: three blocks padded to four; 257: two key tiles
QUERY_EDGES = (1, 31, 32, 33, 127, 128, 129, 160)
NQ_FIXED, NKV_FIXED = 33, 70                                       # two query blocks; three key blocks padded to four


def _cases():
    out = []
    for nkv in KEY_EDGES:           # (a one-key row has no "last key that dominates": no last_spike there)
        out.append((f"k{nkv}", 2, 2, NQ_FIXED, nkv, ("random", "neg_tail") + (("last_spike",) if nkv > 1 else ())))
    for nq in QUERY_EDGES:
        out.append((f"q{nq}", 2, 2, nq, NKV_FIXED, ("random", "neg_tail")))
    out.append(("h5", 1, 5, 65, 95, ("random", "neg_tail", "last_spike")))
    return tuple(out)


CASES = _cases()                                                  # (name, B, heads, Nq, Nkv, builders)
CASE = {c[0]: c for c in CASES}
KEY_CASES = tuple(f"k{n}" for n in KEY_EDGES)
QUERY_CASES = tuple(f"q{n}" for n in QUERY_EDGES)

# fault -> (builder, cases, types): where a kernel with that defect must be caught
FAULTS = {
    "extra_zero_key": ("neg_tail", KEY_CASES + ("h5",), DTYPES),
    "drop_last_key": ("last_spike", KEY_CASES[1:] + ("h5",), DTYPES),
    "no_delta": ("random", QUERY_CASES + ("h5",), DTYPES),
    "stale_last_row": ("random", QUERY_CASES[1:] + ("h5",), DTYPES),
    # (bf16's clean Frobenius error is 0.3 %: a 1 % fault is not a factor 2 M away from it; the kernels are one template
    # over the type, so f16 speaks for both)
    "p_scale_1pct": ("random", QUERY_CASES + KEY_CASES[1:] + ("h5",), (torch.float16,)),
}


def seed_of(case, builder):
    return 1000 * [c[0] for c in CASES].index(case) + sorted(BUILDERS).index(builder)


@functools.lru_cache(maxsize=None)
def inputs(case, builder):
    """(q, kv, dO) of a case: fp32 values exact in both 16-bit types.  Shared; do not modify."""
    _, B, heads, Nq, Nkv, _ = CASE[case]
    return BUILDERS[builder](seed_of(case, builder), B, heads, Nq, Nkv)


@functools.lru_cache(maxsize=None)
def case_reference(case, builder):
    return reference(*inputs(case, builder), CASE[case][2], SCALE)


@functools.lru_cache(maxsize=None)
def case_emulation(case, builder, dtype, fault=None):
    return emulate(*inputs(case, builder), CASE[case][2], SCALE, dtype, fault)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels through the C ABI, every argument explicit
# ---------------------------------------------------------------------------------------------------------------------
POISON = 768.0                          # what run_kernels leaves in every output element and statistic nobody wrote


def _ceil(a, b):
    return -(-a // b)


def default_nkblk(Nkv):
    n = _ceil(Nkv, 32)
    return n + (n & 1)


def _check_rows(t, C, what):
    assert t.dim() == 3 and t.shape[2] == C and t.stride(2) == 1, what
    assert t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0, (what, t.stride(), t.data_ptr() % 16)


def run_kernels(q, kv, dO, heads, scale, *, o=None, dq=None, nqpad=None, nkblk=None, blocks_per_chunk=4,
                kv_pack_heads=None, split_kv_pack=False, det=False, backward=True):
    """pack -> forward -> dQ -> dK/dV on device tensors, straight through refign_amd._lib.call.

    q, dO (B, Nq, heads * 64) and kv (B, Nkv, 2 * heads * 64) may be views: their batch and row strides are passed on as
    they are (dO must have the strides of `o`: the dQ kernel addresses both with one pair).  `o`, `dq`: output views to
    write into (default: fresh contiguous tensors).  nqpad: row count of the statistics (default 32 * nqblk); nkblk: key
    blocks of the K / V packs (default: ceil(Nkv / 32) made even); blocks_per_chunk: 32-query blocks per dK/dV workgroup;
    split_kv_pack: K and V packed by two rfn_attn_pack calls of `heads` heads (kv_pack_heads = heads) instead of one call
    of 2 * heads; det: rfn_attn_bwd_dkv_det.  Returns (o, lse2, delta, dq, dkv) with lse2 / delta (B * heads, nqpad);
    every buffer starts out as POISON (accT: NaN), so an element that no kernel wrote shows."""
    from refign_amd import _lib
    dev, dtype = q.device, q.dtype
    B, Nq, C = q.shape
    Nkv = kv.shape[1]
    assert C == heads * 64 and dtype in DT_CODE and kv.dtype == dtype and dO.dtype == dtype
    nqblk, nkpad = _ceil(Nq, 32), _ceil(Nkv, 32) * 32
    nqpad = 32 * nqblk if nqpad is None else nqpad
    nkblk = default_nkblk(Nkv) if nkblk is None else nkblk
    pheads = (heads if split_kv_pack else 2 * heads) if kv_pack_heads is None else kv_pack_heads
    if o is None:
        o = torch.full((B, Nq, C), POISON, dtype=dtype, device=dev)
    if dq is None:
        dq = torch.full((B, Nq, C), POISON, dtype=dtype, device=dev)
    # everything the kernels index with is checked here, on the host, before anything is launched
    _check_rows(q, C, "q"), _check_rows(dO, C, "dO"), _check_rows(o, C, "o"), _check_rows(dq, C, "dq")
    _check_rows(kv, 2 * C, "kv")
    assert o.shape == q.shape == dq.shape == dO.shape and kv.shape[0] == B
    assert dO.stride() == o.stride(), "dO and o share one pair of strides"
    assert nkblk % 2 == 0 and nkblk * 32 >= Nkv and nqpad >= 32 * nqblk and blocks_per_chunk >= 1
    assert pheads == (heads if split_kv_pack else 2 * heads)
    dt = DT_CODE[dtype]
    ptr = lambda t: None if t is None else t.data_ptr()    # noqa: E731

    def pack(src, nheads, nrows, nblk, src2=None):
        new = lambda: torch.full((B * nheads * nblk * PACK_BLOCK,), 0xA5, dtype=torch.uint8, device=dev)   # noqa: E731
        r, t = new(), new()
        r2, t2 = (new(), new()) if src2 is not None else (None, None)
        assert src2 is None or src2.stride() == src.stride()
        _lib.call("rfn_attn_pack", dev, ptr(src), src.stride(0), src.stride(1), B, nheads, nrows, nblk, ptr(r), ptr(t),
                  ptr(src2), ptr(r2), ptr(t2))
        return r, t, r2, t2

    k_view, v_view = kv[:, :, :C], kv[:, :, C:]
    if split_kv_pack:
        kr, kt, _, _ = pack(k_view, heads, Nkv, nkblk)
        vr, vt, _, _ = pack(v_view, heads, Nkv, nkblk)
        krp, ktp, vrp, vtp = kr.data_ptr(), kt.data_ptr(), vr.data_ptr(), vt.data_ptr()
    else:
        kvr, kvt, _, _ = pack(kv, 2 * heads, Nkv, nkblk)
        voff = heads * nkblk * PACK_BLOCK
        krp, ktp, vrp, vtp = kvr.data_ptr(), kvt.data_ptr(), kvr.data_ptr() + voff, kvt.data_ptr() + voff
    lse2 = torch.full((B * heads, nqpad), POISON, dtype=torch.float32, device=dev)
    delta = torch.full((B * heads, nqpad), POISON, dtype=torch.float32, device=dev)
    _lib.call("rfn_attn_fwd", dev, ptr(q), q.stride(0), q.stride(1), krp, vtp, ptr(o), o.stride(0), o.stride(1), ptr(lse2), B,
              heads, Nq, Nkv, nkblk, nqpad, float(scale), pheads, dt)
    if not backward:
        return o, lse2, None, None, None
    _lib.call("rfn_attn_bwd_dq", dev, ptr(q), q.stride(0), q.stride(1), ptr(dO), ptr(o), o.stride(0), o.stride(1), krp, vrp,
              ktp, ptr(lse2), ptr(delta), ptr(dq), dq.stride(0), dq.stride(1), B, heads, Nq, Nkv, nkblk, nqpad, float(scale),
              pheads, dt)
    if dO.stride() == q.stride():
        qr, qt, gr, gt = pack(q, heads, Nq, nqblk, src2=dO)
    else:
        qr, qt, _, _ = pack(q, heads, Nq, nqblk)
        gr, gt, _, _ = pack(dO, heads, Nq, nqblk)
    images = _ceil(nqblk, blocks_per_chunk) if det else 1
    accT = torch.full((images * B * heads * 2 * 64 * nkpad,), math.nan, dtype=torch.float32, device=dev)
    dkv = torch.full((B, Nkv, 2 * C), POISON, dtype=dtype, device=dev)
    _lib.call("rfn_attn_bwd_dkv_det" if det else "rfn_attn_bwd_dkv", dev, ptr(k_view), ptr(v_view), kv.stride(0),
              kv.stride(1), ptr(qr), ptr(qt), ptr(gr), ptr(gt), ptr(lse2), ptr(delta), ptr(accT), ptr(dkv), B, heads, Nq, Nkv,
              nqblk, nqpad, nkpad, blocks_per_chunk, float(scale), dt)
    return o, lse2, delta, dq, dkv

"""GPU: the kernels under poisoned neighbours and stale memory (tests/guardband.py; its self-test is test_guardband_cpu.py).

Every other GPU test assumes that the memory around an operand, and the memory `torch.empty` hands to a wrapper, is harmless.
Here each case places its inputs in a GuardArena, calls the EXISTING Python wrapper inside `arena.allocations()` -- so outputs and
every internal temporary are poison until written -- and computes the reference from the un-placed inputs.  The driver runs a case
at two placements (skew 0, and the smallest alignment the wrapper's own domain check accepts) and the three fills, and asserts:

  1. guards     nothing was written outside the ranges handed out;
  2. reference  every output is within the bound of its reference under every fill (reference and bound are those of the
                existing test of the same kernel, named next to each case; the references are finite, so this also means every
                logical output element was written);
  3. invariance outputs of entry points without floating-point atomics are equal BIT FOR BIT across the three fills.  The sites
                that add with float atomics ("Audit") are exempt from 3 and run a second time in their
                deterministic form (refign_amd.determinism) with it where that form exists.

A case is `case(arena) -> {name: (got, want, bound)}`: bound a float = max |got - want|, a pair = (rtol, atol) of allclose,
want None = an output that is only held to finiteness and invariance (raw slab partials whose SUM has the reference).
Shapes are the smallest ones at which the existing tests exercise the ragged paths; nothing runs here that the suite does not run
already, only the surroundings change.  With `-s` the driver prints one line per case: arena size, time, and which outputs were
held to bit-invariance / exempt as atomic sites (profiles/guardband.txt is such a run).
"""
import math
import time

import pytest
import torch
import torch.nn.functional as F

from guardband import FILLS, GuardArena

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
EPS = {BF16: 2.0 ** -8, F16: 2.0 ** -11}                 # as in test_mfma_gpu.py
_DN = {BF16: "bf16", F16: "f16", F32: "f32"}
MiB = 1 << 20

CASES = {}
_MEMO = {}


def case(name, skew=16, nbytes=48 * MiB, atomic=(), det=False):
    """Register a case.  `skew`: the second placement's offset from a 256-byte boundary; `atomic`: outputs summed with float
    atomics (exempt from invariance); `det`: run a second time inside determinism.deterministic() with every output invariant."""
    def deco(fn):
        CASES[name] = dict(fn=fn, skew=skew, nbytes=nbytes, atomic=set(atomic), det=False)
        if det:
            CASES[name + "/det"] = dict(fn=fn, skew=skew, nbytes=nbytes, atomic=set(), det=True)
        return fn
    return deco


def _once(key, fn):
    """Inputs and reference of a case: computed at its first run (of six) and left unchanged."""
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _rand(shape, dev, dtype, seed, scale=1.0):           # test_mfma_gpu._rand
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev).to(dtype)


def _bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).clone()


def _caches():
    """Workspaces the wrappers keep between calls (the per-stream scratch of _tensor.workspace, the ticket workspace of the split
    correlation layer): set aside for the duration of a run so that they are allocated again, under the arena, and put back after
    it (a captured graph of another test may hold their addresses).  The packed weights and tables of params.derived live on the
    parameter objects, which every run creates anew."""
    from refign_amd import _tensor, correlation
    return (_tensor._WS, correlation._SPLIT_WS)


class _fresh_caches:
    def __enter__(self):
        self.saved = [(c, dict(c)) for c in _caches()]
        for c, _ in self.saved:
            c.clear()

    def __exit__(self, *exc):
        for c, old in self.saved:
            c.clear()
            c.update(old)
        return False


def _within(name, got, want, bound, ctx):
    assert got.shape == want.shape, (name, ctx, tuple(got.shape), tuple(want.shape))
    g, w = got.detach().double(), want.detach().double()
    assert bool(torch.isfinite(w).all()), (name, "reference not finite")
    err = (g - w).abs()
    if isinstance(bound, tuple):
        rtol, atol = bound
        ok = bool((err <= atol + rtol * w.abs()).all())
        lim = f"rtol {rtol} atol {atol}"
    else:
        ok = bool(float(err.max()) <= bound) if err.numel() else True
        lim = f"{bound:.4g}"
    if not ok:
        bad = ~(err <= (bound[1] + bound[0] * w.abs() if isinstance(bound, tuple) else bound))
        idx = bad.flatten().nonzero().flatten()
        raise AssertionError(f"{ctx}: output {name}: {int(bad.sum())} of {bad.numel()} elements outside the bound ({lim}); "
                             f"{int(torch.isnan(g).sum())} NaN, {int(torch.isinf(g).sum())} inf; flat indices "
                             f"{idx[:4].tolist()} ... {idx[-2:].tolist()}, got {g.flatten()[idx[:4]].tolist()}")


def _drive(name):
    from refign_amd import determinism
    spec = CASES[name]
    t0 = time.time()
    high = 0
    held, exempt = set(), set()
    try:
        for skew in (0, spec["skew"]):
            ref_bits = None
            for fill in FILLS:
                ctx = f"case {name}, skew {skew}, fill 0x{fill:02X}"
                arena = GuardArena(torch.device("cuda:0"), fill, spec["nbytes"], skew=skew)
                try:
                    with _fresh_caches():
                        if spec["det"]:
                            with determinism.deterministic():
                                res = spec["fn"](arena)
                        else:
                            res = spec["fn"](arena)
                        torch.cuda.synchronize()
                except RuntimeError as e:
                    if "HIP error" in str(e) or "illegal memory" in str(e) or "hipError" in str(e):
                        pytest.exit(f"GPU fault in {ctx}: {e}", returncode=3)      # nothing more runs on a faulted device
                    raise
                assert getattr(torch.empty, "__module__", "") != "guardband", "the allocator patch leaked out of its context"
                arena.check()                                                       # 1. guards
                high = max(high, arena.high_water)
                bits = {}
                for k, (got, want, bound) in res.items():
                    assert got is not None, (ctx, k, "the wrapper declined a placement its documented domain allows")
                    if want is None:
                        assert bool(torch.isfinite(got.double()).all()), (ctx, k, "not finite")
                    else:
                        _within(k, got, want, bound, ctx)                           # 2. reference
                    if k in spec["atomic"]:
                        exempt.add(k)
                    else:
                        held.add(k)
                        bits[k] = _bits(got)
                if ref_bits is None:
                    ref_bits = bits
                for k, b in bits.items():                                           # 3. invariance
                    if not torch.equal(b, ref_bits[k]):
                        d = (b != ref_bits[k]).flatten().nonzero().flatten()
                        raise AssertionError(f"{ctx}: output {k} differs from the run with fill 0x00 in {d.numel()} of "
                                             f"{b.numel()} elements (flat indices {d[:4].tolist()} ... {d[-2:].tolist()})")
    finally:
        _MEMO.clear()
    print(f"\nguardband {name}: arena {spec['nbytes'] // MiB} MiB (high water {high / MiB:.1f} MiB), {time.time() - t0:.2f} s, "
          f"bit-invariant: {sorted(held) or '-'}; exempt (float atomics): {sorted(exempt) or '-'}")


# =====================================================================================================================
# mfma.gemm_nt -- reference and bound of test_mfma_gpu.test_gemm_nt_matches_fp32_reference / test_gemm_nt_epilogues /
# test_gemm_nt_second_generation_kernel: fp32 product of the same 16-bit operands, 2 eps(16 bit) of the result's range.
# Second placement 16 bytes: _row_major tests data_ptr() % 16.
# =====================================================================================================================
def _gemm_nt_case(M, N, K, dtype):
    def fn(arena):
        from refign_amd.mfma import gemm_nt
        dev = arena.device

        def make():
            x, w, b = _rand((M, K), dev, dtype, 1), _rand((N, K), dev, dtype, 2, K ** -0.5), _rand((N,), dev, dtype, 3)
            xb = torch.zeros((M, K + 64), dtype=dtype, device=dev)
            xb[:, :K] = x
            want2 = x.float() @ w.float().t()
            return x, w, b, xb[:, :K], want2 + b.float(), want2
        x, w, b, xs, want, want2 = _once("in", make)
        xp, wp, bp, xsp = arena.place(x), arena.place(w), arena.place(b), arena.place(xs)   # xsp: ld = K + 64, padding = poison
        with arena.allocations():
            got = gemm_nt(xp, wp, bp)
            got2 = gemm_nt(xsp, wp)
        return {"y": (got, want, 2 * EPS[dtype] * float(want.abs().max())),
                "y_strided_x": (got2, want2, 2 * EPS[dtype] * float(want2.abs().max()))}
    return fn


for _dt in (BF16, F16):
    for _s in ((77, 8, 128), (260, 24, 64), (300, 64, 64)):
        case(f"gemm_nt/{_s[0]}x{_s[1]}x{_s[2]}/{_DN[_dt]}")(_gemm_nt_case(*_s, _dt))


def _gemm_nt_epilogue_case(dtype):
    def fn(arena):
        from refign_amd.mfma import gemm_nt
        dev = arena.device
        B, T, N, K = 3, 170, 320, 128

        def make():
            x, w, b = _rand((B * T, K), dev, dtype, 4), _rand((N, K), dev, dtype, 5, K ** -0.5), _rand((N,), dev, dtype, 6)
            res = _rand((B * T, N), dev, dtype, 7)
            mask = torch.tensor([0.0, 1.0 / 0.9, 1.0 / 0.9], device=dev)
            z = x.float() @ w.float().t() + b.float()
            return x, w, b, res, mask, res.float() + mask.repeat_interleave(T)[:, None] * z
        x, w, b, res, mask, want = _once("in", make)
        xp, wp, bp, rp, mp = (arena.place(t) for t in (x, w, b, res, mask))
        with arena.allocations():
            got = gemm_nt(xp, wp, bp, res=rp, rowscale=mp, rows_per_sample=T)
        assert torch.equal(got[:T], res[:T])                       # dropped sample: the residual passes through exactly
        return {"y": (got, want, 2 * EPS[dtype] * float(want.abs().max()))}
    return fn


for _dt in (BF16, F16):
    case(f"gemm_nt/residual_rowscale/{_DN[_dt]}")(_gemm_nt_epilogue_case(_dt))


@case("gemm_nt/second_generation/40001x320x320/bf16", nbytes=96 * MiB)
def _gemm_nt_gen2(arena):
    from refign_amd.mfma import gemm_nt
    dev, M, N, K = arena.device, 40001, 320, 320

    def make():
        x, w, b = _rand((M, K), dev, BF16, 11), _rand((N, K), dev, BF16, 12, K ** -0.5), _rand((N,), dev, BF16, 13)
        return x, w, b, x.float() @ w.float().t() + b.float()
    x, w, b, want = _once("in", make)
    xp, wp, bp = arena.place(x), arena.place(w), arena.place(b)
    with arena.allocations():
        got = gemm_nt(xp, wp, bp)
    return {"y": (got, want, 2 * EPS[BF16] * float(want.abs().max()))}


# =====================================================================================================================
# mfma.gemm_tn -- test_gemm_tn_matches_fp32_reference (partials: 1e-5 max|want| sqrt(T / 1000 + 1) + 1e-3 on their fp64 sum),
# test_gemm_tn_accumulates_into_gradient_views (2e-5 ...), test_gemm_tn_fallback_on_four_byte_aligned_views,
# test_grouped_weight_gradients_match_fp64.  Second placement 4 bytes: _tn_domain tests data_ptr() % 4 (such operands run
# gemm_tn_fallback_kernel); 16 bytes for the grouped launch (defer_gemm_tn tests % 16).
# The accumulate form adds with fp32 atomics (exempt); its deterministic form (stored slabs + sum_rows) is held to invariance.
# =====================================================================================================================
def _gemm_tn_case(T, N, K, rows, dtype, views=False, partial=True):
    def fn(arena):
        from refign_amd.mfma import gemm_tn
        dev = arena.device

        def make():
            if views:                                              # column slices [:, 2:] of buffers two columns wider
                g, x = _rand((T, N + 2), dev, dtype, 50)[:, 2:2 + N], _rand((T, K + 2), dev, dtype, 51)[:, 2:2 + K]
            else:
                g, x = _rand((T, N), dev, dtype, 8), _rand((T, K), dev, dtype, 9)
            gen = torch.Generator(device="cpu").manual_seed(20)
            gw0, gb0 = torch.randn(N, K, generator=gen).to(dev), torch.randn(N, generator=gen).to(dev)
            want = g.double().t() @ x.double()
            return g, x, gw0, gb0, want, gw0.double() + want, gb0.double() + g.double().sum(0)
        g, x, gw0, gb0, want, want_w, want_b = _once("in", make)
        root = math.sqrt(T / 1000 + 1)
        gp, xp = arena.place(g), arena.place(x)
        gw, gb = arena.place(gw0), arena.place(gb0)                # known finite values the kernel adds on top of
        out = {}
        with arena.allocations():
            if partial:
                part = gemm_tn(gp, xp, rows)
                assert part is not None and part.dtype == F32 and part.shape[1:] == (N, K)
                out["partials"] = (part, None, None)
                out["dW_partials"] = (part.double().sum(0), want, 1e-5 * float(want.abs().max()) * root + 1e-3)
            assert gemm_tn(gp, xp, rows, out=gw, bias_out=gb) is gw
        out["dW_accumulated"] = (gw, want_w, 2e-5 * float(want_w.abs().max()) * root + 1e-3)
        out["db_accumulated"] = (gb, want_b, 2e-5 * float(want_b.abs().max()) * root + 1e-3)
        return out
    return fn


_ACC = ("dW_accumulated", "db_accumulated")
for _dt in (BF16, F16):
    case(f"gemm_tn/1000x64x256_rows96/{_DN[_dt]}", skew=4, atomic=_ACC, det=True)(_gemm_tn_case(1000, 64, 256, 96, _dt))
    case(f"gemm_tn/4111x128x64/{_DN[_dt]}", skew=4, atomic=_ACC, det=True)(_gemm_tn_case(4111, 128, 64, None, _dt))
    case(f"gemm_tn/fallback_views_1000x64x64_rows96/{_DN[_dt]}", skew=4, atomic=_ACC, det=True)(
        _gemm_tn_case(1000, 64, 64, 96, _dt, views=True))


def _grouped_case(dtype, scaled):
    shapes = [(8160, 320, 320), (8160, 640, 320), (8160, 1280, 320), (8160, 320, 1280), (2040, 320, 1280), (4111, 128, 64),
              (2040, 512, 2048), (8160, 64, 64), (8160, 320, 320), (1000, 64, 256), (8160, 320, 320)]

    def fn(arena):
        from refign_amd import mfma
        dev = arena.device

        def make():
            probs = []
            gen = torch.Generator(device="cpu").manual_seed(70)
            for i, (T, N, K) in enumerate(shapes):
                g, x = _rand((T, N), dev, dtype, 30 + i), _rand((T, K), dev, dtype, 60 + i)
                gw0, gb0 = torch.randn(N, K, generator=gen).to(dev), torch.randn(N, generator=gen).to(dev)
                rps = T // 4 + 1
                rs = (torch.rand(4, generator=gen).to(dev) + 0.5) if scaled else None
                gd = g.double()
                if rs is not None:
                    gd = gd * rs.double().repeat_interleave(rps)[:T, None]
                probs.append((g, x, gw0, gb0 if i % 3 else None, rs, rps, gw0.double() + gd.t() @ x.double(),
                              gb0.double() + gd.sum(0)))
            return probs
        probs = _once("in", make)
        placed = [(arena.place(g), arena.place(x), arena.place(gw0), None if gb0 is None else arena.place(gb0),
                   None if rs is None else arena.place(rs), rps) for g, x, gw0, gb0, rs, rps, _, _ in probs]
        with arena.allocations():
            with mfma.deferred_wgrads():
                for g, x, gw, gb, rs, rps in placed:
                    assert mfma.defer_gemm_tn(g, x, gw, gb, rs, rps if scaled else 0), "outside the grouped kernel's domain"
        out = {}
        for i, ((g, x, gw, gb, rs, rps), pr) in enumerate(zip(placed, probs)):
            tol = 2e-5 * math.sqrt(g.shape[0] / 1000 + 1)
            out[f"dW{i}"] = (gw, pr[6], tol * float(pr[6].abs().max()) + 1e-3)
            if gb is not None:
                out[f"db{i}"] = (gb, pr[7], tol * float(pr[7].abs().max()) + 1e-3)
        return out
    return fn


_GROUPED_OUT = [f"dW{i}" for i in range(11)] + [f"db{i}" for i in range(11)]
for _dt in (BF16, F16):
    for _sc in (False, True):
        # (no deterministic form: defer_gemm_tn declines in deterministic mode and the caller launches gemm_tn itself)
        case(f"gemm_tn_grouped/{'scaled' if _sc else 'plain'}/{_DN[_dt]}", skew=16, nbytes=320 * MiB, atomic=_GROUPED_OUT)(
            _grouped_case(_dt, _sc))


# =====================================================================================================================
# mfma.conv2d_nhwc / conv.conv2d_mfma_grad / mfma.conv2d_nhwc_wgrad -- test_conv2d_implicit_gemm_matches_fp32_reference
# (2 eps max|want| + 1e-3), test_conv2d_autograd_on_mfma_kernels_matches_fp32_autograd, test_conv_wgrad_fallback_channels_not_a_
# multiple_of_8.  The wrappers state no pointer alignment (contiguity only): second placement 16 bytes.
# =====================================================================================================================
def _conv_fwd_case(B, H, W, C, N, k, stride, pad, dil, dtype):
    def fn(arena):
        from refign_amd.mfma import conv2d_nhwc, pack_conv_weight
        dev = arena.device

        def make():
            x = _rand((B, C, H, W), dev, dtype, 30)
            w = _rand((N, C, k, k), dev, dtype, 31, (C * k * k) ** -0.5)
            b = _rand((N,), dev, dtype, 32)
            want = F.leaky_relu(F.conv2d(x.float(), w.float(), b.float(), stride, pad, dil), 0.1).permute(0, 2, 3, 1)
            return x.permute(0, 2, 3, 1).contiguous(), w, b, want
        xh, w, b, want = _once("in", make)
        xp, wq, bp = arena.place(xh), arena.place(w), arena.place(b)
        bound = 2 * EPS[dtype] * float(want.abs().max()) + 1e-3
        with arena.allocations():
            wp = pack_conv_weight(wq, dtype)
            got = conv2d_nhwc(xp, wp, bp, k, k, stride, pad, dil, act=3)
            wide = torch.empty(want.shape[:3] + (N + 16,), dtype=dtype, device=dev)       # poison around the channel slice
            got_slice = conv2d_nhwc(xp, wp, bp, k, k, stride, pad, dil, act=3, out=wide[..., 8:8 + N])
        assert got_slice is not None
        # the columns beside the slice are still the fill
        side = torch.cat([wide[..., :8], wide[..., 8 + N:]], -1).contiguous().view(torch.uint8)
        assert bool((side == arena.fill).all()), "conv2d_nhwc(out=slice) wrote beside the channel slice"
        return {"y": (got, want, bound), "y_slice": (wide[..., 8:8 + N], want, bound)}
    return fn


for _dt in (BF16, F16):
    for _c in ((3, 9, 11, 16, 8, 3, 1, 2, 2), (1, 33, 40, 8, 64, 7, 4, 3, 1), (1, 19, 27, 88, 128, 3, 1, 1, 1)):
        case(f"conv2d_nhwc/{'x'.join(map(str, _c))}/{_DN[_dt]}")(_conv_fwd_case(*_c, _dt))


def _conv_grad_case(B, H, W, C, N, k, stride, pad, dil, dtype):
    def fn(arena):
        from refign_amd.conv import conv2d_mfma_grad
        dev = arena.device

        def make():
            x = _rand((B, C, H, W), dev, dtype, 40)
            w = _rand((N, C, k, k), dev, F32, 41, (C * k * k) ** -0.5)
            b = _rand((N,), dev, F32, 42)
            w16, b16 = w.to(dtype).float().requires_grad_(True), b.to(dtype).float().requires_grad_(True)
            x32 = x.float().requires_grad_(True)
            want = F.conv2d(x32, w16, b16, stride, pad, dil)
            gy = _rand(tuple(want.shape), dev, dtype, 43)
            want.backward(gy.float())
            return x, w, b, gy, want.detach(), x32.grad, w16.grad, b16.grad
        x, w, b, gy, want, dx, dw, db = _once("in", make)
        xp, wp, bp = (arena.place(t).requires_grad_(True) for t in (x, w, b))
        gyp = arena.place(gy)
        with arena.allocations():
            got = conv2d_mfma_grad(xp, wp, bp, stride, pad, dil, dtype)
            assert got is not None and got.shape == want.shape
            got.backward(gyp)
        e = EPS[dtype]
        tol = 1e-5 * math.sqrt(want.numel() // N / 1000 + 1)
        return {"y": (got, want, 2 * e * float(want.abs().max()) + 1e-3),
                "dx": (xp.grad, dx, 2 * e * float(dx.abs().max()) + 1e-3),
                "dw": (wp.grad, dw, tol * float(dw.abs().max()) + 1e-3),
                "db": (bp.grad, db, tol * float(db.abs().max()) + 1e-3)}
    return fn


for _dt in (BF16, F16):
    for _c in ((2, 36, 44, 3, 64, 7, 4, 3, 1), (2, 27, 30, 256, 19, 1, 1, 0, 1)):
        # db: column sums of gy added with fp32 atomics (conv2d_nhwc_wgrad bias_out); dw is the ordered sum of stored slabs
        case(f"conv2d_mfma_grad/{'x'.join(map(str, _c))}/{_DN[_dt]}", atomic=("db",), det=True)(_conv_grad_case(*_c, _dt))


def _conv_wgrad_fallback_case(dtype):
    B, H, W, C, N, k, stride, pad, dil = 2, 9, 11, 4, 64, 3, 1, 1, 1

    def fn(arena):
        from refign_amd import mfma
        dev = arena.device

        def make():
            x = _rand((B, C, H, W), dev, dtype, 55)
            w = torch.zeros((N, C, k, k), dtype=torch.float64, requires_grad=True)
            y = F.conv2d(x.cpu().double(), w, None, stride, pad, dil)
            gy = _rand(tuple(y.shape), dev, dtype, 56)
            y.backward(gy.cpu().double())
            gb0 = torch.randn(N, generator=torch.Generator().manual_seed(57)).to(dev)
            return (x.permute(0, 2, 3, 1).contiguous(), gy.permute(0, 2, 3, 1).contiguous(), gb0,
                    w.grad.permute(0, 2, 3, 1).reshape(N, k * k * C).to(dev), gb0.double() + gy.double().sum((0, 2, 3)))
        xh, gyh, gb0, want, want_b = _once("in", make)
        Kpad = -(-k * k * C // 64) * 64
        xp, gp, gb = arena.place(xh), arena.place(gyh), arena.place(gb0)
        with arena.allocations():
            part = mfma.conv2d_nhwc_wgrad(gp, xp, k, k, Kpad, stride, pad, dil, bias_out=gb)
        assert part is not None and part.shape[1:] == (N, Kpad)
        root = math.sqrt(gyh.numel() // N / 1000 + 1)
        got = part.double().sum(0)
        return {"partials": (part, None, None),
                "dW": (got[:, :k * k * C], want, 1e-5 * float(want.abs().max()) * root + 1e-3),
                "dW_padding_columns": (part[:, :, k * k * C:], torch.zeros_like(part[:, :, k * k * C:]), 0.0),
                "db": (gb, want_b, 2e-5 * float(want_b.abs().max()) * root + 1e-3)}
    return fn


for _dt in (BF16, F16):
    case(f"conv2d_nhwc_wgrad/fallback_2x9x11x4x64/{_DN[_dt]}", atomic=("db",), det=True)(_conv_wgrad_fallback_case(_dt))


# =====================================================================================================================
# mfma.attention -- test_attention_forward_backward_vs_fp32_reference (o: 4 eps max + 1e-3; gradients 2 % of range + 1e-4) and the
# gradient-free path of test_attention_spiked_scores_and_no_grad.  The R-/T-packs, lse2, delta and accT come from the patched
# allocator.  Second placement 16 bytes: _attn_ok tests data_ptr() % 16.  dK / dV are added with fp32 atomics (exempt);
# the deterministic form (one image per query chunk, added in order) is held to invariance.
# =====================================================================================================================
def _ref_attention(q, kv, heads, scale):                           # test_mfma_gpu._ref_attention
    B, N, C = q.shape
    d = C // heads
    qh = q.view(B, N, heads, d).transpose(1, 2)
    k, v = kv.view(B, -1, 2, heads, d).permute(2, 0, 3, 1, 4).unbind(0)
    a = ((qh @ k.transpose(-2, -1)) * scale).softmax(-1)
    return (a @ v).transpose(1, 2).reshape(B, N, C)


def _attention_case(B, heads, N, Nkv, dtype):
    def fn(arena):
        from refign_amd.mfma import attention
        dev, C, scale = arena.device, heads * 64, 64 ** -0.5

        def make():
            q, kv = _rand((B, N, C), dev, dtype, 10, 1.5), _rand((B, Nkv, 2 * C), dev, dtype, 11, 1.5)
            go = _rand((B, N, C), dev, dtype, 12)
            qf, kvf = q.float().requires_grad_(True), kv.float().requires_grad_(True)
            of = _ref_attention(qf, kvf, heads, scale)
            of.backward(go.float())
            return q, kv, go, of.detach(), qf.grad, kvf.grad
        q, kv, go, of, dq, dkv = _once("in", make)
        qp, kvp = arena.place(q).requires_grad_(True), arena.place(kv).requires_grad_(True)
        gop = arena.place(go)
        qn, kvn = arena.place(q), arena.place(kv)
        with arena.allocations():
            o = attention(qp, kvp, heads, scale)
            assert o is not None and o.dtype == dtype
            o.backward(gop)
            with torch.no_grad():
                o2 = attention(qn, kvn, heads, scale)
        bo = 4 * EPS[dtype] * float(of.abs().max()) + 1e-3
        return {"o": (o, of, bo), "o_no_grad": (o2, of, bo),
                "dq": (qp.grad, dq, 0.02 * float(dq.abs().max()) + 1e-4),
                "dkv": (kvp.grad, dkv, 0.02 * float(dkv.abs().max()) + 1e-4)}
    return fn


for _dt in (BF16, F16):
    for _s in ((1, 1, 31, 33), (2, 2, 333, 70)):
        case(f"attention/{'x'.join(map(str, _s))}/{_DN[_dt]}", atomic=("dkv",), det=True)(_attention_case(*_s, _dt))


# =====================================================================================================================
# LayerNorm -- test_layernorm_gpu.test_layernorm_fwd_bwd (allclose bounds restated below), test_layernorm_pass_through_sums_both_
# gradients (rfn_layernorm_bwd_add) and test_layernorm_two_consumers_and_pass_through_sum_in_the_kernel (rfn_layernorm_bwd_add2)
# at C = 320.  layernorm.py states no alignment: second placement 16 bytes.
# =====================================================================================================================
def _layernorm_case(rows, C, in_dt, out_dt):
    def fn(arena):
        from refign_amd.layernorm import layer_norm
        dev = arena.device

        def make():
            g = torch.Generator().manual_seed(rows + C)
            x = (2 * torch.randn(rows, C, generator=g) + 0.5).to(dev).to(in_dt)
            w = (1 + 0.2 * torch.randn(C, generator=g)).to(dev)
            b = (0.1 * torch.randn(C, generator=g)).to(dev)
            gy = torch.randn(rows, C, generator=g).to(dev).to(out_dt)
            xr, wr, br = x.float().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
            yr = F.layer_norm(xr, (C,), wr, br, 1e-6)
            yr.backward(gy.float())
            return x, w, b, gy, yr.detach(), xr.grad, wr.grad, br.grad
        x, w, b, gy, yr, dx, dw, db = _once("in", make)
        xp, wp, bp = (arena.place(t).requires_grad_() for t in (x, w, b))
        gyp = arena.place(gy)
        with arena.allocations():
            y = layer_norm(xp, wp, bp, 1e-6, out_dt)
            assert y.dtype == out_dt
            y.backward(gyp)
        lo = out_dt == BF16 or in_dt == BF16
        rt = rows ** 0.5
        return {"y": (y, yr, (2e-2, 2e-2) if lo else (1e-4, 1e-5)),
                "dx": (xp.grad, dx, (2e-2, 2e-2) if lo else (1e-3, 1e-4)),
                "dw": (wp.grad, dw, (2e-2 if lo else 1e-3, (2e-2 if lo else 1e-4) * rt)),
                "db": (bp.grad, db, (2e-2 if lo else 1e-3, (2e-2 if lo else 1e-4) * rt))}
    return fn


for _r, _c in ((7, 32), (5, 160), (33, 1024)):
    for _i, _o in ((F32, F32), (F32, BF16), (BF16, BF16)):
        case(f"layernorm/{_r}x{_c}/{_DN[_i]}_{_DN[_o]}")(_layernorm_case(_r, _c, _i, _o))


def _layernorm_add_case(dtype, two):
    C = 320

    def fn(arena):
        from refign_amd.layernorm import LayerNorm, layer_norm_pass, layer_norm_pass2
        dev = arena.device

        def make():
            torch.manual_seed(C + two)
            ln = LayerNorm(C, eps=1e-6).to(dev)
            shape = (2, 301, C) if two else (3, 257, C)
            gen = torch.Generator().manual_seed(5)
            x = torch.randn(shape, generator=gen).to(dev).to(dtype)
            gs = [torch.randn(shape, generator=gen).to(dev).to(dtype) for _ in range(3)]
            xb = x.clone().requires_grad_()
            yb = ln(xb)                                            # the plain LayerNorm kernel on fresh tensors: the tests' reference
            gsum = (gs[0].float() + gs[1].float()).to(dtype) if two else gs[0]
            torch.autograd.backward([yb, xb * 1.0], [gsum, gs[2]])
            return x, ln.weight.detach().clone(), ln.bias.detach().clone(), gs, yb.detach(), xb.grad, ln.weight.grad, ln.bias.grad
        x, w, b, gs, yb, dx, dw, db = _once("in", make)
        xp = arena.place(x).requires_grad_()
        wp, bp = arena.place(w).requires_grad_(), arena.place(b).requires_grad_()
        g1, g2, g3 = (arena.place(t) for t in gs)
        with arena.allocations():
            if two:
                y, y2, xq = layer_norm_pass2(xp, wp, bp, 1e-6)
                torch.autograd.backward([y, y2, xq], [g1, g2, g3])
            else:
                y, xq = layer_norm_pass(xp, wp, bp, 1e-6)
                torch.autograd.backward([y, xq], [g1, g3])
        lo = dtype == BF16
        tol = 2e-2 if lo else 1e-5
        pw = (2e-2 if lo else 1e-4, 0.3 if lo else 1e-3) if two else (1e-4, 1e-4)
        return {"y": (y, yb, 0.0), "dx": (xp.grad, dx, tol * float(dx.float().abs().max())),
                "dw": (wp.grad, dw, pw), "db": (bp.grad, db, pw)}
    return fn


for _dt in (F32, BF16):
    case(f"layernorm_bwd_add/3x257x320/{_DN[_dt]}")(_layernorm_add_case(_dt, 0))
    case(f"layernorm_bwd_add2/2x301x320/{_DN[_dt]}")(_layernorm_add_case(_dt, 1))


# =====================================================================================================================
# BatchNorm train forward / backward -- test_mfma_gpu.test_batchnorm_relu_train_kernels (bounds restated).  The batch statistics
# are summed with fp64 / fp32 atomics (exempt: everything downstream of them); the deterministic form is held to invariance.
# bn.py states no alignment for the input: second placement 16 bytes.
# =====================================================================================================================
def _bn_case(B, C, H, W, relu, dtype):
    def fn(arena):
        from refign_amd.bn import bn_act_train
        dev = arena.device

        def make():
            torch.manual_seed(0)
            ref = torch.nn.BatchNorm2d(C).to(dev)
            with torch.no_grad():
                ref.weight.uniform_(0.5, 1.5)
                ref.bias.uniform_(-0.5, 0.5)
            sd = {k: v.clone() for k, v in ref.state_dict().items()}
            x = (_rand((B, C, H, W), dev, dtype, 40, 2.0) + 0.7).contiguous(memory_format=torch.channels_last)
            g = _rand((B, C, H, W), dev, dtype, 41)
            xr = x.float().requires_grad_(True)
            yr = ref(xr)
            yr = torch.relu(yr) if relu else yr
            yr.backward(g.float())
            return (x, g, sd, yr.detach(), xr.grad, ref.weight.grad, ref.bias.grad, ref.running_mean.clone(),
                    ref.running_var.clone())
        x, g, sd, yr, dx, dw, db, rm, rv = _once("in", make)
        bn = torch.nn.BatchNorm2d(C).to(dev)
        bn.load_state_dict(sd)
        for n in ("weight", "bias"):
            getattr(bn, n).data = arena.place(getattr(bn, n).data)
        for n in ("running_mean", "running_var"):
            setattr(bn, n, arena.place(getattr(bn, n)))
        xp = arena.place(x).requires_grad_(True)
        gp = arena.place(g)
        with arena.allocations():
            y = bn_act_train(xp, bn, relu, dtype)
            y.backward(gp)
        e = EPS[dtype]
        return {"y": (y, yr, 4 * e * float(yr.abs().max()) + 1e-3),
                "dx": (xp.grad, dx, 0.02 * float(dx.abs().max()) + 1e-4),
                "dweight": (bn.weight.grad, dw, 0.02 * float(dw.abs().max()) + 1e-3),
                "dbias": (bn.bias.grad, db, 0.02 * float(db.abs().max()) + 1e-3),
                "running_mean": (bn.running_mean, rm, (1e-5, 1e-4)), "running_var": (bn.running_var, rv, (1e-4, 1e-5))}
    return fn


_BN_OUT = ("y", "dx", "dweight", "dbias", "running_mean", "running_var")
for _dt in (BF16, F16):
    for _s in ((4, 64, 9, 5, False), (2, 256, 17, 23, True)):
        case(f"batchnorm/{'x'.join(str(int(v)) for v in _s)}/{_DN[_dt]}", atomic=_BN_OUT, det=True)(_bn_case(*_s, _dt))


# =====================================================================================================================
# reduce.hip: sum_rows -- test_params_gpu.test_sum_rows (allclose rtol 1e-5, atol 2e-5 sqrt(S) + 1e-6 against fp64; ordered sums:
# bit-invariant).  params.sum_rows states no alignment: second placement 16 bytes.
# =====================================================================================================================
def _sum_rows_case(S, n, dt):
    def fn(arena):
        from refign_amd.params import sum_rows
        dev = arena.device

        def make():
            g = torch.Generator().manual_seed(S * 7 + n)
            x = torch.randn(S, n, generator=g).to(dev).to(dt)
            base = torch.randn(n, generator=g).to(dev)
            return x, base, x.double().sum(0)
        x, base, want = _once("in", make)
        xp, out = arena.place(x), arena.place(base)
        with arena.allocations():
            got = sum_rows(xp)
            sum_rows(xp, out=out, accumulate=True)
        assert got.dtype == F32 and got.shape == (n,)
        tol = (1e-5, 2e-5 * (S ** 0.5) + 1e-6)
        return {"sum": (got, want, tol), "accumulated": (out, base.double() + want, tol)}
    return fn


for _dt in (F32, BF16):
    for _s in ((3, 24), (65, 64), (1000, 320)):
        case(f"sum_rows/{_s[0]}x{_s[1]}/{_DN[_dt]}")(_sum_rows_case(*_s, _dt))


# =====================================================================================================================
# reduce.hip: multi-tensor cast / transpose-cast / permute-cast through params._cast_table, _transpose_table, _permute_table --
# test_params_gpu.test_refresh_multi_tensor_cast_is_torch_rounding / test_refresh_transposed_copies_multi_tensor: bit-equal to
# torch's conversion (bound 0).  Element counts 1, 3, 4097 and one above rfn_multi_cast_chunk_elems(); fp32 sources only need
# 4-byte alignment: second placement 4 bytes.
# =====================================================================================================================
def _numels():
    from refign_amd import _lib
    return [1, 3, 4097, _lib.load_library().rfn_multi_cast_chunk_elems() + 5]


def _multi_cast_case(dtype):
    def fn(arena):
        from refign_amd import params
        dev = arena.device
        src = _once("in", lambda: [_rand((n,), dev, F32, 80 + i) for i, n in enumerate(_numels())])
        sp = [arena.place(s) for s in src]
        with arena.allocations():
            dst = [torch.empty(s.shape, dtype=dtype, device=dev) for s in sp]
        table, nrows = params._cast_table(dst, sp, dev)
        params._multi_cast(table, nrows, dev, dtype)
        return {f"cast{i}": (d, s.to(dtype), 0.0) for i, (d, s) in enumerate(zip(dst, src))}
    return fn


def _multi_transpose_case(dtype):
    shapes = [(1, 1), (3, 1), (17, 241), (130, 127)]              # 1, 3, 4097 and 16510 elements; no multiple of the 64 x 64 tile

    def fn(arena):
        from refign_amd import _lib, params
        from refign_amd._tensor import ptr
        dev = arena.device
        assert shapes[-1][0] * shapes[-1][1] > _lib.load_library().rfn_multi_cast_chunk_elems()
        src = _once("in", lambda: [_rand(s, dev, F32, 90 + i) for i, s in enumerate(shapes)])
        sp = [arena.place(s) for s in src]                         # parameters stored (N, K)
        with arena.allocations():
            dst = [torch.empty((s.shape[1], s.shape[0]), dtype=dtype, device=dev) for s in sp]
        table, ntiles = params._transpose_table(dst, [s.t() for s in sp], dev)
        _lib.call(params._CAST16[dtype][1], dev, ptr(table), ntiles)
        return {f"transpose{i}": (d, s.t().to(dtype), 0.0) for i, (d, s) in enumerate(zip(dst, src))}
    return fn


def _multi_permute_case(dtype):
    shapes = [(1,), (3,), (17, 241), (5, 13, 2, 127)]             # 1, 3, 4097 and 16510 elements

    def fn(arena):
        from refign_amd import _lib, params
        from refign_amd._tensor import ptr
        dev = arena.device
        src = _once("in", lambda: [_rand(s, dev, F32, 100 + i) for i, s in enumerate(shapes)])
        sp = [arena.place(s) for s in src]
        views = [s.permute(*reversed(range(s.dim()))) for s in sp]            # the layout change: all dimensions reversed
        with arena.allocations():
            dst = [torch.empty(tuple(v.shape), dtype=dtype, device=dev) for v in views]
        table, nrows = params._permute_table(dst, views, dev)
        _lib.call("rfn_multi_permute_cast_f32", dev, ptr(table), nrows)
        return {f"permute{i}": (d, s.permute(*reversed(range(s.dim()))).to(dtype), 0.0)
                for i, (d, s) in enumerate(zip(dst, src))}
    return fn


for _dt in (BF16, F16):
    case(f"multi_cast/{_DN[_dt]}", skew=4)(_multi_cast_case(_dt))
    case(f"multi_transpose_cast/{_DN[_dt]}", skew=4)(_multi_transpose_case(_dt))
case("multi_permute_cast/bf16", skew=4)(_multi_permute_case(BF16))
case("multi_permute_cast/f32", skew=4)(_multi_permute_case(F32))

# =====================================================================================================================
# Depthwise 3x3 (csrc/dwconv.hip) -- forward and the fused backward through autograd: test_dwconv_gpu.test_dwconv_matches_conv2d
# (allclose bounds restated) at its smallest ragged entries (ragged W, C = 8, a dilation of 18 on a 5 x 4 map); the GELU form:
# test_fused_dwconv_gelu_matches_conv_then_exact_gelu; the statistics form and the store-free rolling-window form on the EXACT
# inputs of test_dwconv_roll_gpu (every sum exact in any order, so even the atomically added statistics are held to the bit and
# to invariance).  dwconv.py states no alignment: second placement 16 bytes.
# The weight / bias gradients of the fused backward are ordered sums over stripes (test_two_calls_are_bit_identical...).
# =====================================================================================================================
def _dwconv_case(B, H, W, C, dil, dtype):
    def fn(arena):
        from refign_amd.dwconv import dwconv3x3_nhwc
        dev = arena.device

        def make():
            g = torch.Generator().manual_seed(B * 1000 + H * 10 + C + dil)
            x = torch.randn(B, H, W, C, generator=g).to(dev).to(dtype)
            w = (0.3 * torch.randn(C, 1, 3, 3, generator=g)).to(dev)
            b = (0.1 * torch.randn(C, generator=g)).to(dev)
            gy = torch.randn(B, H, W, C, generator=g).to(dev).to(dtype)
            xr = x.float().permute(0, 3, 1, 2).requires_grad_()
            wr, br = w.clone().requires_grad_(), b.clone().requires_grad_()
            yr = F.conv2d(xr, wr, br, padding=dil, dilation=dil, groups=C)
            yr.backward(gy.float().permute(0, 3, 1, 2))
            return x, w, b, gy, yr.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad, br.grad
        x, w, b, gy, yr, dx, dw, db = _once("in", make)
        xp, wp, bp = (arena.place(t).requires_grad_() for t in (x, w, b))
        gp = arena.place(gy)
        with arena.allocations():
            y = dwconv3x3_nhwc(xp, wp, bp, dil)
            assert y.dtype == dtype and y.shape == x.shape
            y.backward(gp)
        tol = (1e-4, 1e-4) if dtype == F32 else (2e-2, 2e-2)
        rt = (B * H * W) ** 0.5
        wtol = (1e-3, 1e-3 * rt) if dtype == F32 else (2e-2, 2e-2 * rt)
        return {"y": (y, yr, tol), "dx": (xp.grad, dx, tol), "dw": (wp.grad, dw, wtol), "db": (bp.grad, db, wtol)}
    return fn


for _dt in (F32, BF16):
    for _s in ((1, 5, 3, 8, 1), (2, 19, 7, 64, 6), (3, 5, 4, 2048, 18)):
        case(f"dwconv3x3/{'x'.join(map(str, _s))}/{_DN[_dt]}")(_dwconv_case(*_s, _dt))


@case("dwconv3x3_gelu/2x9x13x64/bf16")
def _dwconv_gelu(arena):
    from refign_amd.dwconv import dwconv3x3_gelu_tokens
    dev, (B, H, W, C) = arena.device, (2, 9, 13, 64)

    def make():
        g = torch.Generator().manual_seed(C + H)
        x = (torch.randn(B, H * W, C, generator=g) * 1.5).to(dev).to(BF16)
        w = (torch.randn(C, 1, 3, 3, generator=g) * 0.4).to(dev)
        b = torch.randn(C, generator=g).to(dev)
        z = F.conv2d(x.float().view(B, H, W, C).permute(0, 3, 1, 2), w, b, padding=1, groups=C)
        z = z.permute(0, 2, 3, 1).reshape(B, H * W, C)
        return x, w, b, z, F.gelu(z)
    x, w, b, z_ref, a_ref = _once("in", make)
    xp, wp, bp = arena.place(x), arena.place(w), arena.place(b)
    xg = arena.place(x).requires_grad_()
    with arena.allocations():
        with torch.no_grad():
            a = dwconv3x3_gelu_tokens(xp, wp, bp, H, W)
        a2, z = dwconv3x3_gelu_tokens(xg, wp, bp, H, W, with_z=True)
    return {"gelu": (a, a_ref, (2.0 ** -8, 2e-3)), "gelu_with_z": (a2, a_ref, (2.0 ** -8, 2e-3)), "z": (z, z_ref, (2.0 ** -8, 2e-3))}


def _dwconv_stats_case(B, H, W, C, dil, dtype):
    def fn(arena):
        from test_dwconv_roll_gpu import _exact_conv, _exact_inputs, _exact_sums
        from refign_amd.dwconv import dwconv3x3_nhwc, dwconv3x3_stats_nhwc
        dev = arena.device

        def make():
            s0, s1 = _exact_sums(B, H, W, C, dil, dtype)
            want = torch.cat([s0, s1, torch.tensor([float(B * H * W)], dtype=torch.float64)]).to(dev)
            return _exact_inputs(B, H, W, C, dil, dtype, dev) + (_exact_conv(B, H, W, C, dil, dtype).to(dev), want)
        x, w, b, y_ref, sums_ref = _once("in", make)
        xp, wp, bp = arena.place(x), arena.place(w), arena.place(b)
        with arena.allocations(), torch.no_grad():
            sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)         # poison: the kernel may not add to it
            y = dwconv3x3_nhwc(xp, wp, bp, dil, stats=sums)                          # rfn_dwconv3x3_nhwc_fwd_stats
            free = dwconv3x3_stats_nhwc(xp, wp, bp, dil)                             # the store-free rolling-window pass
        return {"y": (y, y_ref, 0.0), "stats_storing": (sums, sums_ref, 0.0), "stats_store_free": (free, sums_ref, 0.0)}
    return fn


for _dt in (BF16, F16):
    for _s in ((2, 19, 7, 64, 6), (2, 37, 9, 8, 1)):
        # (the exact inputs make the atomically added statistics order-independent: held to invariance in both forms)
        case(f"dwconv3x3_stats/{'x'.join(map(str, _s))}/{_DN[_dt]}", det=True)(_dwconv_stats_case(*_s, _dt))


# =====================================================================================================================
# reduce.hip: MultiTensorAdamW / MultiTensorAdam on parameter sets with 1, 3, 4097 and chunk + 5 elements against torch's own step
# -- test_params_gpu.test_multi_tensor_adamw_matches_torch_fused / test_adam_gpu.test_multi_tensor_adam_matches_torch: parameters
# and both moments to 2e-6 relative.  Parameters, gradients and (created inside the patched zeros_like) both moments live in the
# arena; fp32 tensors need 4-byte alignment only: second placement 4 bytes.
# =====================================================================================================================
def _adam_case(decoupled):
    def fn(arena):
        from refign_amd.optim import MultiTensorAdam, MultiTensorAdamW
        dev = arena.device
        cls, wrap = (torch.optim.AdamW, MultiTensorAdamW) if decoupled else (torch.optim.Adam, MultiTensorAdam)

        def mk(params):
            kw = dict(fused=True) if decoupled else dict(foreach=False)
            return cls([{"params": params[:2], "lr": 1e-3, "weight_decay": 0.01},
                        {"params": params[2:], "lr": 1e-2, "weight_decay": 0.1, "betas": (0.8, 0.99)}], **kw)

        def make():
            ps = [torch.nn.Parameter(_rand((n,), dev, F32, 110 + i)) for i, n in enumerate(_numels())]
            p0 = [p.detach().clone() for p in ps]
            grads = [[_rand((p.numel(),), dev, F32, 120 + 10 * it + i, 0.1 + it) for i, p in enumerate(ps)] for it in range(3)]
            ref = mk(ps)
            for it in range(3):
                for p, g in zip(ps, grads[it]):
                    p.grad = g.clone()
                ref.step()
            return p0, grads, [p.detach() for p in ps], [ref.state[p]["exp_avg"] for p in ps], [ref.state[p]["exp_avg_sq"] for p in ps]
        p0, grads, want_p, want_m, want_v = _once("in", make)
        qs = [torch.nn.Parameter(arena.place(p)) for p in p0]
        for q in qs:
            q.grad = arena.place(torch.zeros_like(q))
        with arena.allocations():
            mine = mk(qs)
            fast = wrap(mine)
            for it in range(3):
                for q, g in zip(qs, grads[it]):
                    q.grad.copy_(g)
                fast.step()
        assert fast.launches == 2                                  # torch made the first step (state creation)
        out = {}
        for i, q in enumerate(qs):
            out[f"p{i}"] = (q.detach(), want_p[i], 2e-6 * float(want_p[i].abs().max()))
            out[f"exp_avg{i}"] = (mine.state[q]["exp_avg"], want_m[i], 2e-6 * float(want_m[i].abs().max()) + 1e-12)
            out[f"exp_avg_sq{i}"] = (mine.state[q]["exp_avg_sq"], want_v[i], 2e-6 * float(want_v[i].abs().max()) + 1e-12)
        return out
    return fn


case("multi_tensor_adamw", skew=4)(_adam_case(True))
case("multi_tensor_adam", skew=4)(_adam_case(False))

# =====================================================================================================================
# Correlation (csrc/corr.hip, gcorr.hip) against the CPU oracle as in test_ops_gpu.py: test_corr_hot_vs_oracle_ragged (rtol 1e-4,
# atol 1e-4), test_corr_backward_strip_kernel_vs_oracle, test_local_layer_fused_warp_vs_oracle (rtol 1e-3, atol 2e-5),
# test_local_correlation_layer_channel_split_matches_one_kernel_path's joined split (1, 128, 9, 12) against the oracle layer
# (rtol 1e-4, atol 1e-5, the bound of test_corr_channel_split_tiles_vs_oracle) and test_global_layer_golden.
# correlation.py asks for contiguous fp32 tensors and states no alignment: second placement 16 bytes.
# The ragged shapes (W % 4 or C % 8) take the generic backward, which scatters with float atomics: their gradients are exempt.
# =====================================================================================================================
ORACLE = None                                                      # the session's CPU oracle (conftest fixture), set by the test


def _np(a, dev):
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _corr_hot_case(shape):
    def fn(arena):
        import numpy as np
        from refign_amd.correlation import spatial_correlation_sample
        dev = arena.device

        def make():
            rng = np.random.default_rng(sum(shape))
            a, b = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
            want = ORACLE.corr_forward(a, b, patch_size=9)
            go = rng.standard_normal(want.shape).astype(np.float32)
            w1, w2 = ORACLE.corr_backward(a, b, go, patch_size=9)
            return [_np(v, dev) for v in (a, b, go, want, w1, w2)]
        a, b, go, want, w1, w2 = _once("in", make)
        ta, tb = arena.place(a).requires_grad_(), arena.place(b).requires_grad_()
        gop = arena.place(go)
        with arena.allocations():
            out = spatial_correlation_sample(ta, tb, patch_size=9)
            out.backward(gop)
        return {"out": (out, want, (1e-4, 1e-4)), "grad1": (ta.grad, w1, (1e-4, 1e-4)), "grad2": (tb.grad, w2, (1e-4, 1e-4))}
    return fn


for _s in ((1, 3, 2, 130), (2, 9, 17, 63), (1, 130, 9, 65)):
    case(f"correlation/hot_ragged/{'x'.join(map(str, _s))}", atomic=("grad1", "grad2"))(_corr_hot_case(_s))


def _corr_strip_bwd_case(shape):
    def fn(arena):
        import numpy as np
        from refign_amd import correlation
        dev = arena.device
        B, C, H, W = shape

        def make():
            rng = np.random.default_rng(sum(shape) + 7)
            a, b = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
            go = rng.standard_normal((B, 9, 9, H, W)).astype(np.float32)
            w1, w2 = ORACLE.corr_backward(a, b, go, patch_size=9)
            return [_np(v, dev) for v in (a, b, go, w1, w2)]
        a, b, go, w1, w2 = _once("in", make)
        ap, bp, gp = arena.place(a), arena.place(b), arena.place(go)
        with arena.allocations():
            g1, g2 = correlation.backward(ap, bp, gp, 1, 1, 9, 9, 0, 0, 1, 1, 1, 1, 1, 1)
        return {"grad1": (g1, w1, (1e-4, 1e-4)), "grad2": (g2, w2, (1e-4, 1e-4))}
    return fn


for _s in ((3, 8, 5, 4), (2, 16, 19, 36)):
    case(f"correlation/backward_strip/{'x'.join(map(str, _s))}")(_corr_strip_bwd_case(_s))


@case("local_correlation_layer/fused_warp/2x24x21x70")
def _local_layer_warp(arena):
    import numpy as np
    from refign_amd.correlation import local_correlation_layer
    dev, (B, C, H, W) = arena.device, (2, 24, 21, 70)

    def make():
        rng = np.random.default_rng(11)
        src = ORACLE.l2_normalize(rng.standard_normal((B, C, H, W)).astype(np.float32))
        trg = ORACLE.l2_normalize(rng.standard_normal((B, C, H, W)).astype(np.float32))
        flo = (2.5 * rng.standard_normal((B, 2, H, W))).astype(np.float32)
        flo[0, :, :3, :3] = 40.0   # out of range region
        want = ORACLE.local_correlation_layer(ORACLE.warp(src, flo), trg)
        return [_np(v, dev) for v in (src, trg, flo, want)]
    src, trg, flo, want = _once("in", make)
    sp, tp, fp = arena.place(src), arena.place(trg), arena.place(flo)
    with arena.allocations():
        two = local_correlation_layer(sp, tp, flow=fp, single_kernel_warp=False)
        one = local_correlation_layer(sp, tp, flow=fp, single_kernel_warp=True)
    return {"warp_then_correlate": (two, want, (1e-3, 2e-5)), "single_kernel_warp": (one, want, (1e-3, 2e-5))}


@case("local_correlation_layer/joined_channel_split/1x128x9x12")
def _local_layer_split(arena):
    import numpy as np
    from refign_amd import correlation
    dev, shape = arena.device, (1, 128, 9, 12)
    assert correlation._channel_splits(*shape) > 1                  # the ticket workspace is allocated (zeroed) under the arena

    def make():
        rng = np.random.default_rng(sum(shape) + 1)
        a = ORACLE.l2_normalize(np.maximum(rng.standard_normal(shape), 0).astype(np.float32) + 1e-3)
        b = ORACLE.l2_normalize(np.maximum(rng.standard_normal(shape), 0).astype(np.float32) + 1e-3)
        return [_np(v, dev) for v in (a, b, ORACLE.local_correlation_layer(b, a))]
    a, b, want = _once("in", make)
    ap, bp = arena.place(a), arena.place(b)
    with arena.allocations():
        first = correlation.local_correlation_layer(bp, ap)
        again = correlation.local_correlation_layer(bp, ap)         # the tickets are left zero by every call
    return {"out": (first, want, (1e-4, 1e-5)), "out_second_call": (again, want, (1e-4, 1e-5))}


@case("correlation/fp16_dispatch/corr_hot_c19_21x37", atomic=("grad1", "grad2"))
def _corr_half(arena):
    """test_ops_gpu.test_corr_half_dispatch: the fp64 oracle on the half-rounded operands, one half rounding (2^-10) of the range."""
    import numpy as np
    from conftest import golden
    from refign_amd import correlation
    dev = arena.device
    g = golden("corr_hot_c19_21x37")
    a = [int(v) for v in g["args"]]

    def make():
        kw = dict(kernel_size=(a[0], a[1]), patch_size=(a[2], a[3]), padding=(a[4], a[5]), dilation=(a[6], a[7]),
                  dilation_patch=(a[8], a[9]), stride=(a[10], a[11]))
        h = [_np(g[k].astype(np.float16), dev) for k in ("in1", "in2", "grad_out")]
        d1, d2, dg = (t.cpu().numpy().astype(np.float64) for t in h)
        w1, w2 = ORACLE.corr_backward(d1, d2, dg, **kw)
        return h + [_np(v, dev) for v in (ORACLE.corr_forward(d1, d2, **kw), w1, w2)]
    h1, h2, hg, want, w1, w2 = _once("in", make)
    p1, p2, pg = arena.place(h1), arena.place(h2), arena.place(hg)
    with arena.allocations():
        out = correlation.forward(p1, p2, *a)
        g1, g2 = correlation.backward(p1, p2, pg, *a)
    assert out.dtype == F16 and g1.dtype == F16 and g2.dtype == F16
    eps = 2.0 ** -10
    return {"out": (out, want, eps * max(float(want.abs().max()), 1e-3)),
            "grad1": (g1, w1, eps * max(float(w1.abs().max()), 1e-3)), "grad2": (g2, w2, eps * max(float(w2.abs().max()), 1e-3))}


@case("global_correlation/globalcorr_c24_5x7_6x4")
def _global_layer(arena):
    from conftest import golden
    from refign_amd.modules import GlobalFeatureCorrelationLayer
    dev = arena.device
    g = _once("in", lambda: {k: _np(v, dev) for k, v in golden("globalcorr_c24_5x7_6x4").items() if k in ("source", "target", "out")})
    sp, tp = arena.place(g["source"]), arena.place(g["target"])
    with arena.allocations():
        out = GlobalFeatureCorrelationLayer(cyclic_consistency=True)(sp, tp)
    return {"out": (out, g["out"], (2e-4, 2e-6))}


# =====================================================================================================================
# matching.warp forward / backward -- test_matcher_gpu.test_warp_backward_matches_grid_sample_autograd (1e-5 / 2e-5 relative to
# max(range, 1); flows that leave the image are part of the case; the backward scatters with float atomics: exempt), align_tail --
# test_ops_gpu.test_align_tail_vs_unfused (13 x 19 -> 52 x 76), l2_normalize_channels -- test_l2_normalize_channels and its
# channels-last 16-bit form (rtol 1e-6, atol 1e-7 against F.normalize).  No alignment stated: second placement 16 bytes.
# =====================================================================================================================
def _warp_case(B, C, H, W, amp):
    def fn(arena):
        from test_matcher_gpu import _grid_sample_warp
        from refign_amd.matching import warp
        dev = arena.device

        def make():
            g = torch.Generator().manual_seed(B * 100 + C)
            x = torch.randn(B, C, H, W, generator=g).to(dev)
            flo = (torch.randn(B, 2, H, W, generator=g) * amp).to(dev)
            go = torch.randn(B, C, H, W, generator=g).to(dev)
            x2, f2 = x.clone().requires_grad_(True), flo.clone().requires_grad_(True)
            y2 = _grid_sample_warp(x2, f2)
            y2.backward(go)
            return x, flo, go, y2.detach(), x2.grad, f2.grad
        x, flo, go, y2, dx, df = _once("in", make)
        xp, fp = arena.place(x).requires_grad_(True), arena.place(flo).requires_grad_(True)
        gp = arena.place(go)
        with arena.allocations():
            y = warp(xp, fp)
            y.backward(gp)
        return {"y": (y, y2, 1e-5 * max(float(y2.abs().max()), 1.0)),
                "grad_x": (xp.grad, dx, 2e-5 * max(float(dx.abs().max()), 1.0)),
                "grad_flow": (fp.grad, df, 2e-5 * max(float(df.abs().max()), 1.0))}
    return fn


for _s in ((2, 5, 17, 23, 3.0), (2, 2, 9, 1, 2.0)):
    case(f"warp/{'x'.join(str(int(v)) for v in _s)}", atomic=("grad_x", "grad_flow"))(_warp_case(*_s))


@case("align_tail/13x19_to_52x76")
def _align_tail(arena):
    import numpy as np
    from refign_amd.matching import align_tail
    dev = arena.device

    def make():
        rng = np.random.default_rng(3)
        B, H, W, h, w = 2, 52, 76, 13, 19
        logits = rng.standard_normal((B, 19, H, W)).astype(np.float32)
        fq = (4 * rng.standard_normal((B, 2, h, w))).astype(np.float32)
        lq = rng.uniform(-4, 4, (B, 1, h, w)).astype(np.float32)
        fu = F.interpolate(torch.from_numpy(fq), size=(H, W), mode="bilinear", align_corners=False).numpy()
        lu = F.interpolate(torch.from_numpy(lq), size=(H, W), mode="bilinear", align_corners=False).numpy()
        want_w, want_m = ORACLE.warp(logits, fu, return_mask=True)
        return [_np(v, dev) for v in (logits, fq, lq, fu, ORACLE.confidence_from_logvar(lu), want_w, want_m)]
    logits, fq, lq, fu, conf, want_w, want_m = _once("in", make)
    lp, fp, qp = arena.place(logits), arena.place(fq), arena.place(lq)
    with arena.allocations():
        warped, mask, cert, flow_up = align_tail(lp, fp, qp, return_flow=True)
    assert float((mask != want_m.to(mask.dtype)).float().mean()) < 1e-3    # only pixels within 1 ulp of the border may differ
    return {"flow_up": (flow_up, fu, (1e-5, 1e-5)), "certainty": (cert.reshape(conf.shape), conf, (1e-4, 1e-6)),
            "warped": (warped, want_w, (1e-4, 2e-4)), "mask": (mask, None, None)}


def _l2norm_case(B, C, H, W, dt):
    def fn(arena):
        from fill import hashed_uniform
        from refign_amd.matching import l2_normalize_channels
        dev = arena.device

        def make():
            tag = f"l2n/{B}/{C}/{H}/{W}" if dt == F32 else f"l2n16/{B}/{C}/{H}/{W}"
            x = (_np(hashed_uniform((B, C, H, W), tag), dev) * 4 - 2).to(dt)
            x[0, :, 0, 0] = 0
            if dt != F32:
                x = x.contiguous(memory_format=torch.channels_last)
            return x, F.normalize(x.float(), p=2, dim=1).contiguous()
        x, want = _once("in", make)
        xp = arena.place(x)
        with arena.allocations():
            got = l2_normalize_channels(xp)
        assert got.dtype == F32 and tuple(got.shape) == (B, C, H, W)
        assert float(got[0, :, 0, 0].abs().max()) == 0.0
        return {"y": (got, want, (1e-6, 1e-7))}
    return fn


for _dt in (F32, F16, BF16):
    for _s in ((2, 128, 7, 9), (3, 8, 5, 7)):
        case(f"l2_normalize_channels/{'x'.join(map(str, _s))}/{_DN[_dt]}")(_l2norm_case(*_s, _dt))


# =====================================================================================================================
# upcat.upsample_concat forward + backward (the gather kernel, RFN_UPCAT_BWD's default) -- test_seg_gpu.test_upsample_concat_fused_
# matches_interpolate_cat, first `sizes, chans` entry (allclose 1e-5 / 1e-5 in fp32, 2e-2 / 2e-2 in bf16); the fused up-sampling
# cross-entropy -- test_loss_gpu.test_fused_upsample_ce_matches_interpolate_then_cross_entropy at (2, 19, 9, 13, 36, 52), weighted,
# bf16 (loss to 1e-5 max(1, |loss|), gradient to 2^-7 of its range; loss and gradient are added with float atomics: exempt).
# No alignment stated: second placement 16 bytes.
# =====================================================================================================================
def _upcat_case(dt):
    sizes, chans, n = [(34, 60), (17, 30), (9, 15), (5, 8)], [32, 32, 32, 32], 3

    def fn(arena):
        from refign_amd.upcat import upsample_concat
        dev = arena.device
        H, W = max(s[0] for s in sizes), max(s[1] for s in sizes)

        def make():
            g = torch.Generator().manual_seed(len(sizes) * 7 + chans[0])
            toks = [torch.randn(n, h * w, c, generator=g).to(dev).to(dt) for (h, w), c in zip(sizes, chans)]
            refs = [t.clone().requires_grad_() for t in toks]
            parts = []
            for t, (h, w), c in zip(refs, sizes, chans):
                m = t.transpose(1, 2).reshape(n, c, h, w)
                parts.append(m if (h, w) == (H, W) else F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False))
            want = torch.cat(parts, 1)
            go = torch.randn(want.shape, generator=g).to(dev).to(dt)
            want.backward(go)
            return toks, go, want.detach(), [r.grad for r in refs]
        toks, go, want, grads = _once("in", make)
        tp = [arena.place(t).requires_grad_() for t in toks]
        gp = arena.place(go)
        with arena.allocations():
            got = upsample_concat(tp, sizes, (H, W))
            assert got.shape == want.shape and got.dtype == dt
            got.backward(gp)
        tol = (2e-2, 2e-2) if dt == BF16 else (1e-5, 1e-5)
        out = {"y": (got, want, tol)}
        out.update({f"grad{i}": (t.grad, g, tol) for i, (t, g) in enumerate(zip(tp, grads))})
        return out
    return fn


for _dt in (F32, BF16):
    case(f"upsample_concat/34x60_17x30_9x15_5x8/{_DN[_dt]}")(_upcat_case(_dt))


@case("upsample_ce/2x19x9x13_to_36x52/weighted/bf16", atomic=("grad", "loss"), det=True)
def _upsample_ce(arena):
    from test_loss_gpu import _reference
    from refign_amd import seg
    dev, (B, C, h, w, H, W) = arena.device, (2, 19, 9, 13, 36, 52)

    def make():
        g = torch.Generator().manual_seed(B * 100 + h + W)
        logits = (torch.randn(B, C, h, w, generator=g) * 3).to(dev).to(BF16)
        target = torch.randint(0, C, (B, H, W), generator=g).to(dev)
        target[torch.rand(B, H, W, generator=g).to(dev) < 0.2] = 255
        weight = torch.rand(B, H, W, generator=g).to(dev)
        want, want_grad = _reference(logits, (H, W), target, weight, 255)
        return logits, target, weight, want, want_grad
    logits, target, weight, want, want_grad = _once("in", make)
    lg = arena.place(logits).requires_grad_()
    tp, wp = arena.place(target), arena.place(weight)
    with arena.allocations():
        loss = seg.PixelWeightedCrossEntropyLoss(255)(seg.DeferredUpsample(lg, (H, W)), tp, pixel_weight=wp)
        (3.0 * loss).backward()
    assert loss.dtype == F32 and lg.grad.dtype == BF16
    return {"loss": (loss.detach(), want, 1e-5 * max(1.0, abs(float(want)))),
            "grad": (lg.grad.float() / 3.0, want_grad.float(), 2.0 ** -7 * float(want_grad.float().abs().max()))}


# =====================================================================================================================
# Halo-tiled 3 x 3 convolution (csrc/conv3x3.hip) -- test_conv3x3_gpu.test_halo_tiled_conv3x3_matches_fp32 at its smallest ragged
# entry (relative error of the range below 2e-3 in f16) and test_halo_tiled_conv3x3_fp32_result_of_split_products at
# (1, 67, 90, 96, 64) (below 2e-4).  The weights are plain tensors made per run, so their packed copies (params.derived, cached on
# the tensor object) are packed under the arena.  No alignment stated: second placement 16 bytes.
# =====================================================================================================================
@case("conv3x3_halo/2x37x61x64x64/f16_relu")
def _conv3x3(arena):
    from refign_amd import conv
    dev, (B, H, W, C, N) = arena.device, (2, 37, 61, 64, 64)

    def make():
        torch.manual_seed(H * W + C)
        x = torch.randn(B, C, H, W, device=dev).to(F16).contiguous(memory_format=torch.channels_last)
        w = torch.randn(N, C, 3, 3, device=dev) * (9 * C) ** -0.5
        bias = torch.randn(N, device=dev) * 0.1
        return x, w, bias, F.relu(F.conv2d(x.float(), w.to(F16).float(), bias.to(F16).float(), padding=1))
    x, w, bias, ref = _once("in", make)
    xp, wp, bp = arena.place(x), arena.place(w), arena.place(bias)
    with arena.allocations(), torch.no_grad():
        y = conv.conv2d_mfma(xp, wp, bp, 1, 1, 1, act="relu", dtype=F16)
    assert y is not None and tuple(y.shape) == (B, N, H, W)
    # (`err < 2e-3`: the largest double below the bound stands for the strict inequality)
    return {"y": (y, ref, math.nextafter(2e-3 * float(ref.abs().max()), 0.0))}


@case("conv3x3_halo/split_products/1x67x90x96x64")
def _conv3x3_split(arena):
    from refign_amd import split32
    dev, (B, H, W, C, N, act) = arena.device, (1, 67, 90, 96, 64, 3)

    def make():
        torch.manual_seed(C + N)
        x = torch.randn(B, C, H, W, device=dev)
        w = torch.randn(N, C, 3, 3, device=dev) * (9 * C) ** -0.5
        bias = torch.randn(N, device=dev) * 0.1
        return x[:, :C // 2].contiguous(), x[:, C // 2:].contiguous(), w, bias, F.leaky_relu(F.conv2d(x, w, bias, padding=1), 0.1)
    xa, xb, w, bias, ref = _once("in", make)
    pa, pb, wp, bp = (arena.place(t) for t in (xa, xb, w, bias))
    with arena.allocations(), torch.no_grad():
        y = split32.conv2d_parts([pa, pb], wp, bp, 1, 1, 1, act)
    assert y is not None and tuple(y.shape) == (B, N, H, W)
    return {"y": (y, ref, math.nextafter(2e-4 * float(ref.abs().max()), 0.0))}


# =====================================================================================================================
# fp32 attention (csrc/attn32.hip) -- test_split32_gpu.test_attention_fp32_kernel_matches_fp64 at its smallest ATTN entry
# (1, 2, 31, 5, 64): forward and the three gradients against fp64, 2e-5 of the range + 1e-7.  One query chunk: no atomics in dK / dV
# (only the backward with more than one query chunk adds with them).  Second placement 16 bytes: split32.attention tests
# data_ptr() % 16.
# =====================================================================================================================
@case("attention_fp32/1x2x31x5x64")
def _attn32(arena):
    from refign_amd import split32
    dev, (B, h, N, Nkv, D), scale = arena.device, (1, 2, 31, 5, 64), 0.125
    C = h * D

    def make():
        q, kv, go = _rand((B, N, C), dev, F32, 9), _rand((B, Nkv, 2 * C), dev, F32, 10), _rand((B, N, C), dev, F32, 12)
        qd, kvd = q.double().requires_grad_(True), kv.double().requires_grad_(True)
        k, v = kvd.view(B, Nkv, 2, h, D).permute(2, 0, 3, 1, 4).unbind(0)
        od = (torch.softmax(qd.view(B, N, h, D).transpose(1, 2) @ k.transpose(-1, -2) * scale, -1) @ v).transpose(1, 2).reshape(B, N, C)
        od.backward(go.double())
        return q, kv, go, od.detach(), qd.grad, kvd.grad
    q, kv, go, od, dq, dkv = _once("in", make)
    qp, kvp, gp = arena.place(q).requires_grad_(True), arena.place(kv).requires_grad_(True), arena.place(go)
    with arena.allocations():
        o = split32.attention(qp, kvp, h, scale)
        assert o is not None and tuple(o.shape) == (B, N, C)
        o.backward(gp)
    return {n: (got, want, 2e-5 * float(want.abs().max()) + 1e-7) for n, got, want in
            (("o", o, od), ("dq", qp.grad, dq), ("dkv", kvp.grad, dkv))}


# <<< further families are registered below this line >>>


@pytest.mark.parametrize("name", list(CASES))
def test_guardband(dev, oracle, name):
    global ORACLE
    ORACLE = oracle
    _drive(name)


# =====================================================================================================================
# The EMA kernel, directly: rfn_multi_ema_f32 through params.ema_update (dst16 = 0, all it ever passes) AND through the ABI with a
# hand-built table {ema*, live*, dst16*, n} that has dst16 set (the branch that is unreachable from Python).
# Reference: fp64 E a + L b_k with a = float32(m), b_k = float32(1) - a -- the kernel's documented arithmetic.
# Bound: 3 * 2^-24 (|E a| + |L b_k|): three fp32 roundings (two multiplies and an add; two with the contraction to an fma).  A CPU
# model of the kernel over 2^20 N(0, 1) pairs reaches 0.66 of it, separate multiplies and fma alike.
# Known deviation: the reference implementation and the non-GPU branch of ema_update multiply by
# float32(1 - m), the kernel by float32(1) - float32(m); for m = 0.999 these are 1.29e-5 apart relatively, so against torch's
# coefficient only the derived envelope bound + |L| |float32(1 - m) - b_k| is asserted.
# =====================================================================================================================
@pytest.mark.parametrize("skew", [0, 4])                           # 4: the kernel's scalar path
@pytest.mark.parametrize("momentum", [0.0, 0.5, 0.9, 0.999])       # 0.0: min(1 - 1 / (step + 1), ema_momentum) at step 0
def test_ema_kernel_directly(dev, momentum, skew):
    from refign_amd import _lib, params
    from refign_amd._tensor import ptr
    import numpy as np
    chunk = _lib.load_library().rfn_multi_cast_chunk_elems()
    E0, L0 = [], []
    for i, n in enumerate((1, 3, 4097, chunk + 5)):
        e, l_ = _rand((n,), dev, F32, 200 + i), _rand((n,), dev, F32, 210 + i)
        big = torch.arange(0, n, 97, device=dev)                   # a few elements with |live| > 100 |ema|
        l_[big] = 150.0 * e[big] + torch.sign(e[big]) * 1e-3
        assert bool((l_[big].abs() > 100 * e[big].abs()).all())
        E0.append(e), L0.append(l_)
    a = np.float32(momentum)
    b_k = np.float32(1.0) - a
    b_torch = np.float32(1.0 - momentum)
    results = {}
    for route in ("ema_update", "abi_dst16"):
        arena = GuardArena(dev, 0xFF, 8 * MiB, skew=skew)
        E, L = [arena.place(t) for t in E0], [arena.place(t) for t in L0]
        key = ("guardband", momentum, skew)
        try:
            with arena.allocations():
                if route == "ema_update":
                    params.ema_update(E, L, momentum, key)
                    D = None
                else:
                    D = [torch.empty(t.shape, dtype=BF16, device=dev) for t in E]
                    rows = []
                    for e, l_, d in zip(E, L, D):
                        n = e.numel()
                        rows += [(e.data_ptr() + 4 * off, l_.data_ptr() + 4 * off, d.data_ptr() + 2 * off, min(chunk, n - off))
                                 for off in range(0, n, chunk)]
            if route == "abi_dst16":
                table = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev)
                _lib.call("rfn_multi_ema_f32", dev, ptr(table), len(rows), float(momentum))
        finally:
            params.forget(key)
        arena.check()
        for i, (e, l_, e0, l0) in enumerate(zip(E, L, E0, L0)):
            assert torch.equal(l_, l0), "the live parameters are read only"
            ta, tb = e0.double() * float(a), l0.double() * float(b_k)
            bound = 3 * 2.0 ** -24 * (ta.abs() + tb.abs())
            err = (e.double() - (ta + tb)).abs()
            assert bool((err <= bound).all()), (route, i, float((err / bound.clamp_min(1e-300)).max()))
            # torch's coefficient float32(1 - m): the derived envelope only
            err_t = (e.double() - (ta + l0.double() * float(b_torch))).abs()
            assert bool((err_t <= bound + l0.double().abs() * abs(float(b_torch) - float(b_k))).all()), (route, i)
            if momentum == 0.0:
                assert torch.equal(e.view(torch.int32), l0.view(torch.int32))
            if D is not None:
                assert torch.equal(D[i].view(torch.int16), e.to(BF16).view(torch.int16)), (i, "dst16 != ema_after.to(bfloat16)")
        results[route] = [e.clone() for e in E]
    for x, y in zip(results["ema_update"], results["abi_dst16"]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "the dst16 branch may not change the fp32 result"

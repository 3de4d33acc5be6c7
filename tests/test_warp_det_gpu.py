"""GPU: the order-free backward of matching.warp (csrc/warp.hip rfn_warp_bwd_det_f32: 64-bit fixed-point sums for grad_x, stored
per-group partials for grad_flow) and the fp32 gather backward of the generic correlation (rfn_corr_bwd_gather_f32), both reached
through determinism.deterministic(scatter_forms=True).

The reference of the warp is an fp64 restatement on the CPU built from the SAME fp32 tap weights: the operations of the kernels'
warp_tap (csrc/bilinear.h, which also states the tap validity and `finite`), in its order, on fp32 CPU tensors (every one of them
an IEEE operation on both sides), then products and sums in fp64.  Bounds (include/refign_hip.h), per element:
  grad_x     |got - ref| <= 2^-22 S + 2^-30 M,  S = sum |g w| over the element's terms, M = the plane's largest |g|
             (2^-23 S: the fp32 product of every term and the final rounding; the quantisation is H W u / 2 <= M 2^(2 L - 62),
             below 2^-38 M at these sizes; the factor 2 absorbs a last-bit difference of a tap weight between host and device);
  grad_flow  |got - ref| <= 2^-22 sum |term|,   term = g (ne - nw) (1 - ty) and its three siblings.
"""
import numpy as np
import pytest
import torch
from conftest import golden

from guardband import FILLS, GuardArena

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 9, 1), (2, 5, 17, 23), (1, 33, 32, 40), (1, 70, 8, 8)]      # a one-pixel axis, ragged, two groups, three groups
AMPLITUDE = {(2, 2, 9, 1): 3.0, (2, 5, 17, 23): 3.0, (1, 33, 32, 40): 12.0, (1, 70, 8, 8): 30.0}
_MEMO = {}


# ---------------------------------------------------------------------------------------------------------------- helpers
def _taps(flow):
    """warp_tap (csrc/bilinear.h), its validity flags and its `finite`, on fp32 CPU tensors -> offsets (4, B, H, W) int64, validity (4, ...) bool,
    weights (4, ...) fp32 in the order nw, ne, sw, se, the fractions (tx, ty, ax, ay) and `finite`."""
    B, _, H, W = flow.shape
    f32 = torch.float32
    gx = torch.arange(W, dtype=f32).view(1, 1, W).expand(B, H, W)
    gy = torch.arange(H, dtype=f32).view(1, H, 1).expand(B, H, W)
    wm, hm = torch.tensor(float(max(W - 1, 1)), dtype=f32), torch.tensor(float(max(H - 1, 1)), dtype=f32)
    two, one = torch.tensor(2.0, dtype=f32), torch.tensor(1.0, dtype=f32)
    vx = two * (gx + flow[:, 0]) / wm - one
    vy = two * (gy + flow[:, 1]) / hm - one
    ix = ((vx + one) / two) * torch.tensor(float(W - 1), dtype=f32)
    iy = ((vy + one) / two) * torch.tensor(float(H - 1), dtype=f32)
    x0f, y0f = torch.floor(ix), torch.floor(iy)
    tx, ty = ix - x0f, iy - y0f
    ax, ay = one - tx, one - ty
    finite = (ix == ix) & (iy == iy) & (ix.abs() < 1e9) & (iy.abs() < 1e9)
    x0 = torch.where(finite, x0f, torch.full_like(x0f, -2.0)).long()
    y0 = torch.where(finite, y0f, torch.full_like(y0f, -2.0)).long()
    x1, y1 = x0 + 1, y0 + 1
    vx0, vx1, vy0, vy1 = (x0 >= 0) & (x0 < W), (x1 >= 0) & (x1 < W), (y0 >= 0) & (y0 < H), (y1 >= 0) & (y1 < H)
    cx0, cx1, cy0, cy1 = x0.clamp(0, W - 1), x1.clamp(0, W - 1), y0.clamp(0, H - 1), y1.clamp(0, H - 1)
    off = torch.stack((cy0 * W + cx0, cy0 * W + cx1, cy1 * W + cx0, cy1 * W + cx1))
    valid = torch.stack((vx0 & vy0, vx1 & vy0, vx0 & vy1, vx1 & vy1))
    w = torch.stack((ax * ay, tx * ay, ax * ty, tx * ty))
    assert w.dtype == f32
    return off, valid, torch.where(valid, w, torch.zeros_like(w)), (tx, ty, ax, ay), finite


def _reference(x, flow, go):
    """fp64 restatement -> grad_x, S (sum |g w| per element), grad_flow, sum |term| per element (all fp64, CPU)."""
    B, C, H, W = x.shape
    HW = H * W
    off, valid, w, (tx, ty, ax, ay), finite = _taps(flow)
    g = go.double().view(B, C, HW)
    gx_ref, S = torch.zeros(B, C, HW, dtype=torch.float64), torch.zeros(B, C, HW, dtype=torch.float64)
    for k in range(4):
        term = g * w[k].double().view(B, 1, HW)
        idx = off[k].view(B, 1, HW).expand(B, C, HW)
        gx_ref.scatter_add_(2, idx, term)
        S.scatter_add_(2, idx, term.abs())
    xs = x.double().view(B, C, HW)
    nw, ne, sw, se = (torch.where(valid[k].view(B, 1, HW), xs.gather(2, off[k].view(B, 1, HW).expand(B, C, HW)),
                                  torch.zeros((), dtype=torch.float64)) for k in range(4))
    txd, tyd, axd, ayd = (t.double().view(B, 1, HW) for t in (tx, ty, ax, ay))
    fx_terms = (g * (ne - nw) * ayd, g * (se - sw) * tyd)
    fy_terms = (g * (sw - nw) * axd, g * (se - ne) * txd)
    live_x = (finite.view(B, HW) & torch.tensor(W > 1)).double()
    live_y = (finite.view(B, HW) & torch.tensor(H > 1)).double()
    gf_ref = torch.stack(((fx_terms[0] + fx_terms[1]).sum(1) * live_x, (fy_terms[0] + fy_terms[1]).sum(1) * live_y), 1)
    gf_abs = torch.stack(((fx_terms[0].abs() + fx_terms[1].abs()).sum(1) * live_x,
                          (fy_terms[0].abs() + fy_terms[1].abs()).sum(1) * live_y), 1)
    return gx_ref.view(B, C, H, W), S.view(B, C, H, W), torch.nan_to_num(gf_ref).view(B, 2, H, W), \
        torch.nan_to_num(gf_abs).view(B, 2, H, W)


def _general_inputs(shape):
    """Gaussian features and grad_out, Gaussian flows of the shape's amplitude (CPU fp32), and their reference: made once."""
    key = ("general", shape)
    if key not in _MEMO:
        B, C, H, W = shape
        g = torch.Generator().manual_seed(B * 100 + C)
        x = torch.randn(B, C, H, W, generator=g)
        flo = torch.randn(B, 2, H, W, generator=g) * AMPLITUDE[shape]
        go = torch.randn(B, C, H, W, generator=g)
        _MEMO[key] = (x, flo, go, _reference(x, flo, go))
    return _MEMO[key]


def _det_entry(x, flo, go, want_x=True, want_f=True):
    """rfn_warp_bwd_det_f32 itself, with a workspace of exactly the size the library asks for."""
    from refign_amd import _lib
    from refign_amd._tensor import ptr
    B, C, H, W = x.shape
    nbytes = _lib.load_library().rfn_warp_bwd_det_workspace_bytes(B, C, H, W, int(want_x), int(want_f))
    G = -(-C // 32)
    assert nbytes == (8 * B * C * H * W + 4 * B * C if want_x else 0) + (8 * G * B * H * W if want_f and G > 1 else 0)
    ws = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=x.device)
    gx = torch.full_like(x, float("nan")) if want_x else None
    gf = torch.full_like(flo, float("nan")) if want_f else None
    _lib.call("rfn_warp_bwd_det_f32", x.device, ptr(x), ptr(flo), ptr(go), ptr(gx), ptr(gf), ptr(ws), B, C, H, W)
    return gx, gf


def _default_entry(x, flo, go):
    from refign_amd import _lib
    from refign_amd._tensor import ptr
    B, C, H, W = x.shape
    gx, gf = torch.empty_like(x), torch.empty_like(flo)
    _lib.call("rfn_warp_bwd_f32", x.device, ptr(x), ptr(flo), ptr(go), ptr(gx), ptr(gf), B, C, H, W)
    return gx, gf


def _check_grad_x(got, ref, S, go, what):
    M = go.abs().double().amax(dim=(2, 3), keepdim=True)
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -22 * S + 2.0 ** -30 * M
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: grad_x max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert bool((err <= bound).all()), (what, worst)


# ------------------------------------------------------------------------------------------------------- through autograd
@pytest.mark.parametrize("shape", SHAPES)
def test_warp_backward_runs_in_widened_mode_and_refuses_in_plain_mode(dev, shape):
    """Inside deterministic(scatter_forms=True) warp(x, flo).backward(go) gives both gradients (the test that fails without the
    feature); inside plain deterministic() the same call raises the message it always raised."""
    from refign_amd import determinism
    from refign_amd.matching import warp
    x, flo, go, (gx_ref, S, gf_ref, gf_abs) = _general_inputs(shape)
    x1, f1 = x.to(dev).requires_grad_(True), flo.to(dev).requires_grad_(True)
    with determinism.deterministic(scatter_forms=True):
        assert determinism.enabled() and determinism.scatter_forms()
        warp(x1, f1).backward(go.to(dev))
    assert not determinism.enabled() and not determinism.scatter_forms()
    assert x1.grad is not None and f1.grad is not None
    _check_grad_x(x1.grad, gx_ref, S, go, f"autograd {shape}")
    assert bool(((f1.grad.double().cpu() - gf_ref).abs() <= 2.0 ** -22 * gf_abs).all())
    x2, f2 = x.to(dev).requires_grad_(True), flo.to(dev).requires_grad_(True)
    with determinism.deterministic():
        assert not determinism.scatter_forms()
        with pytest.raises(RuntimeError, match="rfn_warp_bwd_f32 refused in deterministic mode: warp_bwd_kernel"):
            warp(x2, f2).backward(go.to(dev))


# -------------------------------------------------------------------------------------------------------------- the entry
def _exact_inputs(shape):
    """grad_out and features of small integers; flows of an integer in [-2, 2] plus a fraction in {0, 0.25, 0.5, 0.75}, so every
    pixel's taps overlap its neighbours' and rows / columns at the border reach outside.  The kernel does not use x + flow as it
    stands but sends it through the normalised coordinate and back (2 v / (W - 1) - 1, then (v + 1) / 2 (W - 1)); where that round
    trip does not return a quarter exactly (W - 1 not a power of two) the pixel draws again, and after eight draws it is sent
    far outside the image instead (no taps).  Every tap weight is then a multiple of 1/16 and every term and partial sum exact."""
    key = ("exact", shape)
    if key not in _MEMO:
        B, C, H, W = shape
        g = torch.Generator().manual_seed(7 * B + C)

        def draw():
            return (torch.randint(-2, 3, (B, 2, H, W), generator=g) + torch.randint(0, 4, (B, 2, H, W), generator=g) / 4.0).float()

        def inexact(f):
            tx, ty, _, _ = _taps(f)[3]
            return ((tx * 4 != torch.floor(tx * 4)) | (ty * 4 != torch.floor(ty * 4))).unsqueeze(1).expand_as(f)

        flo = draw()
        for _ in range(8):
            flo = torch.where(inexact(flo), draw(), flo)
        flo = torch.where(inexact(flo), torch.full_like(flo, 4.0 * max(H, W) + 0.5), flo)
        off, valid, w, _, _ = _taps(flo)
        assert bool((w * 16 == torch.floor(w * 16)).all())
        assert float(valid.any(0).float().mean()) > 0.5, "most pixels must keep a tap inside the image"
        x = torch.randint(-3, 4, (B, C, H, W), generator=g).float()
        go = torch.randint(-4, 5, (B, C, H, W), generator=g).float()
        _MEMO[key] = (x, flo, go, _reference(x, flo, go))
    return _MEMO[key]


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_case_is_bit_equal_to_the_atomic_form_and_to_fp64(dev, shape):
    x, flo, go, (gx_ref, _, gf_ref, _) = _exact_inputs(shape)
    xd, fd, gd = x.to(dev), flo.to(dev), go.to(dev)
    gx, gf = _det_entry(xd, fd, gd)
    gx0, gf0 = _default_entry(xd, fd, gd)
    assert torch.equal(gx.view(torch.int32), gx0.view(torch.int32)), "grad_x differs from rfn_warp_bwd_f32"
    assert torch.equal(gx.cpu().view(torch.int32), (gx_ref.float() + 0.0).view(torch.int32)), "grad_x differs from fp64"
    assert torch.equal(gf.cpu(), gf_ref.float()), "grad_flow differs from fp64"
    if shape[1] <= 32:
        assert torch.equal(gf.view(torch.int32), gf0.view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES)
def test_general_case_within_the_rounding_bound(dev, shape):
    x, flo, go, (gx_ref, S, gf_ref, gf_abs) = _general_inputs(shape)
    xd, fd, gd = x.to(dev), flo.to(dev), go.to(dev)
    gx, gf = _det_entry(xd, fd, gd)
    _check_grad_x(gx, gx_ref, S, go, f"general {shape}")
    err = (gf.double().cpu() - gf_ref).abs()
    print(f"general {shape}: grad_flow max err {float(err.max()):.3e}, worst err / bound "
          f"{float((err / (2.0 ** -22 * gf_abs).clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= 2.0 ** -22 * gf_abs).all())
    if shape[1] <= 32:                                     # the single-group store path: the bits of rfn_warp_bwd_f32
        assert torch.equal(gf.view(torch.int32), _default_entry(xd, fd, gd)[1].view(torch.int32))
    # either output alone (the head's feature warps want grad_flow only; the other pointer is NULL) and a second call
    assert torch.equal(_det_entry(xd, fd, gd, want_x=False)[1].view(torch.int32), gf.view(torch.int32))
    assert torch.equal(_det_entry(xd, fd, gd, want_f=False)[0].view(torch.int32), gx.view(torch.int32))
    gx2, gf2 = _det_entry(xd, fd, gd)
    assert torch.equal(gx2.view(torch.int32), gx.view(torch.int32)) and torch.equal(gf2.view(torch.int32), gf.view(torch.int32))


def _odd_flow_inputs(C):
    """(1, C, 5, 7) exact inputs whose first pixels carry the flows on which a guard of the int conversion decides: NaN, the
    infinities, +-2e9 (beyond int32), +-1e5 (finite, far outside), W + 0.5 and -1.5, in either component; quarter-pixel flows
    elsewhere (drawn as in _exact_inputs, so every surviving tap weight is a multiple of 1/16).  -> x, flow, grad_out, the
    reference, and the mask of the pixels that are non-finite or far."""
    key = ("odd", C)
    if key not in _MEMO:
        B, H, W = 1, 5, 7
        x, flo, go, _ = _exact_inputs((B, C, H, W))
        nan, inf = float("nan"), float("inf")
        odd = [(nan, None), (None, nan), (nan, nan), (inf, None), (None, -inf), (-inf, inf), (2e9, None), (None, -2e9), (-2e9, 2e9),
               (1e5, None), (None, -1e5), (-1e5, 1e5), (W + 0.5, None), (None, H + 0.5), (-1.5, None), (None, -1.5), (None, -1.5)]
        flo = flo.clone()
        # (None: the component keeps its exact draw.  -1.5 along x is pixel 14 = column 0: both taps outside)
        for p, (fx, fy) in enumerate(odd):
            for c, f in enumerate((fx, fy)):
                if f is not None:
                    flo[0, c, p // W, p % W] = f
        _, valid, w, _, finite = _taps(flo)
        assert bool((w * 16 == torch.floor(w * 16)).all()) and bool(valid.any(0)[0, 2, 1:3].all())    # (the two -1.5 rows keep taps)
        far = ~finite | (flo.abs() >= 1e5).any(1)
        assert int(far.sum()) == 12 and not bool(valid[:, far].any())
        _MEMO[key] = (x, flo, go, _reference(x, flo, go), far)
    return _MEMO[key]


@pytest.mark.parametrize("C", [3, 40])                      # one channel group, two
def test_non_finite_and_far_flows(dev, C):
    """The tap validity (warp_tap, csrc/bilinear.h) where the conversion to int is guarded: both forms of the backward drop every
    tap of such a pixel, give it no flow gradient, and agree with the fp64 reference bit for bit."""
    x, flo, go, (gx_ref, _, gf_ref, _), far = _odd_flow_inputs(C)
    xd, fd, gd = x.to(dev), flo.to(dev), go.to(dev)
    want = (gx_ref.float() + 0.0).view(torch.int32)
    for name, (gx, gf) in (("rfn_warp_bwd_det_f32", _det_entry(xd, fd, gd)), ("rfn_warp_bwd_f32", _default_entry(xd, fd, gd))):
        gf = gf.cpu()
        assert bool((gf[:, 0][far] == 0).all()) and bool((gf[:, 1][far] == 0).all()), f"{name}: flow gradient at a far pixel"
        assert torch.equal(gx.cpu().view(torch.int32), want), f"{name}: grad_x differs from fp64"
        assert torch.equal(gf, gf_ref.float()), f"{name}: grad_flow differs from fp64"


def test_collision_case_repeats_its_bits(dev):
    """Every pixel of a 32 x 40 map lands in one 2 x 2 neighbourhood: H W adds per destination, in whatever order they arrive."""
    B, C, H, W = 1, 2, 32, 40
    g = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    frac = torch.rand(B, 2, H, W, generator=g) * 0.98 + 0.01
    flo = torch.stack((17.0 + frac[:, 0] - xx, 9.0 + frac[:, 1] - yy), 1)
    x, go = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    off = _taps(flo)[0]
    assert len(torch.unique(off)) == 4
    gx_ref, S, gf_ref, gf_abs = _reference(x, flo, go)
    xd, fd, gd = x.to(dev), flo.to(dev), go.to(dev)
    runs = [_det_entry(xd, fd, gd) for _ in range(5)]
    for gx, gf in runs[1:]:
        assert torch.equal(gx.view(torch.int32), runs[0][0].view(torch.int32))
        assert torch.equal(gf.view(torch.int32), runs[0][1].view(torch.int32))
    _check_grad_x(runs[0][0], gx_ref, S, go, "collision")
    assert int((runs[0][0] != 0).sum()) == 4 * B * C


def test_non_finite_grad_out_marks_its_plane(dev):
    shape = (2, 5, 17, 23)
    x, flo, go, _ = _general_inputs(shape)
    xd, fd = x.to(dev), flo.to(dev)
    clean = _det_entry(xd, fd, go.to(dev))[0]
    bad = go.clone()
    bad[1, 3, 5, 7] = float("inf")
    gx = _det_entry(xd, fd, bad.to(dev))[0]
    assert bool(torch.isnan(gx[1, 3]).all())
    keep = torch.ones(2, 5, dtype=torch.bool)
    keep[1, 3] = False
    assert torch.equal(gx[keep.to(dev)].view(torch.int32), clean[keep.to(dev)].view(torch.int32))
    zero = go.clone()
    zero[0, 2] = 0.0                                       # a plane of zeros: written as zeros, not left as the workspace was
    assert bool((_det_entry(xd, fd, zero.to(dev))[0][0, 2] == 0).all())


@pytest.mark.parametrize("shape", [(2, 5, 17, 23), (1, 70, 8, 8)])
def test_guard_band(dev, shape):
    """Operands, outputs and the workspace out of a poisoned arena: nothing outside them is written, and the bits do not depend
    on what the memory held before."""
    from refign_amd import _tensor, determinism
    from refign_amd.matching import warp
    x, flo, go, (gx_ref, S, _, _) = _general_inputs(shape)
    saved = dict(_tensor._WS)
    bits = None
    try:
        for fill in FILLS:
            _tensor._WS.clear()                             # the per-stream scratch is allocated again, inside the arena
            arena = GuardArena(dev, fill, 24 << 20, skew=16)
            xa, fa = arena.place(x.to(dev)).requires_grad_(True), arena.place(flo.to(dev)).requires_grad_(True)
            ga = arena.place(go.to(dev))
            with arena.allocations(), determinism.deterministic(scatter_forms=True):
                warp(xa, fa).backward(ga)
            arena.check()
            assert any(label.startswith("empty") and b - a >= 1 << 22 for a, b, label in arena.ranges), "workspace not in the arena"
            got = (xa.grad.view(torch.int32).clone(), fa.grad.view(torch.int32).clone())
            _check_grad_x(xa.grad, gx_ref, S, go, f"guard band {shape} fill {fill:#x}")
            if bits is None:
                bits = got
            assert torch.equal(got[0], bits[0]) and torch.equal(got[1], bits[1]), f"fill {fill:#x} changed the result"
    finally:
        _tensor._WS.clear()
        _tensor._WS.update(saved)


# -------------------------------------------------------------------------------------------------------- the correlation
def test_corr_gather_f32_matches_golden_and_repeats(dev):
    from refign_amd import _lib, correlation, determinism
    from refign_amd._tensor import ptr
    g = golden("corr_gen_k3_p5_s2")
    assert g["in1"].dtype == np.float32
    a = [int(v) for v in g["args"]]
    in1, in2, go = (torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in ("in1", "in2", "grad_out"))
    B, C, iH, iW = in1.shape
    outs = []
    for _ in range(2):
        g1, g2 = torch.full_like(in1, float("nan")), torch.full_like(in2, float("nan"))
        _lib.call("rfn_corr_bwd_gather_f32", dev, ptr(in1), ptr(in2), ptr(go), ptr(g1), ptr(g2), B, C, iH, iW, *a)
        outs.append((g1, g2))
    np.testing.assert_allclose(outs[0][0].cpu().numpy(), g["grad_in1"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(outs[0][1].cpu().numpy(), g["grad_in2"], rtol=1e-4, atol=1e-4)
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    # the wrapper: the gather form in the widened mode, the unchanged refusal in the plain mode
    with determinism.deterministic(scatter_forms=True):
        w1, w2 = correlation.backward(in1, in2, go, *a)
    assert torch.equal(w1.view(torch.int32), outs[0][0].view(torch.int32)) and torch.equal(w2.view(torch.int32), outs[0][1].view(torch.int32))
    with determinism.deterministic():
        with pytest.raises(RuntimeError, match="rfn_corr_bwd refused in deterministic mode: corr_generic_bwd_kernel"):
            correlation.backward(in1, in2, go, *a)

"""GPU: the depthwise 3x3 backward in one pass over grad_y (csrc/dwconv.hip dwconv3x3_bwd_kernel, rfn_dwconv3x3_nhwc_bwd):
grad_x and grad_weight / grad_bias against F.conv2d's autograd in float64 on the same (already rounded) inputs, in fp32,
bf16 and fp16; `flags`; bit-reproducibility; the weight-gradient-only route; both autograd functions."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]

# (B, H, W, C, dilation): the smallest shapes at which the kernel can go wrong
SHAPES = [
    (1, 1, 1, 8, 1),          # every tap but the centre is outside
    (1, 5, 3, 8, 1),          # W shorter than a quad
    (2, 7, 9, 40, 1),         # channel vectors that do not fill the block, W % 4 == 1
    (1, 3, 5, 1280, 1),       # sliced grid with 16 idle threads per block
    (2, 9, 13, 1024, 6),      # sliced, dilated, H % dilation != 0
    (1, 4, 11, 64, 6),        # every vertical tap outside
    (3, 5, 4, 2048, 18),      # large dilation on a small map
    # the launch code's size switches.  Channel blocks x block rows: the block rows stop at the 128 rows of the workspace
    # (32 pixel lanes per block at C = 128: 3 960 quads = 124 rows, one quad per thread; 8 100 quads = 128 rows, threads
    # walk several quads) ...
    (1, 44, 360, 128, 1), (1, 90, 360, 128, 1),
    # ... and the sliced grid stops at 64 block rows (8 pixel lanes per block at C = 1024: 184 / 726 slots)
    (1, 23, 31, 1024, 1), (2, 33, 41, 1024, 1),
]
SOME = [(2, 7, 9, 40, 1), (2, 9, 13, 1024, 6), (3, 5, 4, 2048, 18)]


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """Inputs (rounded to `dtype`, on the CPU) and the float64 reference gradients of F.conv2d on them; shared, never modified."""
    B, H, W, C, dil = shape
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W + C + dil)
    x = torch.randn(B, H, W, C, generator=g).to(dtype)
    gy = torch.randn(B, H, W, C, generator=g).to(dtype)
    w = 0.3 * torch.randn(C, 1, 3, 3, generator=g)
    xr = x.double().permute(0, 3, 1, 2).requires_grad_()
    wr = w.double().requires_grad_()
    br = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wr, br, padding=dil, dilation=dil, groups=C).backward(gy.double().permute(0, 3, 1, 2))
    return x, gy, w, xr.grad.permute(0, 2, 3, 1).contiguous(), wr.grad, br.grad


def _tap_major(w):
    return w.float().reshape(w.shape[0], 9).t().contiguous()


def _bwd(x, gy, w_tap, dil, want_gx=True, flags=0, dw=None, db=None):
    """rfn_dwconv3x3_nhwc_bwd (want_gx) or rfn_dwconv3x3_nhwc_bwd_weight straight through the ABI"""
    from refign_amd import _lib
    from refign_amd._tensor import DTYPE_CODE, ptr
    B, H, W, C = x.shape
    lib = _lib.load_library()
    ws = torch.empty(lib.rfn_dwconv3x3_bwd_weight_workspace_bytes(C), dtype=torch.uint8, device=x.device)
    if dw is None:
        dw = torch.full((9, C), float("nan"), device=x.device)
        db = torch.full((C,), float("nan"), device=x.device)
    tail = (ptr(dw), ptr(db), ptr(ws), B, H, W, C, dil, DTYPE_CODE[x.dtype], flags)
    if want_gx:
        gx = torch.full_like(x, float("nan"))
        _lib.call("rfn_dwconv3x3_nhwc_bwd", x.device, ptr(x), ptr(gy), ptr(w_tap), ptr(gx), *tail)
    else:
        gx = None
        _lib.call("rfn_dwconv3x3_nhwc_bwd_weight", x.device, ptr(x), ptr(gy), *tail)
    return gx, dw, db


def _tols(dtype, npix):
    if dtype == torch.float32:
        return dict(rtol=1e-4, atol=1e-4), dict(rtol=1e-3, atol=1e-3 * npix ** 0.5)
    return dict(rtol=2e-2, atol=2e-2), dict(rtol=2e-2, atol=2e-2 * npix ** 0.5)


def _on(dev, shape, dtype):
    x, gy, w, gx_ref, gw_ref, gb_ref = _case(shape, dtype)
    return x.to(dev), gy.to(dev), _tap_major(w).to(dev), gx_ref.to(dev), gw_ref.to(dev), gb_ref.to(dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_backward_matches_conv2d_autograd(dev, shape, dtype):
    B, H, W, C, dil = shape
    x, gy, w_tap, gx_ref, gw_ref, gb_ref = _on(dev, shape, dtype)
    gx, dw, db = _bwd(x, gy, w_tap, shape[4])
    tol, wtol = _tols(dtype, B * H * W)
    gw = dw.t().reshape(C, 1, 3, 3).double()
    print(f"{shape} {dtype}: max |gx - ref| = {float((gx.double() - gx_ref).abs().max()):.3e}, "
          f"|gw - ref| = {float((gw - gw_ref).abs().max()):.3e}, |gb - ref| = {float((db.double() - gb_ref).abs().max()):.3e}")
    assert gx.dtype == dtype
    assert torch.allclose(gx.double(), gx_ref, **tol)
    assert torch.allclose(gw, gw_ref, **wtol)
    assert torch.allclose(db.double(), gb_ref, **wtol)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", SOME, ids=lambda s: "x".join(map(str, s)))
def test_flags_accumulate_into_parameter_layout(dev, shape, dtype):
    """flags = 3: grad_weight in the parameter's (C, 1, 3, 3) layout, and both ADDED to what the buffers held"""
    B, H, W, C, dil = shape
    x, gy, w_tap, gx_ref, gw_ref, gb_ref = _on(dev, shape, dtype)
    g = torch.Generator().manual_seed(7)
    pre_w, pre_b = torch.randn(C, 1, 3, 3, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    gx0, dw0, db0 = _bwd(x, gy, w_tap, shape[4])                                   # fresh, tap-major
    gx, dw, db = _bwd(x, gy, w_tap, dil, flags=3, dw=pre_w.clone(), db=pre_b.clone())
    tol, wtol = _tols(dtype, B * H * W)
    assert torch.equal(gx, gx0)
    assert torch.allclose(gx.double(), gx_ref, **tol)
    # one fp32 addition apart from the fresh result ...
    assert torch.equal(dw, pre_w + dw0.t().reshape(C, 1, 3, 3))
    assert torch.equal(db, pre_b + db0)
    # ... and the gradient itself is the reference's
    assert torch.allclose((dw - pre_w).double(), gw_ref, **wtol)
    assert torch.allclose((db - pre_b).double(), gb_ref, **wtol)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", SOME, ids=lambda s: "x".join(map(str, s)))
def test_two_calls_are_bit_identical_and_the_weight_only_route_gives_the_same_bits(dev, shape, dtype):
    x, gy, w_tap, *_ = _on(dev, shape, dtype)
    gx1, dw1, db1 = _bwd(x, gy, w_tap, shape[4])
    gx2, dw2, db2 = _bwd(x, gy, w_tap, shape[4])
    assert torch.equal(gx1, gx2) and torch.equal(dw1, dw2) and torch.equal(db1, db2)
    # GX = false (no input gradient wanted): the same launch geometry, the same sums in the same order
    _, dw3, db3 = _bwd(x, gy, w_tap, shape[4], want_gx=False)
    assert torch.equal(dw1, dw3) and torch.equal(db1, db3)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_autograd_routes_give_the_gradients_of_the_torch_formulation(dev, dtype):
    """dwconv3x3_nhwc and dwconv3x3_gelu_tokens(with_z=True) with input AND parameter gradients wanted (the fused launch),
    and with a constant input (the weight-gradient-only route)"""
    from refign_amd.dwconv import dwconv3x3_gelu_tokens, dwconv3x3_nhwc
    B, H, W, C = 2, 9, 13, 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, C, generator=g).to(dtype)
    gy = torch.randn(B, H, W, C, generator=g).to(dtype)
    w0 = 0.3 * torch.randn(C, 1, 3, 3, generator=g)
    b0 = 0.1 * torch.randn(C, generator=g)
    xr = x.double().permute(0, 3, 1, 2).requires_grad_()
    wr, br = w0.double().requires_grad_(), b0.double().requires_grad_()
    F.conv2d(xr, wr, br, padding=1, groups=C).backward(gy.double().permute(0, 3, 1, 2))
    gx_ref, gw_ref, gb_ref = xr.grad.permute(0, 2, 3, 1).to(dev), wr.grad.to(dev), br.grad.to(dev)
    x, gy, w0, b0 = x.to(dev), gy.to(dev), w0.to(dev), b0.to(dev)
    tol, wtol = _tols(dtype, B * H * W)

    def check(xa, w, b, with_gx):
        if with_gx:
            assert torch.allclose(xa.grad.double(), gx_ref, **tol)
        else:
            assert xa.grad is None
        assert torch.allclose(w.grad.double(), gw_ref, **wtol)
        assert torch.allclose(b.grad.double(), gb_ref, **wtol)

    for with_gx in (True, False):
        xa = x.clone().requires_grad_(with_gx)
        w, b = w0.clone().requires_grad_(), b0.clone().requires_grad_()
        dwconv3x3_nhwc(xa, w, b, 1).backward(gy)
        check(xa, w, b, with_gx)
        # the Mix-FFN form: `a` is non-differentiable, the gradient arrives on the pre-activation z
        xa = x.clone().requires_grad_(with_gx)
        w, b = w0.clone().requires_grad_(), b0.clone().requires_grad_()
        a, z = dwconv3x3_gelu_tokens(xa.reshape(B, H * W, C), w, b, H, W, with_z=True)
        assert not a.requires_grad
        z.backward(gy.reshape(B, H * W, C))
        check(xa, w, b, with_gx)

"""Depthwise 3x3 convolution on channels-last / token layout, forward and backward in HIP (csrc/dwconv.hip).

`dwconv3x3_tokens(x, weight, bias, H, W)` is the DWConv of the Mix-FFN (mix_transformer.py:556-568) WITHOUT the two
NCHW transposes of the reference: x is (B, N=H*W, C) and stays that way.  `dwconv3x3_nhwc(x, weight, bias, dilation)`
is the same on (B, H, W, C) maps with dilation (DAFormer ASPP branches, daformer.py:46-62).  `weight` is the reference
parameter itself, shape (C, 1, 3, 3); activations float32, bfloat16 or float16, accumulation fp32, weight grads fp32.
"""
import os

import torch

from . import _lib, determinism
from ._tensor import DTYPE_CODE, ptr, require_device_tensor, workspace
from .params import as_dtype, grad_sink, tap_major_f32 as _tap_major

_DW_WS_STRIPES = 128       # kMaxStripes in csrc/dwconv.hip (checked against the ABI in the GPU tests)


def _f32(p):
    """fp32 contiguous view of a bias / affine parameter (None stays None)"""
    return None if p is None else as_dtype(p, torch.float32).detach().contiguous()


def _fwd(x, w_tap, bias, dilation, flip, stats=None):
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    lib = _lib.load_library()
    if stats is not None and determinism.enabled():         # ... as per-block partial rows + an ordered column sum
        ws = workspace(lib.rfn_dwconv3x3_stats_det_workspace_bytes(B, H, W, C, dilation), x.device)
        _lib.call("rfn_dwconv3x3_nhwc_fwd_stats_det", x.device, ptr(x), ptr(w_tap), ptr(bias), ptr(y), ptr(stats), ptr(ws), B,
                  H, W, C, dilation, DTYPE_CODE[x.dtype])
        return y
    if stats is not None:                                   # + the BatchNorm statistics of the result (csrc/dwconv.hip STATS)
        _lib.call("rfn_dwconv3x3_nhwc_fwd_stats", x.device, ptr(x), ptr(w_tap), ptr(bias), ptr(y), ptr(stats), B, H, W, C,
                  dilation, DTYPE_CODE[x.dtype])
        return y
    _lib.call("rfn_dwconv3x3_nhwc_fwd", x.device, ptr(x), ptr(w_tap), ptr(bias), ptr(y), B, H, W, C, dilation, DTYPE_CODE[x.dtype],
              1 if flip else 0)
    return y


class _DWConv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, dilation, stats=None):
        if x.dtype not in DTYPE_CODE:
            x = x.float()
        x = require_device_tensor(x.contiguous(), "x")
        w_tap, b32 = _tap_major(weight), _f32(bias)
        ctx.save_for_backward(x, w_tap)
        ctx.dilation, ctx.has_bias = dilation, bias is not None
        ctx.wshape, ctx.wdtype = weight.shape, weight.dtype
        ctx.weight, ctx.bias = weight, bias
        return _fwd(x, w_tap, b32, dilation, False, stats)

    @staticmethod
    def backward(ctx, gy):
        x, w_tap = ctx.saved_tensors
        return _dwconv_backward(ctx, x, w_tap, gy.to(x.dtype).contiguous()) + (None,)


class _DWConv3x3Gelu(torch.autograd.Function):
    """gelu(dwconv3x3(x)) in one kernel; the backward is GELU' (on the saved pre-activation) followed by the backward
    of the plain convolution."""

    @staticmethod
    def forward(ctx, x, weight, bias, with_z=False):
        if x.dtype not in DTYPE_CODE:
            x = x.float()
        x = require_device_tensor(x.contiguous(), "x")
        B, H, W, C = x.shape
        w_tap, b32 = _tap_major(weight), _f32(bias)
        need = any(ctx.needs_input_grad)
        with_z = with_z and need
        ctx.set_materialize_grads(False)          # the non-differentiable output's "gradient" must not become a zero tensor
        z = torch.empty_like(x) if need else None
        a = torch.empty_like(x)
        _lib.call("rfn_dwconv3x3_gelu_nhwc_fwd", x.device, ptr(x), ptr(w_tap), ptr(b32), ptr(z), ptr(a), B, H, W, C,
                  DTYPE_CODE[x.dtype])
        if need:
            ctx.save_for_backward(x, w_tap, z)
            ctx.has_bias, ctx.wshape, ctx.wdtype = bias is not None, weight.shape, weight.dtype
            ctx.weight, ctx.bias, ctx.dilation = weight, bias, 1
        if with_z:
            # (a, z): the activation as a NON-differentiable tensor + the pre-activation that carries the gradient -- the
            # consumer (linear._LinearFn with z=) returns d/dz directly, gelu' applied in its input-gradient GEMM's epilogue
            ctx.mark_non_differentiable(a)
            ctx.with_z = True
            return a, z
        ctx.with_z = False
        return a

    @staticmethod
    def backward(ctx, *grads):
        x, w_tap, z = ctx.saved_tensors
        if ctx.with_z:
            if grads[1] is None:
                return None, None, None, None
            gz = grads[1].to(z.dtype).contiguous()
        else:
            gz = torch.ops.aten.gelu_backward(grads[0].to(z.dtype).contiguous(), z)
        return _dwconv_backward(ctx, x, w_tap, gz)[:3] + (None,)


def _dwconv_backward(ctx, x, w_tap, gy):
    B, H, W, C = x.shape
    gx = gw = gb = None
    need_params = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
    if ctx.needs_input_grad[0] and not need_params:
        gx = _fwd(gy, w_tap, None, ctx.dilation, True)
    if need_params:
        sw, sb = grad_sink(ctx.weight), grad_sink(ctx.bias) if ctx.has_bias else None
        direct = sw is not None and (sb is not None or not ctx.has_bias)
        if direct:
            dw, db = sw, sb
        else:
            dw = torch.empty((9, C), dtype=torch.float32, device=x.device)
            db = torch.empty((C,), dtype=torch.float32, device=x.device) if ctx.has_bias else None
        ws = workspace(_DW_WS_STRIPES * 10 * C * 4, x.device)            # per stream: looked up on the stream it runs on
        tail = (ptr(dw), ptr(db), ptr(ws), B, H, W, C, ctx.dilation, DTYPE_CODE[x.dtype], 3 if direct else 0)
        if ctx.needs_input_grad[0]:                                      # both gradients from one pass over gy
            gx = torch.empty_like(x)
            _lib.call("rfn_dwconv3x3_nhwc_bwd", x.device, ptr(x), ptr(gy), ptr(w_tap), ptr(gx), *tail)
        else:
            _lib.call("rfn_dwconv3x3_nhwc_bwd_weight", x.device, ptr(x), ptr(gy), *tail)
        if not direct:
            gw = dw.t().reshape(ctx.wshape).to(ctx.wdtype)
            gb = db
    return gx, gw, gb, None


def dwconv3x3_gelu_tokens(x, weight, bias, H, W, with_z=False):
    """gelu(DWConv(x)) on tokens (B, N=H*W, C) -> (B, N, C): mix_transformer.py:99-101 in one pass.  with_z (under autograd):
    -> (a, z), a non-differentiable, z the pre-activation carrying the gradient (see _DWConv3x3Gelu); (a, None) otherwise."""
    B, N, C = x.shape
    out = _DWConv3x3Gelu.apply(x.reshape(B, H, W, C), weight, bias, with_z)
    if isinstance(out, tuple):
        return out[0].reshape(B, N, C), out[1].reshape(B, N, C)
    return (out.reshape(B, N, C), None) if with_z else out.reshape(B, N, C)


FUSED_FFN = os.environ.get("RFN_FUSED_FFN", "1") != "0"      # (tests flip the attribute; the variable is for A/B runs of bench.py)


@torch.no_grad()
def ffn_fc1_dw_gelu(x, fc1, dw, H, W):
    """gelu(dw(fc1(x))) of a Mix-FFN (mix_transformer.py:99-101) on gradient-free bf16 / fp16 tokens (views, H*W, C) in ONE kernel
    (csrc/mixffn.hip): the 4C-wide pre-activation never reaches HBM.  `fc1`: the Linear, `dw`: the depthwise nn.Conv2d.  None
    outside the kernel's domain (the caller runs fc1, then dwconv3x3_gelu_tokens)."""
    B, N, C = x.shape
    HID = fc1.weight.shape[0]
    if not (FUSED_FFN and x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and x.is_contiguous() and N == H * W and C % 64 == 0
            and HID % 128 == 0 and fc1.bias is not None and dw.bias is not None and dw.weight.shape == (HID, 1, 3, 3)
            and dw.padding == (1, 1) and dw.stride == (1, 1) and dw.dilation == (1, 1)):
        return None
    w1, b1 = as_dtype(fc1.weight, x.dtype), as_dtype(fc1.bias, x.dtype)
    w_tap, bdw = _tap_major(dw.weight), _f32(dw.bias)
    a = torch.empty((B, N, HID), dtype=x.dtype, device=x.device)
    _lib.call("rfn_ffn_fc1_dw_gelu_f16" if x.dtype == torch.float16 else "rfn_ffn_fc1_dw_gelu_bf16", x.device, ptr(x), ptr(w1),
              ptr(b1), ptr(w_tap), ptr(bdw), ptr(a), B, H, W, C, HID)
    return a


def dwconv3x3_nhwc(x, weight, bias=None, dilation=1, stats=None):
    """x: (B,H,W,C) fp32/bf16; weight: (C,1,3,3); bias: (C) or None; same-size output (padding = dilation).
    `stats` (bf16 / fp16 x, C % 8 == 0): a float64 tensor of 2 C + 1 elements that receives the BatchNorm statistics of the result
    (sum, sum of squares, rows: the buffer of bn._stats_fwd)."""
    if x.dim() != 4 or weight.shape[0] != x.shape[-1]:
        raise RuntimeError("dwconv3x3_nhwc: x must be (B,H,W,C) and weight (C,1,3,3)")
    if stats is not None and not (x.dtype in (torch.bfloat16, torch.float16) and x.shape[-1] % 8 == 0 and stats.dtype == torch.float64
                                  and stats.is_contiguous() and stats.numel() == 2 * x.shape[-1] + 1):
        raise RuntimeError("dwconv3x3_nhwc(stats=...): bf16 / fp16 input with C % 8 == 0 and a float64 buffer of 2 C + 1 elements")
    return _DWConv3x3.apply(x, weight, bias, int(dilation), stats)


def _stats_only(x, w_tap, b32, dilation):
    """(sum, sum of squares, rows) of the rounded convolution result, nothing stored: 2 C + 1 doubles"""
    B, H, W, C = x.shape
    sums = torch.empty(2 * C + 1, dtype=torch.float64, device=x.device)
    if determinism.enabled():
        ws = workspace(_lib.load_library().rfn_dwconv3x3_stats_det_workspace_bytes(B, H, W, C, dilation), x.device)
        _lib.call("rfn_dwconv3x3_nhwc_stats_det", x.device, ptr(x), ptr(w_tap), ptr(b32), ptr(sums), ptr(ws), B, H, W, C,
                  dilation, DTYPE_CODE[x.dtype])
    else:
        _lib.call("rfn_dwconv3x3_nhwc_stats", x.device, ptr(x), ptr(w_tap), ptr(b32), ptr(sums), B, H, W, C, dilation,
                  DTYPE_CODE[x.dtype])
    return sums


@torch.no_grad()
def dwconv3x3_stats_nhwc(x, weight, bias, dilation):
    """The first pass of dwconv3x3_bn_act_nhwc alone: the BatchNorm statistics of dwconv3x3_nhwc(x, weight, bias, dilation)
    (a float64 tensor of 2 C + 1: sum, sum of squares, rows) without storing the convolution.  x: (B, H, W, C) bf16 / fp16."""
    return _stats_only(x, _tap_major(weight), _f32(bias), int(dilation))


@torch.no_grad()
def dwconv3x3_bn_act_nhwc(x, weight, bias, dilation, bn, relu):
    """act(bn(dwconv3x3(x))) with BATCH statistics, gradient-free (the EMA teacher's ASPP branches run their BatchNorms in
    training mode; daformer.py:10-62): two passes over x -- statistics of the convolution result without storing
    it, then convolution + normalisation + ReLU -- instead of convolution, statistics pass and BatchNorm pass over the
    result.  x: (B, H, W, C) bf16 / fp16 contiguous; bn: the (Sync)BatchNorm2d module (running buffers updated as in training)."""
    from . import bn as bnk
    B, H, W, C = x.shape
    w_tap, b32, g, be = _tap_major(weight), _f32(bias), _f32(bn.weight), _f32(bn.bias)
    y = torch.empty_like(x)
    sums = _stats_only(x, w_tap, b32, int(dilation))
    group = bnk.sync_group(bn)
    if group is not None:
        bnk._all_reduce(sums, group, bnk._exchange_comm(bn))
    _lib.call("rfn_dwconv3x3_bn_act_nhwc_fwd", x.device, ptr(x), ptr(w_tap), ptr(b32), ptr(g), ptr(be), ptr(sums),
              ptr(bn.running_mean), ptr(bn.running_var), ptr(y), B, H, W, C, int(dilation), float(bn.eps), float(bn.momentum),
              1 if relu else 0, DTYPE_CODE[x.dtype])
    bn.num_batches_tracked.add_(1)
    return y


def dwconv3x3_tokens(x, weight, bias, H, W):
    """x: (B, N=H*W, C) tokens -> (B, N, C)."""
    B, N, C = x.shape
    return dwconv3x3_nhwc(x.reshape(B, H, W, C), weight, bias, 1).reshape(B, N, C)

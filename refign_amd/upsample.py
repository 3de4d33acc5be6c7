"""Bilinear up-sampling whose backward is reproducible.

`interpolate_bilinear(x, size=..., scale_factor=...)` is `F.interpolate(x, ..., mode='bilinear', align_corners=False)`.
ATen's backward of that op scatters every output gradient into its four source cells with floating-point atomics
(`upsample_bilinear2d_backward` raises under `torch.use_deterministic_algorithms(True)`).  In deterministic mode
(refign_amd/determinism.py) a HIP tensor that wants a gradient takes an autograd Function instead: the forward is ATen's own,
the backward the gather kernel of csrc/det.hip (one thread per input cell adds the output pixels that read it, in raster
order).  Everything else -- the default mode, gradient-free calls, down-sampling -- is the plain F.interpolate call.
"""
import math

import torch
import torch.nn.functional as F

from . import _lib, determinism
from ._tensor import DTYPE_CODE, ptr


def bilinear2d_backward(grad_out, in_size, scales=(0.0, 0.0)):
    """Gradient of the (N, C, h, w) input of a bilinear up-sampling (align_corners=False) for the gradient `grad_out`
    (N, C, H, W) of its result.  `scales`: ATen's source-index scales (1 / scale_factor) when the forward was given a scale
    factor, 0 for h / H, w / W."""
    if not (grad_out.is_cuda and grad_out.dim() == 4 and grad_out.dtype in DTYPE_CODE):
        raise RuntimeError("bilinear2d_backward: a 4-d fp32 / bf16 / fp16 HIP tensor expected")
    g = grad_out.contiguous()
    N, C, H, W = g.shape
    h, w = int(in_size[0]), int(in_size[1])
    gin = torch.empty((N, C, h, w), dtype=g.dtype, device=g.device)
    _lib.call("rfn_upsample_bilinear2d_bwd", g.device, ptr(g), ptr(gin), N * C, h, w, H, W, float(scales[0]), float(scales[1]),
              DTYPE_CODE[g.dtype])
    return gin


class _UpBilinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, scale_factor):
        # ATen's kernel itself, as F.interpolate calls it outside torch's deterministic switch (under the switch F.interpolate
        # takes an index-based decomposition instead: other launches, other rounding than the default mode's forward)
        ctx.in_size = h, w = x.shape[2:]
        if scale_factor is None:
            ctx.scales, out, sf = (0.0, 0.0), size, None
        else:
            sf = float(scale_factor)
            ctx.scales, out = (1.0 / sf,) * 2, (int(math.floor(h * sf)), int(math.floor(w * sf)))
        return torch._C._nn.upsample_bilinear2d(x, out, False, sf, sf)

    @staticmethod
    def backward(ctx, g):
        return bilinear2d_backward(g, ctx.in_size, ctx.scales), None, None


def interpolate_bilinear(x, size=None, scale_factor=None):
    if determinism.enabled() and x.is_cuda and x.dim() == 4 and x.dtype in DTYPE_CODE and torch.is_grad_enabled() and x.requires_grad:
        up = (scale_factor is not None and float(scale_factor) >= 1.0) or \
            (size is not None and size[0] >= x.shape[2] and size[1] >= x.shape[3])
        if up:
            return _UpBilinearFn.apply(x, None if size is None else (int(size[0]), int(size[1])), scale_factor)
    return F.interpolate(x, size=size, scale_factor=scale_factor, mode='bilinear', align_corners=False)

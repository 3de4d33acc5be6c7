"""The multi-level flow loss of matcher training as ONE autograd node (csrc/flowloss.hip): every pyramid level of one
`MultiScaleFlowLoss.forward` call -- ground-truth resize, robust end-point term, Gaussian negative log-likelihood, masked
mean, weighted sum -- in one forward launch plus a finalize launch, and one backward launch.  No host decision: a level
without a valid pixel contributes 0 (and zero gradients) on the device, where the torch formulation asks the host.  No
floating-point atomics: the same inputs give the same bits.

`losses.MultiScaleFlowLoss` routes here for fp32 CUDA inputs with downsample_gt_flow=True (losses.FUSED_LEVEL_LOSS)."""
import numpy as np
import torch

from . import _lib
from ._tensor import ptr

LOSS_CODES = {"L1Loss": 0, "L2Loss": 1, "HuberLoss": 2}
MAX_LEVELS = 8


def eligible(levels, gt_flow, masks):
    """fp32 CUDA tensors on one device, at most MAX_LEVELS levels of (flow (B,2,h,w), log-variance (B,1|2,h,w) or None),
    masks bool tensors or None per level (of any size: losses._level_mask brings them to the level's afterwards)."""
    if not (torch.is_tensor(gt_flow) and gt_flow.is_cuda and gt_flow.dtype == torch.float32 and gt_flow.dim() == 4
            and gt_flow.shape[1] == 2 and 0 < len(levels) <= MAX_LEVELS):
        return False
    dev, B = gt_flow.device, gt_flow.shape[0]
    for (flow, lv), mask in zip(levels, masks):
        if not (flow.device == dev and flow.dtype == torch.float32 and flow.dim() == 4 and flow.shape[0] == B
                and flow.shape[1] == 2):
            return False
        if lv is not None and not (lv.device == dev and lv.dtype == torch.float32 and lv.shape[1] in (1, 2)
                                   and lv.shape[0] == B and lv.shape[-2:] == flow.shape[-2:]):
            return False
        if mask is not None and not (mask.device == dev and mask.dtype == torch.bool and mask.shape[0] == B):
            return False
    return True


def _table(flows, lvs, masks, gflows, glvs):
    rows = [(ptr(f) or 0, ptr(lv) or 0, ptr(m) or 0, ptr(gf) or 0, ptr(gl) or 0, f.shape[-2], f.shape[-1],
             0 if lv is None else lv.shape[1]) for f, lv, m, gf, gl in zip(flows, lvs, masks, gflows, glvs)]
    return np.asarray(rows, dtype=np.int64)


class _FlowLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, gt_flow, *tensors):
        weights, loss_code, delta = meta
        n = len(weights)
        flows = [t.contiguous() for t in tensors[:n]]
        lvs = [None if t is None else t.contiguous() for t in tensors[n:2 * n]]
        masks = [None if t is None else t.contiguous().view(torch.uint8) for t in tensors[2 * n:]]
        gt_flow = gt_flow.contiguous()
        dev = gt_flow.device
        B, _, H, W = gt_flow.shape
        per_block = _lib.load_library().rfn_flowloss_block_pixels()
        nblocks = sum(-(-B * f.shape[-2] * f.shape[-1] // per_block) for f in flows)
        partials = torch.empty(2 * nblocks, dtype=torch.float64, device=dev)
        out = torch.empty(1 + n, dtype=torch.float32, device=dev)
        counts = torch.empty(n, dtype=torch.float64, device=dev)
        table = _table(flows, lvs, masks, [None] * n, [None] * n)
        w = np.asarray(weights, dtype=np.float64)
        _lib.call("rfn_flowloss_fwd_f32", dev, ptr(gt_flow), B, H, W, table.ctypes.data, w.ctypes.data, n, loss_code, delta,
                  ptr(partials), nblocks, ptr(out), ptr(counts))
        ctx.meta, ctx.n = meta, n
        ctx.has_lv, ctx.has_mask = [lv is not None for lv in lvs], [m is not None for m in masks]
        ctx.save_for_backward(gt_flow, counts, *flows, *[lv for lv in lvs if lv is not None],
                              *[m for m in masks if m is not None])
        total, per_level = out[0], out[1:]
        ctx.mark_non_differentiable(per_level)
        return total, per_level

    @staticmethod
    def backward(ctx, grad_total, _grad_levels):
        weights, loss_code, delta = ctx.meta
        n = ctx.n
        gt_flow, counts, *rest = ctx.saved_tensors
        flows, rest = rest[:n], list(rest[n:])
        lvs = [rest.pop(0) if has else None for has in ctx.has_lv]
        masks = [rest.pop(0) if has else None for has in ctx.has_mask]
        need = ctx.needs_input_grad[2:]
        gflows = [torch.empty_like(f) if need[i] else None for i, f in enumerate(flows)]
        glvs = [torch.empty_like(lv) if lv is not None and need[n + i] else None for i, lv in enumerate(lvs)]
        dev = gt_flow.device
        B, _, H, W = gt_flow.shape
        grad_total = grad_total.to(torch.float32).contiguous()
        table = _table(flows, lvs, masks, gflows, glvs)
        w = np.asarray(weights, dtype=np.float64)
        _lib.call("rfn_flowloss_bwd_f32", dev, ptr(gt_flow), B, H, W, table.ctypes.data, w.ctypes.data, n, loss_code, delta,
                  ptr(counts), ptr(grad_total))
        return (None, None, *gflows, *glvs, *([None] * n))


def multi_level_flow_loss(levels, gt_flow, masks, weights, loss_type, delta=1.0, return_levels=False):
    """levels: [(flow, log-variance or None)], coarsest first as MultiScaleFlowLoss takes them; gt_flow (B,2,H,W) at full
    resolution; masks: per level None or a bool tensor of B*h*w elements ALREADY at the level's size (losses._level_mask);
    weights: one float per level.  -> the weighted sum of the levels' masked means (fp32 scalar), and with return_levels the
    (n,) tensor of those means (no gradient flows through it)."""
    flows = [f for f, _ in levels]
    lvs = [lv for _, lv in levels]
    for f, m in zip(flows, masks):
        if m is not None and m.numel() != f.shape[0] * f.shape[-2] * f.shape[-1]:
            raise RuntimeError(f"multi_level_flow_loss: a mask of {tuple(m.shape)} for a level of {tuple(f.shape)}")
    meta = (tuple(float(w) for w in weights), LOSS_CODES[loss_type], float(delta))
    total, per_level = _FlowLossFn.apply(meta, gt_flow, *flows, *lvs, *masks)
    return (total, per_level) if return_levels else total

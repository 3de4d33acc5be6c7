"""The HRDA logit merge at the end of the decode head (seg.hrda_head, models/hrda.py:139-235) on the kernels of csrc/hrdatail.hip.

`merge_slide(a, lr_seg, hr_seg, boxes)`: teacher / eval, gradient-free --
    up2(sigmoid(a)) * (sum of the sliding crops / their count) + up2((1 - sigmoid(a)) * lr_seg)
`fuse_crop(a, lr_seg, hr_seg, box, head_os)`: the student's one random crop, offset as device data (seg.DeviceBox), forward and
backward in one autograd Function --
    up2(att) * box.insert(hr_seg) + up2((1 - att) * lr_seg),   att = sigmoid(a) * box.mask
`a` are the scale-attention logits BEFORE the sigmoid.  Both return None outside the kernels' domain (the caller then runs the
element-wise chain); inside it the forward result is that chain's bit for bit: fp32, NCHW-shaped with channels-last strides.
"""
import ctypes

import torch

from . import _lib
from ._tensor import DTYPE_CODE, ptr

_L4 = ctypes.c_long * 4


def _strides(t):
    return _L4(*t.stride())


def usable(a, lr_seg, hr_seg):
    """HIP bf16 tensors under autocast, (n, K, h, w) / (., K, hc, wc): the step's precision.  There the chain keeps its element-wise
    steps in bf16 and up-samples, multiplies and adds in fp32 (F.interpolate is on autocast's fp32 list), which the kernels
    reproduce bit for bit.  Everything else stays on the chain: outside autocast it returns 16-bit logits, and with fp32 (or
    fp16's longer mantissas) the blend's fma choice shows in the last bit."""
    return (a.is_cuda and lr_seg.is_cuda and hr_seg.is_cuda and a.dim() == 4 and hr_seg.dim() == 4 and a.shape == lr_seg.shape
            and hr_seg.shape[1] == a.shape[1] and a.dtype == lr_seg.dtype == hr_seg.dtype == torch.bfloat16
            and torch.is_autocast_enabled())


def merge_slide(a, lr_seg, hr_seg, boxes):
    """boxes: the sliding crops' [y1, y2, x1, x2] on the (2h, 2w) grid (seg.scale_box by head_os), hr_seg crop-major as
    seg.extract_slide_crop stacks them.  None when the entry point declines (see include/refign_hip.h)."""
    nl, K, h, w = lr_seg.shape
    nb = len(boxes)
    if nb == 0 or hr_seg.shape[0] != nb * nl or not usable(a, lr_seg, hr_seg) or \
            (torch.is_grad_enabled() and (a.requires_grad or lr_seg.requires_grad or hr_seg.requires_grad)):
        return None
    hc, wc = hr_seg.shape[2:]
    out = torch.empty((nl, 2 * h, 2 * w, K), dtype=torch.float32, device=a.device)
    accepted = ctypes.c_int(0)
    flat = (ctypes.c_int * (4 * nb))(*[int(v) for b in boxes for v in b])
    _lib.call("rfn_hrda_merge_slide", a.device, ptr(a), _strides(a), ptr(lr_seg), _strides(lr_seg), ptr(hr_seg), _strides(hr_seg),
              flat, nb, ptr(out), nl, K, h, w, hc, wc, DTYPE_CODE[a.dtype], ctypes.byref(accepted))
    return out.permute(0, 3, 1, 2) if accepted.value else None


class _FuseCrop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, lr_seg, hr_seg, off, geom):
        n, K, h, w = lr_seg.shape
        hc, wc = hr_seg.shape[2:]
        out = torch.empty((n, 2 * h, 2 * w, K), dtype=torch.float32, device=a.device)
        _lib.call("rfn_hrda_fuse_crop_fwd", a.device, ptr(a), _strides(a), ptr(lr_seg), _strides(lr_seg), ptr(hr_seg),
                  _strides(hr_seg), ptr(off), ptr(out), n, K, h, w, hc, wc, *geom, DTYPE_CODE[a.dtype])
        ctx.save_for_backward(a, lr_seg, hr_seg, off)
        ctx.geom = geom
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        a, lr_seg, hr_seg, off = ctx.saved_tensors
        n, K, h, w = lr_seg.shape
        hc, wc = hr_seg.shape[2:]
        if g.dtype != torch.float32:
            g = g.float()
        g_a = torch.empty((n, h, w, K), dtype=a.dtype, device=a.device)
        g_lr = torch.empty((n, h, w, K), dtype=a.dtype, device=a.device)
        g_hr = torch.empty((n, hc, wc, K), dtype=a.dtype, device=a.device)
        _lib.call("rfn_hrda_fuse_crop_bwd", a.device, ptr(g), _strides(g), ptr(a), _strides(a), ptr(lr_seg), _strides(lr_seg),
                  ptr(hr_seg), _strides(hr_seg), ptr(off), ptr(g_a), ptr(g_lr), ptr(g_hr), n, K, h, w, hc, wc, *ctx.geom,
                  DTYPE_CODE[a.dtype])
        return g_a.permute(0, 3, 1, 2), g_lr.permute(0, 3, 1, 2), g_hr.permute(0, 3, 1, 2), None, None


def fuse_crop(a, lr_seg, hr_seg, box, head_os):
    """box: seg.DeviceBox (offset int64 (oy, ox) on the device, multiples of 2 * head_os; (h, w) of the crop in image pixels)."""
    os_ = int(head_os)
    if not (usable(a, lr_seg, hr_seg) and hr_seg.shape[0] == a.shape[0] and os_ == head_os and box.off.is_cuda
            and box.off.dtype == torch.long and box.off.numel() == 2 and box.off.is_contiguous() and box.divisible % (2 * os_) == 0):
        return None
    geom = (int(box.h / (2.0 * os_)), int(box.w / (2.0 * os_)), 2 * os_, os_)      # mask rows / columns, the two box scales
    return _FuseCrop.apply(a, lr_seg, hr_seg, box.off, geom)

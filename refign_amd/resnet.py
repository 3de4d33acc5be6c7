"""The DeepLabV2 family of the reference (configs/*/refign_deeplabv2.yaml): ResNet-v1c backbone and DeepLabV2Head, with
the reference's constructor keywords and state_dict keys.  Opt-in: config.build_model(cfg, families=("deeplabv2",)).

  models/backbones/resnet.py   ResNet(model_type, pretrained, ..., strides, dilations, out_indices, ...)
  models/heads/deeplabv2.py    DeepLabV2Head(in_channels, in_index, num_classes, ..., dilation_series, padding_series)

Execution of the backbone, all on kernels the package already has:
  * a 16-bit pass on the GPU with BatchNorm in training mode (student and EMA teacher, whose BatchNorm layers the reference
    leaves in training mode): every convolution through conv.Conv2d (implicit-GEMM kernels: conv2d_mfma_grad under autograd,
    conv2d_mfma without), every BatchNorm (+ ReLU) through bn.bn_act_train where bn.usable says so; the residual add + ReLU
    behind the last BatchNorm of a block is one ATen add and one ATen ReLU;
  * a gradient-free pass with BatchNorm in eval mode (the ImageNet encoder of the feature distance, validation): BatchNorm
    folded into the convolution weights (cached per block, dropped by train() / load_state_dict() / .to()), one launch of
    rfn_conv2d_nhwc per convolution with the ReLU in its epilogue.  The kernel adds `res` AFTER the activation
    (csrc/mfma_gemm.hip: y = res + act(acc + bias)), so the last convolution of a block takes the identity as `res` with no
    activation and the block's ReLU stays a separate element-wise op: a bottleneck is three launches plus that ReLU;
  * everything else takes the torch path: CPU tensors, BatchNorm in eval mode under autograd, and fp32 tensors on the GPU.
    The fp32 mode of this backbone is the library's fp32 convolution and torch's BatchNorm, because split-bf16 products
    (refign_amd/split32.py) are not accurate enough for 33 batch-normalised blocks (`unit`, FP32_LIBRARY).  GPU library
    calls are recorded by mfma.note_library (convolutions inside conv.Conv2d and in `unit`, BatchNorm in `unit`).
The max-pool is F.max_pool2d.

The head is sum_r Conv2d(C -> classes, 3x3, dilation d_r, padding p_r).  On the GPU in a 16-bit pass with p_r == d_r it runs
as a tap-GEMM plus a shifted sum (csrc/aspp.hip; `_fused`): one GEMM over the stacked live taps, one gather that writes the
logits once, and in the backward one gather and two GEMMs.  ASPP_FUSED = False (RFN_ASPP_FUSED=0) or anything outside that
domain: one conv.Conv2d per branch.

Data parallelism: the backbone holds BatchNorm layers, so under bn.data_parallel() it does not replay from the collective-free
graph segments of uda._backbone_segments (`has_batchnorm`); more than one rank has not been run for this family.
"""
import ctypes
import os
from typing import List, Optional, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import bn as bnk
from . import mfma as _mfma
from ._tensor import DTYPE_CODE16, ptr, workspace
from .align import BaseHead
from .config import OutOfScopeError
from .conv import ACT_CODE, Conv2d, _nhwc16
from .params import bias_stack, compute_dtype, grad_sink, sum_rows, tap_stack

ARCH = {"resnet18_v1c": ("basic", (2, 2, 2, 2)), "resnet50_v1c": ("bottleneck", (3, 4, 6, 3)),
        "resnet101_v1c": ("bottleneck", (3, 4, 23, 3))}
# file names of the ImageNet checkpoints the reference downloads (open-mmlab third_party); looked up locally only
IMAGENET_FILES = {"resnet18_v1c": "resnet18_v1c-b5776b93.pth", "resnet50_v1c": "resnet50_v1c-2cccc1ad.pth",
                  "resnet101_v1c": "resnet101_v1c-e67eebb6.pth"}
FP32_LIBRARY = True       # fp32 GPU passes of the backbone on the library's fp32 convolution (False: conv.Conv2d's split-bf16 products)


# ---------------------------------------------------------------------------------------------------------------------
# convolution + BatchNorm (+ ReLU) (+ residual), the unit every block is made of
# ---------------------------------------------------------------------------------------------------------------------
class _Folding(nn.Module):
    """A module whose (convolution, BatchNorm) pairs can run folded: the folded weights are cached per pair and dropped by the
    three hooks layers.ConvBNReLU uses (train(), _load_from_state_dict(), _apply())."""

    def __init__(self):
        super().__init__()
        self._folded = {}

    def folded(self, name, conv, bn, dtype):
        """(packed weight, bias) of rfn_conv2d_nhwc for conv with eval-mode bn folded in, in `dtype`.  Kept here and nowhere
        else: the folded tensors are no parameters, so they get no params.derived entry (and no refresh plan is disturbed)."""
        got = self._folded.get((name, dtype))
        if got is None:
            w, b = bnk.fold(conv.weight, conv.bias, bn)
            got = self._folded[(name, dtype)] = (_mfma.pack_conv_weight(w, dtype), b.to(dtype))
        return got

    def train(self, mode=True):
        self._folded = {}
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self._folded = {}
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *a, **k):
        self._folded = {}
        return super()._apply(fn, *a, **k)

    def unit(self, name, x, conv, bn, relu, res=None):
        """relu?(bn(conv(x))) [+ res, no ReLU after it: the caller's].  `res` is only taken on the folded path; elsewhere the
        caller adds it (returns (y, res_added))."""
        if x.is_cuda:
            cd = compute_dtype(x)
            if cd in DTYPE_CODE16 and not bn.training and not torch.is_grad_enabled():
                y = _conv_folded(x, self, name, conv, bn, cd, relu, res)
                if y is not None:
                    return y, res is not None
        if FP32_LIBRARY and x.is_cuda and x.dtype == torch.float32 and compute_dtype(x) == torch.float32:
            # fp32 passes: the library's fp32 convolution, not conv.Conv2d's split-bf16 products.  Their 2^-16 per product, carried
            # through 33 batch-normalised blocks, left the reference step's BatchNorm gradient norm 3.7 % off (bound 2 %); the
            # library's fp32 result is 0.3-0.5 % off (both rows: profiles/deeplabv2_parity.txt)
            _mfma.note_library("conv2d.autograd" if torch.is_grad_enabled() else "conv2d", x, conv.weight)
            y = conv._conv_forward(x, conv.weight, conv.bias)
        else:
            y = conv(x)
        return bnk.bn_act(y, bn, 'relu' if relu else None, note=True), False


def _conv_folded(x, owner, name, conv, bn, dtype, relu, res):
    """One launch of rfn_conv2d_nhwc: folded weight and bias, ReLU in the epilogue, `res` (NCHW-shaped, any strides) added
    after it.  None outside the kernel's domain."""
    s, p, d = conv.stride, conv.padding, conv.dilation
    N, C, KH, KW = conv.weight.shape
    if not (_mfma.ENABLED and conv.groups == 1 and s[0] == s[1] and p[0] == p[1] and d[0] == d[1] and N % 8 == 0
            and not isinstance(p, str)):
        return None
    wp, bp = owner.folded(name, conv, bn, dtype)
    xh = _nhwc16(x, dtype, -(-C // 8) * 8)
    rh = None if res is None else _nhwc16(res, dtype, res.shape[1])
    y = _mfma.conv2d_nhwc(xh, wp, bp, KH, KW, s[0], p[0], d[0], act=ACT_CODE['relu' if relu else None], res=rh)
    return None if y is None else y.permute(0, 3, 1, 2)


class BasicBlock(_Folding):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch'):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride, self.dilation, self.out_channels = stride, dilation, planes

    last_bn = "bn2"

    def forward(self, x):
        identity = x
        if self.downsample is not None:
            identity, _ = self.unit("down", x, self.downsample[0], self.downsample[1], False)
        out, _ = self.unit("1", x, self.conv1, self.bn1, True)
        out, added = self.unit("2", out, self.conv2, self.bn2, False, res=identity)
        if not added:
            out = out + identity
        return F.relu(out, inplace=True)


class Bottleneck(_Folding):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch'):
        super().__init__()
        if style not in ('pytorch', 'caffe'):
            raise ValueError(f"style {style!r}: 'pytorch' (stride on the 3x3) or 'caffe' (stride on the first 1x1)")
        s1, s2 = (1, stride) if style == 'pytorch' else (stride, 1)
        self.bn1 = nn.BatchNorm2d(planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.conv1 = Conv2d(inplanes, planes, 1, stride=s1, bias=False)
        self.conv2 = Conv2d(planes, planes, 3, stride=s2, padding=dilation, dilation=dilation, bias=False)
        self.conv3 = Conv2d(planes, planes * 4, 1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride, self.dilation, self.style, self.out_channels = stride, dilation, style, planes * 4

    last_bn = "bn3"

    def forward(self, x):
        identity = x
        if self.downsample is not None:
            identity, _ = self.unit("down", x, self.downsample[0], self.downsample[1], False)
        out, _ = self.unit("1", x, self.conv1, self.bn1, True)
        out, _ = self.unit("2", out, self.conv2, self.bn2, True)
        out, added = self.unit("3", out, self.conv3, self.bn3, False, res=identity)
        if not added:
            out = out + identity
        return F.relu(out, inplace=True)


_BLOCKS = {"basic": BasicBlock, "bottleneck": Bottleneck}


def _res_layer(block, num_blocks, in_channels, out_channels, stride, dilation, style, contract_dilation):
    """One stage: the first block carries the stride, the 1x1 / stride projection of the identity where the shape changes and,
    with contract_dilation, half the stage's dilation; the others run at stride 1 with the stage's dilation."""
    downsample = None
    if stride != 1 or in_channels != out_channels * block.expansion:
        downsample = nn.Sequential(Conv2d(in_channels, out_channels * block.expansion, 1, stride=stride, bias=False),
                                   nn.BatchNorm2d(out_channels * block.expansion))
    first = dilation // 2 if (dilation > 1 and contract_dilation) else dilation
    layers = [block(in_channels, out_channels, stride=stride, dilation=first, downsample=downsample, style=style)]
    layers += [block(out_channels * block.expansion, out_channels, stride=1, dilation=dilation, style=style)
               for _ in range(1, num_blocks)]
    return nn.Sequential(*layers)


class _Stem(_Folding):
    """(conv, bn, relu) x 3 under the reference's keys stem.{0,1,3,4,6,7} (its nn.Sequential), run unit by unit."""

    def __init__(self, *mods):
        super().__init__()
        for i, m in enumerate(mods):
            self.add_module(str(i), m)

    def forward(self, x):
        for i in (0, 3, 6):
            x, _ = self.unit(str(i), x, self._modules[str(i)], self._modules[str(i + 1)], True)
        return x


class ResNet(nn.Module):
    """models/backbones/resnet.py:106-385 (ResNet-v1c: three 3x3 convolutions in the stem, stride convolution in the identity
    projection)."""
    has_batchnorm = True          # uda._backbone_segments: not collective-free under SyncBatchNorm

    def __init__(self, model_type: str, pretrained: Optional[str] = None, channels_last: Optional[int] = None, in_channels=3,
                 stem_channels=64, base_channels=64, num_stages=4, strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1),
                 out_indices=(0, 1, 2, 3), style='pytorch', frozen_stages=-1, norm_eval=False, with_cp=False,
                 zero_init_residual=True, contract_dilation=False, max_pool_ceil_mode=False):
        super().__init__()
        if model_type not in ARCH:
            raise ValueError(f"model_type {model_type!r}: one of {sorted(ARCH)}")
        if with_cp:
            raise OutOfScopeError("ResNet(with_cp=True): activation checkpointing is out of scope of refign_amd (no config sets it)")
        if channels_last:
            raise OutOfScopeError("ResNet(channels_last=...): out of scope of refign_amd (the kernels keep channels-last memory "
                                  "between layers themselves; no config sets it)")
        if not (1 <= num_stages <= 4 and len(strides) == len(dilations) == num_stages and max(out_indices) < num_stages):
            raise ValueError("ResNet: num_stages in 1 .. 4, one stride and one dilation per stage, out_indices below num_stages")
        kind, stage_blocks = ARCH[model_type]
        self.model_type, self.block = model_type, _BLOCKS[kind]
        self.stem_channels, self.base_channels, self.num_stages = stem_channels, base_channels, num_stages
        self.strides, self.dilations, self.out_indices, self.style = tuple(strides), tuple(dilations), tuple(out_indices), style
        self.frozen_stages, self.norm_eval, self.zero_init_residual = frozen_stages, norm_eval, zero_init_residual
        self.contract_dilation, self.max_pool_ceil_mode = contract_dilation, max_pool_ceil_mode
        self.stage_blocks = stage_blocks[:num_stages]
        half = stem_channels // 2
        self.stem = _Stem(Conv2d(in_channels, half, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(half), nn.ReLU(inplace=True),
                          Conv2d(half, half, 3, stride=1, padding=1, bias=False), nn.BatchNorm2d(half), nn.ReLU(inplace=True),
                          Conv2d(half, stem_channels, 3, stride=1, padding=1, bias=False), nn.BatchNorm2d(stem_channels),
                          nn.ReLU(inplace=True))
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1, ceil_mode=max_pool_ceil_mode)
        self.res_layers, cin = [], stem_channels
        for i, n in enumerate(self.stage_blocks):
            cout = base_channels * 2 ** i
            self.add_module(f"layer{i + 1}", _res_layer(self.block, n, cin, cout, strides[i], dilations[i], style, contract_dilation))
            self.res_layers.append(f"layer{i + 1}")
            cin = cout * self.block.expansion
        self._freeze_stages()
        self.init_weights(pretrained)

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.stem.eval()
            self.stem.requires_grad_(False)
        for i in range(1, self.frozen_stages + 1):
            m = getattr(self, f"layer{i}")
            m.eval()
            m.requires_grad_(False)

    def init_weights(self, pretrained=None):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        if self.zero_init_residual:                      # every block starts as the identity
            for m in self.modules():
                if isinstance(m, (BasicBlock, Bottleneck)):
                    nn.init.zeros_(getattr(m, m.last_bn).weight)
        if pretrained is None:
            return
        path = IMAGENET_FILES[self.model_type] if pretrained == 'imagenet' else pretrained
        hub = os.path.join(os.environ.get('TORCH_HOME', ''), 'hub')
        for cand in (path, os.path.join(hub, path), os.path.join(hub, 'checkpoints', os.path.basename(path)),
                     os.path.join('pretrained_models', os.path.basename(path))):
            if os.path.exists(cand):
                ckpt = torch.load(cand, map_location='cpu')
                break
        else:
            raise FileNotFoundError(f"ResNet weights '{pretrained}' ({path}) not found locally (no network access)")
        sd = ckpt['state_dict'] if 'state_dict' in ckpt else ckpt
        self.load_state_dict({k: v for k, v in sd.items() if not k.startswith('fc.')}, strict=True)

    def forward(self, x):
        x = self.maxpool(self.stem(x))
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.modules.batchnorm._BatchNorm):      # (BatchNorm2d, or SyncBatchNorm after conversion)
                    m.eval()
        return self


# ---------------------------------------------------------------------------------------------------------------------
# DeepLabV2Head
# ---------------------------------------------------------------------------------------------------------------------
ASPP_FUSED = os.environ.get("RFN_ASPP_FUSED", "1") != "0"     # False: one conv.Conv2d per branch (A/B runs, tests)
MAX_TAPS = 64                                                    # csrc/aspp.hip kAsppMaxTaps


def live_taps(H, W, dilations):
    """The taps of 3x3 convolutions with dilation = padding = d, d in `dilations`, whose offset ((ky - 1) d, (kx - 1) d) can land
    inside an H x W map (|dy| < H and |dx| < W): [(branch, ky, kx, dy, dx)] in (branch, ky, kx) order.  The others only ever
    read padding."""
    return [(r, ky, kx, (ky - 1) * d, (kx - 1) * d) for r, d in enumerate(dilations) for ky in range(3) for kx in range(3)
            if abs((ky - 1) * d) < H and abs((kx - 1) * d) < W]


def _live_boxes(H, W, dilations):
    """live_taps as one (y0, y1, x0, x1) box of the 3x3 grid per branch (the live taps of a branch always form one)."""
    return tuple(((0, 3) if d < H else (1, 2)) + ((0, 3) if d < W else (1, 2)) for d in dilations)


class _Plan:
    """What one map size fixes: the tap table, the padded sizes, the per-branch boxes."""

    def __init__(self, H, W, dilations, classes):
        taps = live_taps(H, W, dilations)
        self.T = len(taps)
        self.boxes = _live_boxes(H, W, dilations)
        self.Np = -(-classes // 8) * 8
        self.Nz = -(-(self.T * self.Np) // 64) * 64               # rows of Wt: the gradient GEMMs want a multiple of 64
        self.table = (ctypes.c_int * (2 * self.T))(*[v for t in taps for v in t[3:]])
        self.starts, n = [], 0
        for y0, y1, x0, x1 in self.boxes:
            self.starts.append(n)
            n += (y1 - y0) * (x1 - x0)
        assert n == self.T

    def taps_ptr(self):
        return ctypes.cast(self.table, ctypes.c_void_p)


def _tapsum(Z, plan, bias, B, H, W, dtype):
    Y = torch.empty((B, H, W, plan.Np), dtype=dtype, device=Z.device)
    _lib.call("rfn_aspp_tapsum", Z.device, ptr(Z), Z.stride(0), ptr(bias), 0 if bias is None else bias.shape[0], plan.taps_ptr(),
              plan.T, ptr(Y), B, H, W, plan.Np, DTYPE_CODE16[dtype])
    return Y


def _tapsum_bwd(gh, plan, dZ, B, H, W, dtype):
    _lib.call("rfn_aspp_tapsum_bwd", gh.device, ptr(gh), plan.taps_ptr(), plan.T, ptr(dZ), dZ.stride(0), B, H, W, plan.Np,
              DTYPE_CODE16[dtype])
    return dZ


def _scratch(M, Nz, dtype, device):
    """(M, Nz) 16-bit scratch for Z / dZ: produced and consumed by back-to-back launches on one stream (_tensor.workspace)."""
    n = M * Nz * 2
    return workspace(n, device)[:n].view(dtype).view(M, Nz)


def _fused_forward(x, weights, biases, plan, dtype):
    B, C, H, W = x.shape
    xh = _nhwc16(x, dtype, C)
    X2 = xh.view(B * H * W, C)
    Wt = tap_stack(weights, dtype, plan.boxes, plan.Np, plan.Nz)
    Z = _mfma.gemm_nt(X2, Wt, out=_scratch(B * H * W, plan.Nz, dtype, x.device))
    if Z is None:
        raise RuntimeError("DeepLabV2Head (fused): operands outside the GEMM kernel's domain")
    bias = bias_stack(biases, plan.Np) if biases[0] is not None else None
    return _tapsum(Z, plan, bias, B, H, W, dtype), X2


class _AsppFn(torch.autograd.Function):
    """The fused head under autograd.  inputs: x, then the R weights, then the R biases."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, plan, dtype, R, *wb):
        weights, biases = wb[:R], wb[R:]
        Y, X2 = _fused_forward(x, weights, biases, plan, dtype)
        ctx.save_for_backward(X2)
        ctx.weights, ctx.biases, ctx.plan, ctx.dtype, ctx.xshape = weights, biases, plan, dtype, x.shape
        K = weights[0].shape[0]
        return (Y[..., :K] if K != plan.Np else Y).permute(0, 3, 1, 2)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gy):
        (X2,) = ctx.saved_tensors
        weights, biases, plan, dtype = ctx.weights, ctx.biases, ctx.plan, ctx.dtype
        B, C, H, W = ctx.xshape
        R, K, M = len(weights), weights[0].shape[0], B * H * W
        gh = _nhwc16(gy, dtype, plan.Np)                             # (B, H, W, Np), zero in the padded channels
        need_w = any(ctx.needs_input_grad[4:4 + R])
        need_b = biases[0] is not None and any(ctx.needs_input_grad[4 + R:])
        db = sum_rows(gh.view(M, plan.Np))[:K] if need_b else None   # every branch's bias gradient: the column sums of gY
        gx, gws, gbs = None, [None] * R, [None] * R
        if ctx.needs_input_grad[0] or need_w:
            dZ = _tapsum_bwd(gh, plan, _scratch(M, plan.Nz, dtype, gh.device), B, H, W, dtype)
            if ctx.needs_input_grad[0]:
                dx = _mfma.gemm_nt(dZ, tap_stack(weights, dtype, plan.boxes, plan.Np, plan.Nz, transpose=True))
                if dx is None:
                    raise RuntimeError("DeepLabV2Head (fused): data gradient outside the GEMM kernel's domain")
                gx = dx.view(B, H, W, C).permute(0, 3, 1, 2)
            if need_w:
                part = _mfma.gemm_tn(dZ, X2)                         # fp32 slab partials (S, Nz, C): summed in slab order
                if part is None:
                    raise RuntimeError("DeepLabV2Head (fused): weight gradient outside the GEMM kernel's domain")
                dWt = sum_rows(part.view(part.shape[0], plan.Nz * C)).view(plan.Nz, C)
                for r, (w, (y0, y1, x0, x1)) in enumerate(zip(weights, plan.boxes)):
                    if not ctx.needs_input_grad[4 + r]:
                        continue
                    ny, nx = y1 - y0, x1 - x0
                    a = plan.starts[r] * plan.Np
                    g = dWt[a:a + ny * nx * plan.Np].view(ny, nx, plan.Np, C)[:, :, :K].permute(2, 3, 0, 1)
                    sink = grad_sink(w)
                    if sink is not None:
                        sink[:, :, y0:y1, x0:x1].add_(g)             # dead taps: nothing added
                    else:
                        gws[r] = torch.zeros(w.shape, dtype=w.dtype, device=w.device)
                        gws[r][:, :, y0:y1, x0:x1] = g
        if need_b:
            for r, b in enumerate(biases):
                if not ctx.needs_input_grad[4 + R + r]:
                    continue
                sink = grad_sink(b)
                if sink is not None:
                    sink.add_(db)
                else:
                    gbs[r] = db.to(b.dtype)
        return (gx, None, None, None, *gws, *gbs)


class DeepLabV2Head(BaseHead):
    """models/heads/deeplabv2.py:8-27."""

    def __init__(self, in_channels: int, in_index: Union[List[int], int], num_classes: int,
                 input_transform: Optional[str] = None, dilation_series: List[int] = [6, 12, 18, 24],
                 padding_series: List[int] = [6, 12, 18, 24]):
        super().__init__(num_classes, in_index, input_transform)
        self.conv2d_list = nn.ModuleList(
            Conv2d(in_channels, num_classes, kernel_size=3, stride=1, padding=p, dilation=d, bias=True)
            for d, p in zip(dilation_series, padding_series))
        for m in self.conv2d_list:
            m.weight.data.normal_(0, 0.01)
            m.bias.data.zero_()
        self._plans = {}

    def fused_ok(self, x):
        """forward(x) takes the tap-GEMM path: GPU, 16-bit compute dtype, padding == dilation and stride 1 in every branch, channels
        as the GEMM kernels want them, at most MAX_TAPS live taps."""
        convs = self.conv2d_list
        if not (ASPP_FUSED and _mfma.ENABLED and torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and len(convs) >= 1
                and compute_dtype(x) in DTYPE_CODE16 and x.shape[1] % 64 == 0 and x.shape[2] < 32768 and x.shape[3] < 32768
                and len(convs) <= 8):
            return False
        for c in convs:
            if not (c.kernel_size == (3, 3) and c.stride == (1, 1) and c.groups == 1 and c.padding_mode == 'zeros'
                    and not isinstance(c.padding, str) and c.padding == c.dilation and c.dilation[0] == c.dilation[1]
                    and c.dilation[0] >= 1 and c.in_channels == x.shape[1] and c.out_channels == convs[0].out_channels
                    and (c.bias is None) == (convs[0].bias is None)):
                return False
        return len(live_taps(x.shape[2], x.shape[3], [c.dilation[0] for c in convs])) <= MAX_TAPS

    def _plan(self, H, W):
        plan = self._plans.get((H, W))
        if plan is None:
            if len(self._plans) > 16:
                self._plans.clear()
            c = self.conv2d_list
            plan = self._plans[(H, W)] = _Plan(H, W, [m.dilation[0] for m in c], c[0].out_channels)
        return plan

    def forward(self, x):
        x = self._transform_inputs(x)
        if self.fused_ok(x):
            cd = compute_dtype(x)
            convs = self.conv2d_list
            weights, biases = [c.weight for c in convs], [c.bias for c in convs]
            plan = self._plan(x.shape[2], x.shape[3])
            if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for c in convs for p in c.parameters())):
                return _AsppFn.apply(x, plan, cd, len(convs), *weights, *biases)
            K = convs[0].out_channels
            Y, _ = _fused_forward(x, weights, biases, plan, cd)
            return (Y[..., :K] if K != plan.Np else Y).permute(0, 3, 1, 2)
        return sum(stage(x) for stage in self.conv2d_list)

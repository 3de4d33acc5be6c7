"""Shared layer containers with the reference's parameter names (models/modules.py:16-68,564-596).

These hold parameters under the same state_dict keys as the reference (`conv.weight`, `bn.running_mean`,
`depthwise_conv.conv.weight`, `pointwise_conv.bn.bias`, `proj.weight`) and execute either the training formulation
(conv -> BatchNorm with batch statistics -> activation) or, for frozen/eval networks under no_grad, a folded one
(BatchNorm merged into the conv weights once, activation in the convolution kernel's epilogue).  ConvBNReLU.route() says
which; conv.conv2d chooses the convolution's kernel.
"""
import torch
import torch.nn as nn

from . import bn as bnk
from .conv import ACT_CODE, LEAKY_SLOPE, act_fusable, activate, conv2d, is_depthwise3x3   # noqa: F401  (LEAKY_SLOPE: align.py)
from .params import compute_dtype

_DW_BN_STATS = True
_DW_BN_FUSED = True


class ConvBNReLU(nn.Module):
    """Constructor semantics and parameter names of models/modules.py:16-56, including the depthwise-separable form
    (a depthwise ConvBNReLU followed by a 1x1 pointwise ConvBNReLU, each with its own norm + activation)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dilation=1, groups=1, padding=None,
                 norm_layer=nn.BatchNorm2d, activation_layer=nn.ReLU, bias='auto', depthwise_separable=False,
                 inplace=True, affine=True):
        super().__init__()
        padding = dilation * (kernel_size - 1) // 2 if padding is None else padding
        self.use_norm = norm_layer is not None
        self.use_activation = activation_layer is not None
        self.depthwise_separable = depthwise_separable
        if bias == 'auto':
            bias = not self.use_norm
        if depthwise_separable:
            assert kernel_size > 1 and groups == 1
            self.depthwise_conv = ConvBNReLU(in_channels, in_channels, kernel_size, stride=stride, padding=padding,
                                             dilation=dilation, groups=in_channels, norm_layer=norm_layer,
                                             activation_layer=activation_layer)
            self.pointwise_conv = ConvBNReLU(in_channels, out_channels, 1, norm_layer=norm_layer,
                                             activation_layer=activation_layer)
        else:
            self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, dilation=dilation,
                                  groups=groups, bias=bias)
            if self.use_norm:
                self.bn = norm_layer(out_channels, affine=affine)
        self.act, self.act_slope = None, 0.0
        if self.use_activation:
            probe = activation_layer()
            self.act = 'leaky' if isinstance(probe, nn.LeakyReLU) else 'relu'
            self.act_slope = getattr(probe, 'negative_slope', 0.0)
        self._folded = None

    # -- eval-time folding -------------------------------------------------------------------------------------------
    def folded(self):
        """(weight, bias) with eval-mode BatchNorm folded in; cached until train() / load_state_dict()."""
        if self._folded is None:
            c = self.conv
            self._folded = bnk.fold(c.weight, c.bias, self.bn) if self.use_norm else \
                (c.weight.detach().contiguous(), None if c.bias is None else c.bias.detach().contiguous())
        return self._folded

    def train(self, mode=True):
        self._folded = None
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self._folded = None
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *a, **k):
        self._folded = None
        return super()._apply(fn, *a, **k)

    # -- what a caller may ask of a block ----------------------------------------------------------------------------
    @property
    def last(self):
        """the module whose BatchNorm + activation ends this block"""
        return self.pointwise_conv if self.depthwise_separable else self

    def _out_count(self, x):
        """values per channel of this block's convolution result on `x` (batch x OH x OW)"""
        c = self.conv
        n = x.shape[0]
        for i in (0, 1):
            pad = c.padding[i] if not isinstance(c.padding, str) else (c.dilation[i] * (c.kernel_size[i] - 1) // 2 if c.padding == "same" else 0)
            n *= max(0, (x.shape[2 + i] + 2 * pad - c.dilation[i] * (c.kernel_size[i] - 1) - 1) // c.stride[i] + 1)
        return n

    def _bn_kernel(self, x):
        """BatchNorm(train) + activation of this (plain) block's convolution on `x` go on csrc/bn.hip: THE predicate behind
        bn_kernel_ok, fused_out_ok and route()."""
        return (x.is_cuda and self.use_norm and self.training and act_fusable(self.act, self.act_slope) and bnk.kernel_enabled()
                and bnk.usable(x, self.bn, compute_dtype(x), channels=self.conv.out_channels, count=self._out_count(x)))

    def bn_kernel_ok(self, x):
        """forward(x) of this block ends in the fused BatchNorm(train) + activation pass (csrc/bn.hip) -- the pass that takes
        the decode heads' Dropout2d with it (forward(x, drop=...)) and whose input a caller may compute itself (pre_norm)."""
        return not self.depthwise_separable and self._bn_kernel(x)

    def fused_out_ok(self, x):
        """forward(x, out=...) is available: gradient-free, training-mode BatchNorm on the fused kernel (the EMA teacher's
        decode head) -- the block's result can be written straight into a channel slice of a wider tensor."""
        m = self.last
        return not torch.is_grad_enabled() and m.act in (None, 'relu') and m._bn_kernel(x)

    def pre_norm(self, x, cd):
        """The convolution of a training-mode block on the GPU in the 16-bit compute dtype `cd`: what the fused BatchNorm pass
        normalises.  1x1 (the ASPP / fusion projections): a Linear over channels-last tokens on the MFMA GEMM kernels, forward
        and both gradients -- a route of the block, since it pays only where a BatchNorm pass reads the tokens next; every other
        shape: conv.conv2d (depthwise 3x3: the HIP stencil; dense k x k: the implicit-GEMM kernels)."""
        c = self.conv
        # (under autograd the Linear's gradient GEMMs want N % 64 == 0; other widths take the implicit-GEMM path, which pads its
        # output channels itself)
        if c.groups == 1 and c.kernel_size == (1, 1) and c.stride == (1, 1) and c.padding == (0, 0) and \
                c.in_channels % 64 == 0 and c.out_channels % (64 if torch.is_grad_enabled() else 8) == 0:
            from .linear import linear_tokens
            xh = x.permute(0, 2, 3, 1)
            if xh.dtype != cd:
                xh = xh.to(cd)
            if not xh.is_contiguous():
                xh = xh.contiguous()
            B, H, W, C = xh.shape
            y = linear_tokens(xh.reshape(B * H * W, C), c.weight, c.bias, cd)
            return y.view(B, H, W, -1).permute(0, 3, 1, 2)
        return conv2d(x, c.weight, c.bias, c.stride, c.padding, c.dilation, c.groups, needs_grad=torch.is_grad_enabled())

    # -- one route decision, one body per route ----------------------------------------------------------------------
    ROUTES = ("parts-split32", "separable", "bn-kernel", "folded", "plain")

    def route(self, x, out=None, drop=None):
        """Which body forward(x, out, drop) runs (ROUTES); the kernel of the convolution inside it is conv.conv2d's choice.
          parts-split32  a list of fp32 parts, gradient-free, eval-mode or no BatchNorm: the parts go straight into the split-bf16
                         convolution's operand (a list outside that domain is routed as its concatenation)
          separable      depthwise block, then pointwise block
          bn-kernel      convolution (pre_norm, or the depthwise stencil with statistics), then ONE fused BatchNorm(train) +
                         activation pass (csrc/bn.hip); the only route that takes out= and drop=
          folded         gradient-free, BatchNorm in eval mode: folded into the weights, activation in the kernel's epilogue
          plain          convolution, the BatchNorm module if there is one, activation
        Raises where forward does (drop= off the bn-kernel route)."""
        parts = isinstance(x, (list, tuple))
        if drop is not None:
            if parts or not self.bn_kernel_ok(x):
                raise RuntimeError("ConvBNReLU(drop=...): on the fused BatchNorm(train) pass only (bn_kernel_ok)")
            return "bn-kernel"
        if parts:
            if self._parts_ok(x, out):
                return "parts-split32"
            x = x[0]                       # device, dtype and (B, H, W) of the concatenation
        if self.depthwise_separable:
            return "separable"
        if out is not None or self._bn_kernel(x):     # out=: the caller asked fused_out_ok
            return "bn-kernel"
        return "folded" if self.use_norm and not self.training and not torch.is_grad_enabled() else "plain"

    def forward(self, x, out=None, drop=None):
        # out: a channel slice of a wider channels-last tensor for the result -- where fused_out_ok(x) holds
        # drop: (B, C, 1, 1) Dropout2d multipliers folded into the BatchNorm pass -- only where bn_kernel_ok(x) holds
        r = self.route(x, out, drop)
        if isinstance(x, (list, tuple)):
            # a channel concatenation handed over as its parts (the matcher's decoders: cat(correlation, flow, ...))
            if r == "parts-split32":
                return self._run_parts(x)
            x = torch.cat(list(x), 1)
        if r == "separable":
            return self.pointwise_conv(self.depthwise_conv(x), out=out)
        if r == "bn-kernel":
            return self._run_bn_kernel(x, out, drop)
        # folded / plain.  The frozen matcher's blocks are ONE launch: folded norm in the weights, bias and ReLU / LeakyReLU in the
        # epilogue of the implicit-GEMM kernel (16-bit) or of the split-bf16 one (fp32: parity mode, align.HEAD_SPLIT)
        c = self.conv
        w, b = self.folded() if r == "folded" else (c.weight, c.bias)
        if self.use_norm and r == "plain":
            return activate(self.bn(conv2d(x, w, b, c.stride, c.padding, c.dilation, c.groups)), self.act, self.act_slope)
        return conv2d(x, w, b, c.stride, c.padding, c.dilation, c.groups, act=self.act, slope=self.act_slope)

    def _parts_ok(self, x, out):
        c = getattr(self, "conv", None)
        if not (c is not None and out is None and x[0].is_cuda and c.groups == 1 and not torch.is_grad_enabled()
                and (not self.use_norm or not self.training) and act_fusable(self.act, self.act_slope)
                and all(t.dtype == torch.float32 for t in x) and not torch.is_autocast_enabled("cuda")
                and c.stride[0] == c.stride[1] and c.padding[0] == c.padding[1] and c.dilation[0] == c.dilation[1]):
            return False
        from . import split32
        return split32.usable(*x) and split32.parts_ok(x, c.weight)

    def _run_parts(self, x):
        """split32.conv2d_parts on the parts (_parts_ok has asked for its whole domain)"""
        from . import split32
        c = self.conv
        w, b = self.folded() if self.use_norm else (c.weight, c.bias)
        y = split32.conv2d_parts(list(x), w, b, c.stride[0], c.padding[0], c.dilation[0], act=ACT_CODE[self.act])
        if y is None:
            raise RuntimeError("ConvBNReLU: split32.conv2d_parts declined a call that split32.parts_ok admits")
        return y

    def _dw_stats_ok(self, x, cd):
        """depthwise 3x3 -> BatchNorm(train): the convolution kernel leaves the batch statistics of its result behind
        (csrc/dwconv.hip STATS), the BatchNorm skips its statistics pass.  (_DW_BN_STATS = False: two passes.)"""
        c = self.conv
        return (_DW_BN_STATS and x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and cd == x.dtype
                and is_depthwise3x3(c.weight, c.stride, c.padding, c.dilation, c.groups))

    def _run_bn_kernel(self, x, out=None, drop=None):
        cd, act, c = compute_dtype(x), ACT_CODE[self.act], self.conv
        if drop is None and self._dw_stats_ok(x, cd):
            if not torch.is_grad_enabled() and out is None and act in (0, 1) and _DW_BN_FUSED and self.bn.momentum is not None:
                # gradient-free (EMA teacher): statistics pass without a store, then convolution + BatchNorm + ReLU in one pass
                from .dwconv import dwconv3x3_bn_act_nhwc
                xh = x.permute(0, 2, 3, 1)
                y = dwconv3x3_bn_act_nhwc(xh if xh.is_contiguous() else xh.contiguous(), c.weight, c.bias, c.dilation[0], self.bn,
                                          act == 1)
                return y.permute(0, 3, 1, 2)
            sums = torch.empty(2 * c.out_channels + 1, dtype=torch.float64, device=x.device)
            y = conv2d(x, c.weight, c.bias, c.stride, c.padding, c.dilation, c.groups, stats=sums)
            return bnk.bn_act_train(y, self.bn, act, cd, out=out, sums=sums)
        # decode heads (student and EMA teacher run BatchNorm with batch statistics): convolution on the hand-written
        # kernels where they exist for the pass, then ONE fused BatchNorm(train) + ReLU (csrc/bn.hip)
        return bnk.bn_act_train(self.pre_norm(x, cd), self.bn, act, cd, out=out, drop=drop)


class MLP(nn.Module):
    """Linear embedding of an NCHW map into tokens (models/modules.py:59-68): (B,C,H,W) -> (B,H*W,embed_dim)."""

    def __init__(self, input_dim=2048, embed_dim=768):
        super().__init__()
        from .linear import Linear
        self.proj = Linear(input_dim, embed_dim)

    def forward(self, x):
        return self.proj(x.flatten(2).transpose(1, 2))


class DropPath(nn.Module):
    """Stochastic depth per sample (models/modules.py:564-596)."""

    def __init__(self, drop_prob: float = 0., scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep

    def forward(self, x):
        if self.drop_prob == 0. or not self.training:
            return x
        keep = 1 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)
        if keep > 0.0 and self.scale_by_keep:
            mask.div_(keep)
        return x * mask

    def residual(self, x, y):
        """x + drop_path(y) in ONE elementwise kernel (addcmul) instead of a broadcast multiply and an add: the MiT
        residual stream is pure HBM traffic (2 x 52 blocks x 4 passes per step).  Same random draw as forward()."""
        if self.drop_prob == 0. or not self.training:
            return x + y
        keep = 1 - self.drop_prob
        mask = y.new_empty((y.shape[0],) + (1,) * (y.ndim - 1)).bernoulli_(keep)
        if keep > 0.0 and self.scale_by_keep:
            mask.div_(keep)
        if x.dtype != y.dtype:
            return x + y * mask
        return torch.addcmul(x, y, mask)

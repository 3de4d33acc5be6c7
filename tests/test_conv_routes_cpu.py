"""ConvBNReLU / conv.conv2d on CPU tensors: exactly the F.conv2d -> BatchNorm -> activation composition built from the same
parameters, forward and backward (the host-side route of every block-level case of tests/test_conv_routes_gpu.py), and the
route names of the block."""
import copy
from functools import partial

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from refign_amd.layers import ConvBNReLU

B, H, W = 2, 12, 20
_leaky = partial(nn.LeakyReLU, negative_slope=0.1)
DW = dict(dilation=6, padding=6)

#        name                     constructor args / keywords                                       C_in  train
BLOCKS = [
    ("pw64", (64, 64, 1), {}, 64, True),
    ("pw64to24", (64, 24, 1), {}, 64, True),
    ("dw64", (64, 64, 3), dict(groups=64, **DW), 64, True),
    ("dw12", (12, 12, 3), dict(groups=12, **DW), 12, True),
    ("separable", (64, 64, 3), dict(depthwise_separable=True, **DW), 64, True),
    ("dense3x3", (128, 64, 3), {}, 128, True),
    ("eval_bn_leaky", (64, 64, 3), dict(activation_layer=_leaky), 64, False),
    ("eval_bn_slope02", (64, 64, 3), dict(activation_layer=partial(nn.LeakyReLU, 0.2)), 64, False),
    ("nonorm_leaky", (24, 16, 3), dict(norm_layer=None, activation_layer=_leaky), 24, True),
    ("nonorm_noact", (24, 16, 3), dict(norm_layer=None, activation_layer=None), 24, True),
    ("conv1to32_k7_leaky", (1, 32, 7), dict(padding=0, activation_layer=_leaky), 1, True),
    ("groups2", (64, 64, 3), dict(groups=2), 64, True),
]


def _compose(m, x):
    """what the reference's module computes, from m's own parameters"""
    if m.depthwise_separable:
        return _compose(m.pointwise_conv, _compose(m.depthwise_conv, x))
    c = m.conv
    y = F.conv2d(x, c.weight, c.bias, c.stride, c.padding, c.dilation, c.groups)
    if m.use_norm:
        y = m.bn(y)
    if m.act == 'leaky':
        y = F.leaky_relu(y, m.act_slope)
    elif m.act == 'relu':
        y = F.relu(y)
    return y


def _build(args, kw, train):
    torch.manual_seed(7)
    m = ConvBNReLU(*args, **kw)
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            with torch.no_grad():
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0, 0.1)
                mod.running_mean.normal_(0, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
    return m.train(train)


@pytest.mark.parametrize("name,args,kw,cin,train", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_cpu_block_is_the_composition(name, args, kw, cin, train):
    m = _build(args, kw, train)
    ref = copy.deepcopy(m)
    x = torch.randn(B, cin, H, W)
    g = None
    got = []
    for mod, fn in ((m, lambda t: m(t)), (ref, lambda t: _compose(ref, t))):
        xi = x.clone().requires_grad_(True)
        y = fn(xi)
        g = torch.randn_like(y) if g is None else g
        y.backward(g)
        got.append([y.detach(), xi.grad] + [p.grad for p in mod.parameters()] + [b for b in mod.buffers()])
    assert len(got[0]) == len(got[1])
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_cpu_parts_input_is_the_concatenation():
    m = _build((24, 16, 3), dict(activation_layer=_leaky), True)
    ref = copy.deepcopy(m)
    parts = [torch.randn(B, 16, H, W), torch.randn(B, 8, H, W)]
    assert torch.equal(m(parts), _compose(ref, torch.cat(parts, 1)))


def test_cpu_one_value_per_channel_raises():
    m = _build((64, 64, 3), dict(padding=0), True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m(torch.randn(1, 64, 3, 3))


def test_cpu_drop_raises():
    m = _build((128, 64, 3), {}, True)
    with pytest.raises(RuntimeError, match="on the fused BatchNorm"):
        m(torch.randn(B, 128, H, W), drop=torch.ones(B, 64, 1, 1))


def test_cpu_conv2d_module_is_nn_conv2d():
    from refign_amd.conv import Conv2d
    torch.manual_seed(3)
    m = Conv2d(24, 64, 3, stride=2, padding=1)
    x = torch.randn(B, 24, H, W)
    assert torch.equal(m(x), F.conv2d(x, m.weight, m.bias, 2, 1))


def test_route_names():
    x = torch.randn(B, 64, H, W)
    assert _build((64, 64, 3), dict(depthwise_separable=True, **DW), True).route(x) == "separable"
    assert _build((64, 64, 3), {}, True).route(x) == "plain"                  # (a CPU tensor: no fused BatchNorm pass)
    assert _build((64, 64, 3), {}, False).route(x) == "plain"                 # eval-mode BatchNorm under autograd: the module
    with torch.no_grad():
        assert _build((64, 64, 3), {}, False).route(x) == "folded"
        assert _build((64, 64, 3), {}, False).route([x, x]) == "folded"       # parts outside the split-bf16 domain
        assert _build((64, 64, 3), dict(norm_layer=None), False).route(x) == "plain"
    assert set(ConvBNReLU.ROUTES) == {"parts-split32", "separable", "bn-kernel", "folded", "plain"}

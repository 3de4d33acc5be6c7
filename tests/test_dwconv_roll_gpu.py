"""GPU: the rolling row walk of the gradient-free depthwise 3x3 forms (csrc/dwconv.hip dwconv3x3_roll_kernel: statistics
only, and convolution + BatchNorm + ReLU) at the smallest shapes where a walk down a residue class can go wrong: taps
outside the image on every side, residue classes of unequal length, ragged strips, strips wider than the image, image and
segment seams."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, H, W, C, dilation)
SHAPES = [(3, 5, 4, 2048, 18),     # every off-centre tap outside the image, XCD-sliced geometry, image seams
          (2, 23, 31, 1024, 6),    # H % d != 0: residue classes of 4 and 3 rows
          (1, 40, 67, 192, 3),     # ragged strip (67 = 3 x 22 + 1), idle channel lanes (48 vectors in blocks of 32)
          (2, 19, 7, 64, 6),       # strip (4 outputs, 6 columns, spaced by 6) wider than the image
          (2, 37, 9, 8, 1),        # one channel vector per pixel, many row segments (5 of 8, 8, 8, 8, 5 rows)
          # a class of 17 rows = 2 segments + 1 row: roll_geom() cuts a class into segments of 8 rows at the least when the
          # map has fewer than 4 items per pixel lane of the grid, as here (sliced geometry: 512 lanes, 2 strips)
          (1, 17, 5, 1024, 1)]


def _exact_inputs(B, H, W, C, dil, dtype, dev):
    """integers in [-2, 2], weights in {-1, -0.5, 0, 0.5, 1}, bias multiples of 0.5: every convolution result is a multiple of
    0.5 with |.| <= 9 x 2 x 1 + 1 = 19, exact in bf16 / fp16, and its square a multiple of 0.25 <= 361.  A channel has at most
    B H W <= 2680 results (1 x 40 x 67), so every partial sum of a channel -- a thread's, a block's -- is a multiple of 0.5
    with |.| <= 2680 x 19 = 50 920 < 2^16, of squares a multiple of 0.25 <= 2680 x 361 = 967 480 < 2^20: as multiples of
    0.25 both are integers below 2^22 < 2^24, exact in fp32 in any summation order, and exact in fp64 after that"""
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C + dil)
    x = torch.randint(-2, 3, (B, H, W, C), generator=g).to(dtype)
    w = torch.randint(-2, 3, (C, 1, 3, 3), generator=g).float() * 0.5
    b = torch.randint(-2, 3, (C,), generator=g).float() * 0.5
    return x.to(dev), w.to(dev), b.to(dev)


@functools.lru_cache(maxsize=None)
def _exact_sums(B, H, W, C, dil, dtype):
    """fp64 sums of F.conv2d on the host: (sum, sum of squares) per channel"""
    x, w, b = _exact_inputs(B, H, W, C, dil, dtype, "cpu")
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=dil, dilation=dil, groups=C)
    return y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3))


@functools.lru_cache(maxsize=None)
def _exact_conv(B, H, W, C, dil, dtype):
    """F.conv2d of the same inputs on the host, cast to the dtype (the values are exact in it): (B, H, W, C)"""
    x, w, b = _exact_inputs(B, H, W, C, dil, dtype, "cpu")
    y = F.conv2d(x.float().permute(0, 3, 1, 2), w, b, padding=dil, dilation=dil, groups=C)
    return y.permute(0, 2, 3, 1).contiguous().to(dtype)


def test_exact_reference_is_exact():
    """the premise of the exact tests, on the host: the fp64 sums of every shape are multiples of 0.5 (squares: 0.25) whose
    count of quarter units is below 2^24, and the results themselves survive the cast to bf16 and fp16"""
    for B, H, W, C, dil in SHAPES:
        for dtype in (torch.bfloat16, torch.float16):
            s0, s1 = _exact_sums(B, H, W, C, dil, dtype)
            assert torch.equal(s0 * 2, (s0 * 2).round()) and torch.equal(s1 * 4, (s1 * 4).round())
            assert float((s0 * 4).abs().max()) < 2.0 ** 24 and float((s1 * 4).max()) < 2.0 ** 24
            y = _exact_conv(B, H, W, C, dil, dtype).double()
            assert float(y.abs().max()) <= 19 and torch.equal(y.sum(dim=(0, 1, 2)), s0)


# (`storing` shares the last id with `det`: the cases without it keep the ids they had before the parameter existed)
@pytest.mark.parametrize("det,storing", [pytest.param(d, s, id=f"{d}-storing" if s else str(d))
                                         for s in (False, True) for d in (False, True)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,W,C,dil", SHAPES)
def test_store_free_statistics_are_exact(dev, B, H, W, C, dil, dtype, det, storing):
    """rfn_dwconv3x3_nhwc_stats (and, under `determinism`, rfn_dwconv3x3_nhwc_stats_det) on inputs whose sums are exact in
    every precision involved == the fp64 sums of F.conv2d, to the bit, including the row count: a misplaced tap, a sum
    carried over a seam or a row counted twice at a segment edge cannot hide behind a tolerance.  `storing`: the sums of the
    kernel that stores the convolution (dwconv3x3_nhwc(stats=...): rfn_dwconv3x3_nhwc_fwd_stats / _fwd_stats_det) instead,
    which share the fold; its stored result == F.conv2d of the same inputs, to the bit."""
    from refign_amd import determinism
    from refign_amd.dwconv import dwconv3x3_nhwc, dwconv3x3_stats_nhwc
    x, w, b = _exact_inputs(B, H, W, C, dil, dtype, dev)
    s0, s1 = _exact_sums(B, H, W, C, dil, dtype)
    with determinism.deterministic(det), torch.no_grad():
        if storing:
            sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
            y = dwconv3x3_nhwc(x, w, b, dil, stats=sums)
            sums = sums.cpu()
            assert torch.equal(y.cpu(), _exact_conv(B, H, W, C, dil, dtype))
        else:
            sums = dwconv3x3_stats_nhwc(x, w, b, dil).cpu()
    assert float(sums[2 * C]) == B * H * W
    assert torch.equal(sums[:C], s0)
    assert torch.equal(sums[C:2 * C], s1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,W,C,dil", SHAPES)
def test_store_free_statistics_are_those_of_the_stored_result(dev, B, H, W, C, dil, dtype):
    """random inputs: the kernel that stores the convolution and takes its statistics gives the plain kernel's values, and
    the store-free pass gives the statistics bn._stats_fwd reads back from them (same rounded values, other summation
    order: the 1e-5 relative bound of test_dwconv_leaves_the_batchnorm_statistics_of_its_result)."""
    from refign_amd import bn as bnk
    from refign_amd.dwconv import dwconv3x3_nhwc, dwconv3x3_stats_nhwc
    g = torch.Generator().manual_seed(C + H + dil)
    x = (torch.randn(B, H, W, C, generator=g) + 0.3).to(dev).to(dtype)
    w = torch.randn(C, 1, 3, 3, generator=g).to(dev)
    b = torch.randn(C, generator=g).to(dev)
    with torch.no_grad():
        want = dwconv3x3_nhwc(x, w, b, dil)
        with_stats = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
        got = dwconv3x3_nhwc(x, w, b, dil, stats=with_stats)
    assert torch.equal(got, want)
    sums = dwconv3x3_stats_nhwc(x, w, b, dil)
    ref = torch.empty_like(sums)
    bnk._stats_fwd(want, ref)
    assert float(sums[2 * C]) == float(ref[2 * C]) == B * H * W
    scale = ref[C:2 * C].abs().max()
    assert float((sums[:C] - ref[:C]).abs().max()) <= 1e-5 * float(ref[:C].abs().max() + scale.sqrt())
    assert float((sums[C:2 * C] - ref[C:2 * C]).abs().max()) <= 1e-5 * float(scale)


def _two_pass_and_chain(x, w, b, dil, relu, dev, g):
    from refign_amd import bn as bnk
    from refign_amd.dwconv import dwconv3x3_bn_act_nhwc, dwconv3x3_nhwc
    C = x.shape[-1]
    bn_a = torch.nn.BatchNorm2d(C).to(dev).train()
    with torch.no_grad():
        bn_a.weight.copy_(torch.rand(C, generator=g).to(dev) + 0.5)
        bn_a.bias.copy_(torch.randn(C, generator=g).to(dev))
    bn_b = copy.deepcopy(bn_a)
    with torch.no_grad():
        got = dwconv3x3_bn_act_nhwc(x, w, b, dil, bn_a, relu)
        conv = dwconv3x3_nhwc(x, w, b, dil)
        want = bnk.bn_act_train(conv.permute(0, 3, 1, 2), bn_b, 1 if relu else 0, x.dtype).permute(0, 2, 3, 1)
    assert torch.allclose(bn_a.running_mean, bn_b.running_mean, rtol=1e-6, atol=1e-7)
    assert torch.allclose(bn_a.running_var, bn_b.running_var, rtol=1e-6, atol=1e-7)
    assert int(bn_a.num_batches_tracked) == int(bn_b.num_batches_tracked) == 1
    return got, want


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("B,H,W,C,dil", SHAPES)
def test_convolution_batchnorm_relu_pass(dev, B, H, W, C, dil, relu):
    """dwconv3x3_bn_act_nhwc == depthwise kernel -> csrc/bn.hip statistics -> apply, under the conditions of
    test_gradient_free_dwconv_batchnorm_relu_in_two_input_passes: at most one bf16 rounding step apart, fewer than 1e-3 of
    the elements different, running buffers and num_batches_tracked equal."""
    g = torch.Generator().manual_seed(C + H + dil)
    x = (torch.randn(B, H, W, C, generator=g) + 0.2).to(dev).to(torch.bfloat16)
    w = torch.randn(C, 1, 3, 3, generator=g).to(dev)
    b = torch.randn(C, generator=g).to(dev)
    got, want = _two_pass_and_chain(x, w, b, dil, relu, dev, g)
    err = (got.float() - want.float()).abs()
    assert float(err.max()) <= 2.0 ** -7 * float(want.float().abs().max())
    assert float((err > 0).float().mean()) < 1e-3


@pytest.mark.parametrize("dtype,step", [(torch.bfloat16, 2.0 ** -7), (torch.float16, 2.0 ** -10)])
@pytest.mark.parametrize("B,H,W,C,dil", SHAPES)
def test_convolution_batchnorm_relu_pass_with_exact_statistics(dev, B, H, W, C, dil, dtype, step):
    """the same comparison on the inputs whose statistics are exact, bf16 and fp16: both sides then normalise with the same
    mean and variance, so they may differ by the rounding of the affine map alone -- one step of the result's precision"""
    x, w, b = _exact_inputs(B, H, W, C, dil, dtype, dev)
    got, want = _two_pass_and_chain(x, w, b, dil, True, dev, torch.Generator().manual_seed(C + dil))
    err = (got.float() - want.float()).abs()
    assert float(err.max()) <= step * float(want.float().abs().max())

"""GPU: the deterministic mode (refign_amd/determinism.py, Trainer(deterministic=True)).

1. Every converted entry point alone: the store-and-sum form gives identical bits in 5 launches (two of them while a second
   stream keeps the device busy), agrees with the atomic form to the tolerance that form's own test uses against its
   reference, and the atomic form refuses (RFN_ENONDET -> RuntimeError) while the library's flag is set.  Inputs: magnitudes
   spread over 2^-12 .. 2^12 with mixed signs (`_harsh`), so that a sum visibly depends on its order; whether the atomic form
   differed between launches on them is printed, not asserted.
2. The step: two models built from one seed under Trainer(deterministic=True) agree bit for bit after every one of 8 steps
   in every loss, parameter, EMA parameter, buffer, Adam moment and loss-scale state -- DAFormer and HRDA, bf16 and fp16,
   hipGraph replay on and off.
3. The same across two fresh processes (SHA-256 per tensor per step).
4. Exact resume, 5. validation in between, 6. refusals, 7. the default mode calls none of the new entry points.
"""
import json
import math
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from conftest import ROOT
from fill import hashed_uniform
from test_resume_gpu import _model, _seed, _steps
from test_step_gpu import build, make_batch

pytestmark = pytest.mark.gpu
LOSSES = ("train_loss_src", "train_loss_featdist_src", "train_loss_uda_trg")
NEW_ENTRY_POINTS = ("rfn_bn_stats_fwd_det", "rfn_bn_stats_bwd_det", "rfn_dwconv3x3_nhwc_fwd_stats_det",
                    "rfn_dwconv3x3_nhwc_stats_det", "rfn_attn_bwd_dkv_det", "rfn_dacs_mix_jitter_det", "rfn_upsample_ce_det",
                    "rfn_upsample_bilinear2d_bwd", "rfn_set_deterministic", "rfn_bn_stats_det_workspace_bytes",
                    "rfn_dwconv3x3_stats_det_workspace_bytes", "rfn_dacs_mix_jitter_det_workspace_bytes",
                    "rfn_upsample_ce_det_workspace_bytes")


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _harsh(shape, key, dev, dtype=torch.float32, kmax=12):
    """+-2^k (1 + m): k uniform in [-kmax, kmax], m a hashed 24-bit mantissa, sign hashed."""
    k = np.floor(hashed_uniform(shape, key + "/k") * (2 * kmax + 1)) - kmax
    m = 1.0 + hashed_uniform(shape, key + "/m")
    s = np.where(hashed_uniform(shape, key + "/s") < 0.5, -1.0, 1.0)
    return torch.from_numpy((s * m * np.exp2(k)).astype(np.float32)).to(dev).to(dtype)


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.to(torch.uint8) if t.dtype == torch.bool else t.view(torch.uint8)


def _bit_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))      # NaNs compare too


class _Busy:
    """Unrelated work on a second stream around a launch, so that workgroup arrival order really changes."""

    def __init__(self, dev):
        self.dev, self.stream = dev, torch.cuda.Stream(device=dev)
        self.a = torch.randn(4096, 4096, device=dev)

    def __enter__(self):
        with torch.cuda.stream(self.stream):
            for _ in range(24):
                self.a = torch.tanh(self.a @ self.a * 1e-3)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize(self.dev)
        return False


def _five_launches(dev, run):
    """run() five times, the third and fifth next to a busy stream -> list of tuples of tensors"""
    outs, busy = [], _Busy(dev)
    for i in range(5):
        if i in (2, 4):
            with busy:
                outs.append(run())
        else:
            outs.append(run())
        torch.cuda.synchronize(dev)
    return outs


def _entry_point_case(dev, name, run, tols, raw_default):
    """(a) the deterministic form repeats bit for bit, (b) agrees with the atomic form within tols[i](default_i) per output,
    (c) the atomic form refuses under the flag.  run() -> tuple of fresh output tensors, in the current mode."""
    from refign_amd import _lib, determinism
    with determinism.deterministic():
        det = _five_launches(dev, run)
    for k, o in enumerate(det[1:], 1):
        for i, (x, y) in enumerate(zip(det[0], o)):
            assert _bit_equal(x, y), f"{name}: output {i} of launch {k} differs from launch 0 in deterministic mode"
    dflt = _five_launches(dev, run)
    moved = any(not _bit_equal(x, y) for o in dflt[1:] for x, y in zip(dflt[0], o))
    print(f"\n{name}: atomic form {'DIFFERED' if moved else 'did not differ'} between 5 launches on these inputs")
    for i, (x, y) in enumerate(zip(det[0], dflt[0])):
        err, bound = float((x.double() - y.double()).abs().max()), tols[i](y)
        print(f"{name}: output {i}: |deterministic - atomic| max {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, i, err, bound)
    lib = _lib.load_library()
    with determinism.deterministic():
        assert lib.rfn_get_deterministic() == 1
        rc = raw_default(lib)
        assert rc == -4, (name, rc)
        with pytest.raises(RuntimeError, match="refused in deterministic mode"):
            _lib.check(rc, name)
    assert lib.rfn_get_deterministic() == 0
    return moved


def _rel(f, extra=0.0):
    return lambda ref: f * float(ref.double().abs().max()) + extra


# ---------------------------------------------------------------------------------------------------------------------
# 1. every converted entry point, alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("scaled", [False, True])
def test_gemm_tn_accumulate_form(dev, dtype, scaled):
    """Weight and bias gradient of a Linear layer, 32 768 rows in 64 slabs of 512 (rfn_gemm_tn accumulate = 2 + sum_rows against
    accumulate = 1), with and without the stochastic-depth row scale.  Tolerance: test_mfma_gpu.
    test_gemm_tn_accumulates_into_gradient_views (2e-5 max sqrt(T / 1000 + 1) + 1e-3).
    Observed on an MI355X: see profiles/deterministic_ab.txt."""
    from refign_amd import mfma
    from refign_amd._tensor import current_stream, ptr
    T, N, K = 32768, 128, 128
    kmax = 12 if dtype == torch.bfloat16 else 6                 # fp16: products stay inside the format's range
    g, x = _harsh((T, N), "det/g", dev, dtype, kmax), _harsh((T, K), "det/x", dev, dtype, kmax)
    gw0, gb0 = _harsh((N, K), "det/gw0", dev), _harsh((N,), "det/gb0", dev)
    rs = (torch.rand(4, device=dev) + 0.5) if scaled else None
    rps = T // 4 if scaled else 0

    def run():
        gw, gb = gw0.clone(), gb0.clone()
        assert mfma.gemm_tn(g, x, out=gw, bias_out=gb, rowscale=rs, rows_per_sample=rps) is gw
        return gw, gb

    tol = lambda ref: 2e-5 * float(ref.abs().max()) * math.sqrt(T / 1000 + 1) + 1e-3  # noqa: E731
    gw, gb = gw0.clone(), gb0.clone()
    raw = lambda lib: lib.rfn_gemm_tn(ptr(g), ptr(x), ptr(gw), T, N, K, N, K, 512, 1, ptr(gb), ptr(rs), rps,  # noqa: E731
                                      mfma._DT16[dtype], current_stream(dev))
    _entry_point_case(dev, f"gemm_tn[{dtype}, scaled={scaled}]", run, [tol, tol], raw)
    assert _bit_equal(gw, gw0) and _bit_equal(gb, gb0), "the refused launch wrote"
    # the grouped kernel refuses as a whole; in deterministic mode nothing is queued for it
    from refign_amd import determinism
    with determinism.deterministic(), mfma.deferred_wgrads():
        assert not mfma.defer_gemm_tn(g, x, gw, gb)


def test_conv_weight_gradient_bias_sums(dev):
    """rfn_conv2d_nhwc_wgrad: the slab partials were plain stores already; its bias column sums were atomics (accumulate = 0) and
    are per-slab rows now (accumulate = 2).  Tolerance: test_mfma_gpu's convolution test, 1e-5 sqrt(T / 1000 + 1) max + 1e-3."""
    from refign_amd import mfma
    from refign_amd._tensor import current_stream, ptr
    B, H, W, C, N = 2, 96, 128, 64, 64
    gy = _harsh((B, H, W, N), "det/cgy", dev, torch.bfloat16)
    x = _harsh((B, H, W, C), "det/cx", dev, torch.bfloat16)
    T = B * H * W

    def run():
        bsum = torch.zeros(N, dtype=torch.float32, device=dev)
        part = mfma.conv2d_nhwc_wgrad(gy, x, 3, 3, 9 * C, 1, 1, 1, bias_out=bsum)
        assert part is not None and part.shape[0] >= 8
        return part.sum(0), bsum

    tol = lambda ref: 1e-5 * math.sqrt(T / 1000 + 1) * float(ref.abs().max()) + 1e-3  # noqa: E731
    part = torch.empty((64, N, 9 * C), dtype=torch.float32, device=dev)
    bs = torch.zeros(N, dtype=torch.float32, device=dev)
    raw = lambda lib: lib.rfn_conv2d_nhwc_wgrad(ptr(gy), ptr(x), ptr(part), ptr(bs), B, H, W, C, N, 3, 3, 1, 1, 1, N, 9 * C,  # noqa: E731
                                                512, 0, 1, current_stream(dev))
    _entry_point_case(dev, "conv2d_nhwc_wgrad", run, [tol, tol], raw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_attention_dkv(dev, dtype):
    """dK / dV of the attention backward: 8 160 queries in 64 chunks of 4 blocks per (batch, head), 510 keys.  Tolerance:
    test_mfma_gpu.test_attention_forward_backward_vs_fp32_reference (2 % of the range + 1e-4).  The upstream gradient is
    the harsh tensor (the softmax operands have to stay in range)."""
    from refign_amd import _lib, determinism, mfma
    B, heads, Nq, Nkv = 1, 2, 8160, 510
    C = heads * 64
    q = (hashed_uniform((B, Nq, C), "det/q") * 3 - 1.5)
    kv = (hashed_uniform((B, Nkv, 2 * C), "det/kv") * 3 - 1.5)
    q, kv = torch.from_numpy(q).to(dev).to(dtype), torch.from_numpy(kv).to(dev).to(dtype)
    go = _harsh((B, Nq, C), "det/go", dev, dtype, 8 if dtype == torch.bfloat16 else 5)
    nqblk = -(-Nq // 32)
    assert -(-nqblk // mfma._chunk_blocks(nqblk, Nkv, B * heads)) >= 8

    def run():
        qq, kk = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
        mfma.attention(qq, kk, heads, 0.125).backward(go)
        return (kk.grad,)

    def raw(lib):
        try:
            run()
        except RuntimeError as e:
            assert "rfn_attn_bwd_dkv refused in deterministic mode" in str(e), e
            return -4
        return 0
    real = determinism.enabled
    try:                                     # (c): the wrapper is made to choose the atomic form while the library's flag is set
        def raw_default(lib):
            determinism.enabled = lambda: False
            try:
                return raw(lib)
            finally:
                determinism.enabled = real
        _entry_point_case(dev, f"attn_bwd_dkv[{dtype}]", run, [_rel(0.02, 1e-4)], raw_default)
    finally:
        determinism.enabled = real
    assert _lib.load_library().rfn_get_deterministic() == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_batchnorm_statistics(dev, dtype):
    """Forward (fp64) and backward (fp32) statistics of the BatchNorm kernels over 65 536 rows x 256 channels: 512 workgroup rows
    per channel.  The raw sums repeat bit for bit; through bn_act_train the tolerances are those of
    test_mfma_gpu.test_batchnorm_relu_train_kernels (output 4 eps of the range + 1e-3, gradients 2 % + 1e-4 / 1e-3)."""
    from refign_amd import bn as bnk
    from refign_amd._tensor import current_stream, ptr
    B, C, H, W = 4, 256, 128, 128
    kmax = 12 if dtype == torch.bfloat16 else 6
    x = _harsh((B, C, H, W), "det/bnx", dev, dtype, kmax).contiguous(memory_format=torch.channels_last)
    g = _harsh((B, C, H, W), "det/bng", dev, dtype, kmax).contiguous(memory_format=torch.channels_last)
    torch.manual_seed(0)
    bn0 = torch.nn.BatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn0.weight.uniform_(0.5, 1.5)
        bn0.bias.uniform_(-0.5, 0.5)
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11

    def run():
        import copy
        bn = copy.deepcopy(bn0)
        xx = x.clone().requires_grad_(True)
        y = bnk.bn_act_train(xx, bn, True, dtype)
        y.backward(g)
        xh = x.permute(0, 2, 3, 1).contiguous()
        sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
        bnk._stats_fwd(xh, sums)
        bsums = torch.empty((2, C), dtype=torch.float32, device=dev)
        bnk._stats_bwd(xh, g.permute(0, 2, 3, 1).contiguous(), sums, bn0.weight, bn0.bias, bsums, float(bn0.eps), 1)
        return y.detach(), xx.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var, sums, bsums

    xh = x.permute(0, 2, 3, 1).contiguous()
    sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
    raw = lambda lib: lib.rfn_bn_stats_fwd(ptr(xh), ptr(sums), B * H * W, C, bnk._DT16[dtype], current_stream(dev))  # noqa: E731
    tols = [_rel(4 * eps, 1e-3), _rel(0.02, 1e-4), _rel(0.02, 1e-3), _rel(0.02, 1e-3), _rel(1e-6, 1e-4), _rel(1e-4, 1e-5),
            _rel(1e-5), _rel(0.02, 1e-3)]
    _entry_point_case(dev, f"bn_stats[{dtype}]", run, tols, raw)
    from refign_amd import _lib, determinism
    with determinism.deterministic():
        rc = _lib.load_library().rfn_bn_stats_bwd(ptr(xh), ptr(xh), ptr(sums), None, None, ptr(sums), B * H * W, C, 1e-5, 1,
                                                  bnk._DT16[dtype], current_stream(dev))
        assert rc == -4


@pytest.mark.parametrize("B,H,W,C,dil", [(1, 48, 96, 1024, 6), (4, 96, 128, 64, 1)])
def test_depthwise_statistics(dev, B, H, W, C, dil):
    """BatchNorm statistics left behind by the depthwise kernels (with and without storing the convolution), both grid
    geometries (XCD-sliced: 64 block rows per channel slice; first generation: 384 block rows, one image row each).  Tolerance:
    test_dwconv_gpu.test_dwconv_leaves_the_batchnorm_statistics_of_its_result (1e-5 of the sums' scale).
    The atomics here are fp64 adds of fp32 block sums.  With inputs spread over 2^-24 .. 2^24 pixel by pixel the atomic form did
    not differ between launches on an MI355X: every block sum is dominated by its largest elements, the sums share an exponent
    and the fp64 adds are exact.  So the brightness is a function of the image ROW here, 2^-k with k hashed from 0 .. 40, no
    bias, and the shapes are such that a block covers one or two rows: the block sums then span tens of binades (what was
    observed with that: profiles/deterministic_ab.txt, section 2)."""
    from refign_amd import dwconv
    from refign_amd._tensor import current_stream, ptr
    k = torch.from_numpy(np.floor(hashed_uniform((B, H, 1, 1), "det/dwk") * 41)).to(dev)
    x = (_harsh((B, H, W, C), "det/dwx", dev, torch.float32, 1) * torch.exp2(-k)).to(torch.bfloat16)
    g = torch.Generator().manual_seed(C + H)
    w = torch.randn(C, 1, 3, 3, generator=g).to(dev)
    b = None
    bn0 = torch.nn.BatchNorm2d(C).to(dev).train()

    def run():
        import copy
        with torch.no_grad():
            sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
            y = dwconv.dwconv3x3_nhwc(x, w, b, dil, stats=sums)
            bn = copy.deepcopy(bn0)
            z = dwconv.dwconv3x3_bn_act_nhwc(x, w, b, dil, bn, True)
        return y, sums[:C].clone(), sums[C:2 * C].clone(), sums[2 * C:].clone(), z, bn.running_mean, bn.running_var

    def tol_sum(ref):                   # (sum x against the scale of sum x and sqrt(sum x^2), as the existing test)
        return 1e-5 * float(ref.abs().max() + run.scale.sqrt())
    run.scale = run()[2].abs().max()
    sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
    w_tap = w.float().reshape(C, 9).t().contiguous()
    raw = lambda lib: lib.rfn_dwconv3x3_nhwc_stats(ptr(x), ptr(w_tap), ptr(b), ptr(sums), B, H, W, C, dil, 1,  # noqa: E731
                                                   current_stream(dev))
    tols = [_rel(0.0), tol_sum, _rel(1e-5), _rel(0.0), _rel(2.0 ** -7), _rel(1e-6, 1e-7), _rel(1e-6, 1e-7)]
    _entry_point_case(dev, f"dwconv_stats[C={C}, dil={dil}]", run, tols, raw)


def test_dacs_image_mean(dev):
    """The per-image mean behind the contrast jitter (512 x 1024 images: 512 workgroups per image), through the entry points
    themselves so that the mean is seen before it is rounded to fp32.  Tolerance: test_dacs_gpu (1e-5 of max(1, range)), for the
    image and for the mean.  The atomics are fp64 adds of fp32 block sums: on images whose blocks are equally bright every add
    is exact and the atomic form cannot differ, so the brightness of the 1024-pixel blocks spans 2^-40 .. 1 here."""
    import ctypes
    from refign_amd import _lib, dacs, determinism
    from refign_amd._tensor import current_stream, ptr
    B, H, W = 2, 512, 1024
    mean = torch.tensor(dacs.IMNET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(dacs.IMNET_STD, device=dev).view(1, 3, 1, 1)

    def image(key):                                    # de-normalised brightness 2^-k (1 + m) / 2, k per row = per workgroup
        k = torch.from_numpy(np.floor(hashed_uniform((B, 1, H, 1), key + "/k") * 41)).to(dev)
        m = torch.from_numpy(hashed_uniform((B, 3, H, W), key + "/m")).to(dev)
        return ((torch.exp2(-k) * (1 + m) / 2 - mean) / std).contiguous()
    src, trg = image("det/dsrc"), image("det/dtrg")
    gt = torch.from_numpy((hashed_uniform((B, H // 8, W // 8), "det/dgt") * 19).astype(np.int64)).to(dev)
    gt = gt.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    bits = torch.tensor([0b1010101010101010101, 0b0101010101010101010], dtype=torch.int64, device=dev)
    on, order = (ctypes.c_int * B)(*[1] * B), (ctypes.c_int * (4 * B))(*[1, 0, 2, 3] * B)
    fac, hue = (ctypes.c_float * (4 * B))(*[1.1, 0.9, 1.15, 1.0] * B), (ctypes.c_float * (9 * B))(*[1, 0, 0, 0, 1, 0, 0, 0, 1] * B)
    m3, s3 = (ctypes.c_float * 3)(*dacs.IMNET_MEAN), (ctypes.c_float * 3)(*dacs.IMNET_STD)
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    lib = _lib.load_library()

    def call(fn, ws, img):
        return fn(ptr(src), ptr(trg), ptr(gt), None, None, ptr(img), None, None, ptr(ws), B, H, W, ptr(bits), cast(on), cast(order),
                  cast(fac), cast(hue), cast(m3), cast(s3), current_stream(dev))

    def run():
        det = determinism.enabled()
        ws = torch.zeros(lib.rfn_dacs_mix_jitter_det_workspace_bytes(H, W) // 8, dtype=torch.float64, device=dev)
        img = torch.empty_like(src)
        _lib.check(call(lib.rfn_dacs_mix_jitter_det if det else lib.rfn_dacs_mix_jitter, ws, img), "dacs_mix_jitter")
        return img, ws[:B].clone()

    ws, img = torch.empty(8, dtype=torch.float64, device=dev), torch.empty_like(src)
    tol = lambda ref: 1e-5 * max(1.0, float(ref.abs().max()))  # noqa: E731
    _entry_point_case(dev, "dacs_mix_jitter", run, [tol, tol], lambda lib_: call(lib_.rfn_dacs_mix_jitter, ws, img))
    # the Python wrapper takes the same form
    jit = [([1, 0, 2, 3], [1.1, 0.9, 1.15, 1.0], np.eye(3))] * B
    with determinism.deterministic():
        got, _, _ = dacs.mix(src, trg, gt, None, None, bits, jit, [None] * B, part="image")
        assert _bit_equal(got, run()[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_upsample_cross_entropy(dev, dtype):
    """Loss and low-resolution gradient of the fused up-sampling + cross-entropy on a 512 x 1024 label map (4 096 tiles whose
    footprints share their border cells), harsh pixel weights.  Tolerance: test_loss_gpu (loss 1e-5 max(1, |loss|); gradient
    1e-5 of its range in fp32, 2^-7 in bf16)."""
    from refign_amd import seg
    from refign_amd._tensor import current_stream, ptr
    B, C, h, w, H, W = 2, 19, 128, 256, 512, 1024
    logits = (torch.from_numpy(hashed_uniform((B, C, h, w), "det/lg")).to(dev) * 12 - 6).to(dtype)
    target = torch.from_numpy((hashed_uniform((B, H, W), "det/tg") * C).astype(np.int64)).to(dev)
    target[torch.from_numpy(hashed_uniform((B, H, W), "det/ig")).to(dev) < 0.2] = 255
    weight = _harsh((B, H, W), "det/wt", dev)
    crit = seg.PixelWeightedCrossEntropyLoss(255)

    def run():
        lg = logits.clone().requires_grad_()
        loss = crit(seg.DeferredUpsample(lg, (H, W)), target, pixel_weight=weight)
        loss.backward()
        return loss.detach().reshape(1), lg.grad

    grad = torch.empty((B, C, h, w), dtype=torch.float32, device=dev)
    total = torch.empty(64, dtype=torch.float64, device=dev)
    raw = lambda lib: lib.rfn_upsample_ce(ptr(logits), ptr(target), ptr(weight), ptr(grad), ptr(total), B, C, h, w, H, W, 255,  # noqa: E731
                                          seg._CE_DT[dtype], 1, current_stream(dev))
    tols = [lambda ref: 1e-5 * max(1.0, abs(float(ref))), _rel(1e-5 if dtype == torch.float32 else 2.0 ** -7)]
    _entry_point_case(dev, f"upsample_ce[{dtype}]", run, tols, raw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,c,h,w,size,sf", [(2, 19, 128, 256, None, 2), (1, 3, 33, 47, (100, 150), None), (2, 1, 64, 64, (64, 200), None),
                                            (1, 2, 16, 16, None, 8)])
def test_bilinear_backward_gather_kernel(dev, dtype, n, c, h, w, size, sf):
    """The gather-form backward of bilinear up-sampling against ATen's scatter backward in fp32 (its atomic sums are the
    'default form' here: the library never had one).  Bounds from the formats: a cell adds at most (2 / scale + 1)^2 products in
    fp32 (1e-5 of the range); a 16-bit result is that sum rounded once (bf16 2^-8, fp16 2^-11 of the range).  (torch 2.10 does
    not raise for this op under its deterministic switch: F.interpolate then takes an index-based decomposition.  The Function of
    refign_amd.upsample keeps ATen's forward kernel and runs under the switch too.)"""
    from refign_amd import determinism
    from refign_amd.upsample import interpolate_bilinear
    x = _harsh((n, c, h, w), "det/ux", dev, dtype, 4)
    up = F.interpolate(x.float(), size=size, scale_factor=sf, mode="bilinear", align_corners=False)
    go = _harsh(tuple(up.shape), "det/ugo", dev, dtype, 8 if dtype != torch.float16 else 5)
    xr = x.detach().float().clone().requires_grad_(True)
    F.interpolate(xr, size=size, scale_factor=sf, mode="bilinear", align_corners=False).backward(go.float())

    def run():
        xx = x.detach().clone().requires_grad_(True)
        y = interpolate_bilinear(xx, size=size, scale_factor=sf)
        y.backward(go)
        return y.detach(), xx.grad

    with determinism.deterministic():
        outs = _five_launches(dev, run)
        with determinism.torch_deterministic(True):
            under_switch = run()
        assert _bit_equal(under_switch[0], outs[0][0]) and _bit_equal(under_switch[1], outs[0][1])
    for o in outs[1:]:
        assert _bit_equal(o[0], outs[0][0]) and _bit_equal(o[1], outs[0][1])
    assert _bit_equal(outs[0][0], F.interpolate(x, size=size, scale_factor=sf, mode="bilinear", align_corners=False))
    tol = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    err, scale = float((outs[0][1].float() - xr.grad).abs().max()), float(xr.grad.abs().max())
    print(f"\nbilinear backward [{dtype}, {h}x{w} -> {tuple(up.shape[2:])}]: max error {err:.3e} of range {scale:.3e}")
    assert outs[0][1].dtype == dtype and err <= tol * scale
    # outside the mode the call is F.interpolate itself
    xx = x.detach().clone().requires_grad_(True)
    assert type(interpolate_bilinear(xx, size=size, scale_factor=sf).grad_fn).__name__.startswith("UpsampleBilinear2D")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the step
# ---------------------------------------------------------------------------------------------------------------------
def _state(trainer):
    """Everything the guarantee names, as {name: tensor clone}."""
    m, out = trainer.model, {}
    for k in LOSSES:
        v = m.logged[k]
        out["loss/" + k] = (v.detach() if torch.is_tensor(v) else torch.tensor(float(v))).double().reshape(1).cpu()
    for k, v in m.state_dict().items():                         # parameters, EMA parameters, BatchNorm buffers and counters
        out["model/" + k] = v
    # exp_avg, exp_avg_sq, step -- through state_dict(): the fused AdamW keeps its step count on the device and brings the
    # entries up to date there (the step as a plain number: a loaded state holds it in another container than a run's own)
    for i, s in trainer.optimizer.state_dict()["state"].items():
        for k, v in s.items():
            out[f"adam/{i}/{k}"] = torch.tensor(float(v), dtype=torch.float64) if k == "step" else v
    if trainer.scaler is not None:
        for k, v in trainer.scaler.state_dict().items():
            out["scaler/" + k] = torch.as_tensor(v)
    return {k: v.detach().clone() for k, v in out.items()}


def _run(dev, use_hrda, precision, n=8, deterministic=True, after_step=None, H=None, W=None, its=None, trainer=None,
         with_next=False):
    """n steps from _seed(5) -> (trainer, [state after every step])"""
    from refign_amd.trainer import Trainer
    H, W = (H, W) if H else ((128, 128) if use_hrda else (96, 128))
    if trainer is None:
        _seed(5)
        trainer = Trainer(build(use_hrda, dev, enable_fdist=True), precision=precision, deterministic=deterministic)
    states = []
    for it in (range(n) if its is None else its):
        def batch_of(i):
            b = make_batch(2, H, W, 64 if use_hrda else 32, dev)
            b["image_src"] = b["image_src"] + 0.1 * i
            return b
        trainer.step(batch_of(it), it, next_batch=batch_of(it + 1) if with_next else None)
        torch.cuda.synchronize(dev)
        states.append(_state(trainer))
        if after_step is not None:
            after_step(trainer, it)
    return trainer, states


def _assert_same_trajectory(a, b, what):
    assert len(a) == len(b)
    for i, (sa, sb) in enumerate(zip(a, b)):
        assert set(sa) == set(sb)
        bad = [k for k in sa if not _bit_equal(sa[k], sb[k])]
        assert not bad, f"{what}: step {i + 1}: {len(bad)} of {len(sa)} tensors differ, first {bad[:5]}"


STEP_CASES = [("daformer-bf16-graphs", False, "bf16", "1"), ("hrda-bf16-graphs", True, "bf16", "1"),
              ("hrda-fp16-graphs", True, 16, "1"), ("hrda-bf16-eager", True, "bf16", "0")]


@pytest.mark.parametrize("name,use_hrda,precision,graphs", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_step_is_bit_reproducible(dev, monkeypatch, name, use_hrda, precision, graphs):
    """mit_b0, 8 steps from _seed(5), enable_fdist: two models built in one process, both under Trainer(deterministic=True),
    every tensor of _state bit-equal after every step."""
    from refign_amd import _lib
    monkeypatch.setenv("RFN_HIP_GRAPH", graphs)
    ta, a = _run(dev, use_hrda, precision)
    ta.close()
    tb, b = _run(dev, use_hrda, precision)
    tb.close()
    assert _lib.load_library().rfn_get_deterministic() == 0
    assert all(np.isfinite(float(s["loss/" + k])) for s in a for k in LOSSES)
    assert any(not _bit_equal(a[0][k], a[-1][k]) for k in a[0] if k.startswith("model/")), "the model did not train"
    _assert_same_trajectory(a, b, name)


def test_step_with_next_batch_prefetches_is_bit_reproducible(dev):
    """The same with `next_batch=` (what bench.py and a prefetching loader pass): the class histogram, the ImageNet features and
    the matcher's flow of the following batch are computed a step ahead, on streams of their own."""
    ta, a = _run(dev, True, "bf16", n=4, with_next=True)
    ta.close()
    tb, b = _run(dev, True, "bf16", n=4, with_next=True)
    tb.close()
    _assert_same_trajectory(a, b, "hrda-bf16-graphs-next-batch")


# ---------------------------------------------------------------------------------------------------------------------
# 3. across processes
# ---------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import hashlib, json, sys
sys.path[:0] = [{root!r}, {root!r} + "/tests", {root!r} + "/tests/golden"]
import torch
import test_deterministic_gpu as t
dev = torch.device("cuda:0")
tr, states = t._run(dev, True, "bf16")
tr.close()
out = [{{k: hashlib.sha256(t._bits(v).cpu().numpy().tobytes()).hexdigest() for k, v in s.items()}} for s in states]
json.dump(out, open(sys.argv[1], "w"))
"""


def test_two_processes_give_the_same_digests(dev, tmp_path):
    """The HRDA bf16 case in two fresh child processes, one after the other: a SHA-256 per tensor per step, equal."""
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT))
    outs = []
    for i in range(2):
        path = tmp_path / f"digests{i}.json"
        r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, str(script), str(path)], cwd=ROOT,
                           capture_output=True, text=True)
        assert r.returncode == 0, f"child {i} exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"   # (no second start after a failure)
        outs.append(json.load(open(path)))
    assert len(outs[0]) == len(outs[1]) == 8
    for i, (sa, sb) in enumerate(zip(*outs)):
        bad = [k for k in sa if sa[k] != sb[k]]
        assert set(sa) == set(sb) and not bad, f"step {i + 1}: {len(bad)} digests differ, first {bad[:5]}"


# ---------------------------------------------------------------------------------------------------------------------
# 4. exact resume, 5. validation in between
# ---------------------------------------------------------------------------------------------------------------------
def test_resume_is_exact(dev, tmp_path, monkeypatch):
    """The 8-step case of test_resume_gpu._resume_case (HRDA, lr 1e-4, 2 warm-up steps, bf16, captured student passes) under
    deterministic=True: save after step 4, load into a fresh model and trainer, steps 5-8 bit-equal to the uninterrupted run
    in every loss, parameter, buffer and Adam moment."""
    from refign_amd.trainer import Trainer
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")

    def steps(trainer, its):
        out = []
        for it in its:
            _steps(dev, trainer, [it])
            torch.cuda.synchronize(dev)
            out.append(_state(trainer))
        return out

    _seed(5)
    u = Trainer(_model(dev), precision="bf16", deterministic=True)
    full = steps(u, range(8))
    u.close()
    _seed(5)
    a = Trainer(_model(dev), precision="bf16", deterministic=True)
    first = steps(a, range(4))
    path = str(tmp_path / "last.ckpt")
    a.save_checkpoint(path)
    a.close()
    b = Trainer(_model(dev), precision="bf16", deterministic=True, ckpt_path=path)
    rest = steps(b, range(4, 8))
    b.close()
    _assert_same_trajectory(first, full[:4], "before the save")
    _assert_same_trajectory(rest, full[4:], "resumed")


def test_validation_in_between_leaves_the_trajectory_alone(dev):
    """validate() after step 2 of a deterministic run: steps 3-4 bit-equal to a run without it."""
    t0, plain = _run(dev, True, "bf16", n=4)
    t0.close()
    g = torch.Generator().manual_seed(11)
    loader = [{"image": torch.randn(1, 3, 128, 128, generator=g).to(dev), "semantic": torch.randint(0, 19, (1, 128, 128), generator=g).to(dev)}
              for _ in range(2)]
    seen = []

    def after(trainer, it):
        if it == 1:
            seen.append(trainer.validate({"val": loader}))
    t1, with_val = _run(dev, True, "bf16", n=4, after_step=after)
    t1.close()
    assert len(seen) == 1
    _assert_same_trajectory(with_val, plain, "validate() after step 2")


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals, 7. the default is untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from refign_amd import _lib, determinism
    from refign_amd.matching import warp
    from refign_amd.trainer import Trainer
    lib = _lib.load_library()
    model = build(False, dev)
    with pytest.raises(ValueError, match="precision=32"):
        Trainer(model, deterministic=True, precision=32)
    assert lib.rfn_get_deterministic() == 0
    t = Trainer(model, deterministic=True, precision="bf16")
    assert lib.rfn_get_deterministic() == 1 and determinism.enabled()
    # a kernel the mode does not cover: the warp backward of the matcher's training step names itself
    x = torch.randn(1, 4, 16, 16, device=dev, requires_grad=True)
    flow = torch.randn(1, 2, 16, 16, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="rfn_warp_bwd_f32 refused in deterministic mode: warp_bwd_kernel"):
        out = warp(x, flow)
        (out[0] if isinstance(out, tuple) else out).sum().backward()
    t.close()
    assert lib.rfn_get_deterministic() == 0 and not determinism.enabled()


def test_alignment_model_training_step_refuses(dev):
    """AlignmentModel.training_step (+ backward) under the flag: RuntimeError naming the kernel that would have added with
    atomics -- training the matcher is outside the mode."""
    from conftest import golden
    from test_matcher_gpu import build_matcher, matcher_batch
    from refign_amd import determinism
    model = build_matcher(dev)
    batch = matcher_batch(golden("matcher_step_128x160"), dev)
    with determinism.deterministic():
        with pytest.raises(RuntimeError, match=r"refused in deterministic mode: \w+_kernel"):
            model.training_step(batch, 0).backward()
    model.training_step(batch, 0).backward()                 # ... and runs as before outside it


def test_default_mode_calls_no_new_entry_point(dev, monkeypatch):
    """deterministic=False: one HRDA step makes no call to any entry point this mode added, and the flag reads 0 throughout."""
    from refign_amd import _lib
    from refign_amd.trainer import Trainer
    lib = _lib.load_library()
    calls, flags = {}, []
    for name in NEW_ENTRY_POINTS:
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    real_tn = lib.rfn_gemm_tn

    def tn(*a):
        flags.append(lib.rfn_get_deterministic())
        if a[9] == 2:
            calls["rfn_gemm_tn(accumulate=2)"] = calls.get("rfn_gemm_tn(accumulate=2)", 0) + 1
        return real_tn(*a)
    monkeypatch.setattr(lib, "rfn_gemm_tn", tn)
    real_wgrad, wgrads = lib.rfn_conv2d_nhwc_wgrad, []

    def wgrad(*a):                                     # (..., rows_per_slab, accumulate, dtype, stream)
        wgrads.append(a[-3])
        if a[-3] == 2:
            calls["rfn_conv2d_nhwc_wgrad(accumulate=2)"] = calls.get("rfn_conv2d_nhwc_wgrad(accumulate=2)", 0) + 1
        return real_wgrad(*a)
    monkeypatch.setattr(lib, "rfn_conv2d_nhwc_wgrad", wgrad)
    _seed(5)
    t = Trainer(build(True, dev), precision="bf16")
    assert not t.deterministic
    for it in range(2):
        t.step(make_batch(2, 128, 128, 64, dev), it)
        assert lib.rfn_get_deterministic() == 0
    torch.cuda.synchronize(dev)
    t.close()
    assert calls == {}, calls
    assert flags and not any(flags)
    print(f"\ndefault mode: {len(flags)} rfn_gemm_tn and {len(wgrads)} rfn_conv2d_nhwc_wgrad calls seen in two steps")
    assert set(wgrads) <= {0}
    assert not torch.are_deterministic_algorithms_enabled()

"""K5: the fp8 (OCP e4m3) matrix-core kernels of the EMA-teacher path (csrc/f8.hip, refign_amd/f8.py) against fp32 torch
formulations evaluated on the SAME e4m3-rounded operands.  No reference analogue (the reference is 16-bit AMP,
README.md:262); the module semantics checked are mix_transformer.py:79-207.  Tolerances: a bf16 result is within bf16
rounding (2^-8 relative) of the fp32 value; an e4m3 result is within one e4m3 step (2^-3 relative, 2^-9 * scale absolute
in the subnormal range) of the quantised fp32 value, and bit-equal for the overwhelming majority of elements."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn


def _dev():
    return torch.device("cuda:0")


def deq(b):
    return b.view(F8).float()


def torch_quant(x, q):
    return (x.float() * q).clamp(-448, 448).to(F8).view(torch.uint8)


def test_quantize_matches_torch_e4m3fn():
    from refign_amd import f8
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=g) * s for s in (1e-3, 0.05, 1.0, 30.0, 200.0)]).to(_dev(), torch.bfloat16)
    got = f8.quantize(x)
    want = torch_quant(x, f8.ACT_Q)
    assert torch.equal(deq(got), deq(want))          # value-equal (+-0 aside): OCP e4m3, RNE, saturating at 448


GEMM_CASES = [  # M, N, K
    (300, 64, 64), (1000, 256, 64), (513, 128, 128), (777, 320, 320), (2040, 640, 320), (2040, 1280, 320),
    (1111, 320, 1280), (510, 512, 2048), (510, 2048, 512), (4100, 64, 256), (33000, 256, 64), (70000, 512, 256),
    (640, 320, 5120),
]


@pytest.mark.parametrize("M,N,K", GEMM_CASES)
@pytest.mark.parametrize("out_f8", [False, True])
def test_gemm_nt_f8_vs_fp32(M, N, K, out_f8):
    from refign_amd import f8
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(M + 7 * N + 13 * K)
    x = torch.randn(M, K, generator=g).to(dev, torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(dev, torch.bfloat16)
    bias = torch.randn(N, generator=g).to(dev, torch.bfloat16)
    x8 = f8.quantize(x)
    w8 = torch_quant(w, 448.0 / float(w.float().abs().max()))
    ws = torch.full((N,), float(w.float().abs().max()) / 448.0, device=dev) * (1 + torch.arange(N, device=dev) % 3)
    ref = (deq(x8).double() @ deq(w8).double().t()) * (ws.double()[None] / f8.ACT_Q) + bias.double()[None]
    if out_f8:
        got = deq(f8.gemm_nt(x8, w8, ws, bias=bias, act=1, out_f8=True))
        want = torch.relu(ref) * f8.ACT_Q
        wq = deq(want.float().clamp(-448, 448).to(F8).view(torch.uint8))
        assert (got == wq).float().mean() > 0.995
        assert ((got - want.float()).abs() <= want.abs().float() * 0.0626 + 2 ** -9 + 1e-3).all()   # half a step + slack
    else:
        res = torch.randn(M, N, generator=g).to(dev, torch.bfloat16)
        rs = (torch.rand(4, generator=g) + 0.5).to(dev)
        rps = -(-M // 4)
        got = f8.gemm_nt(x8, w8, ws, bias=bias, res=res, rowscale=rs, rows_per_sample=rps).float()
        row = torch.arange(M, device=dev) // rps
        branch = ref.float().to(torch.bfloat16).float()                    # the kernel rounds the branch to bf16 first
        want = res.float() + rs[row][:, None] * branch
        tol = 2 ** -7 * (want.abs() + branch.abs() * rs.max()) + 1e-3
        assert ((got - want).abs() <= tol).all()


def test_quant_rows_matches_amax_scaling():
    from refign_amd import f8
    dev = _dev()
    lin = torch.nn.Linear(320, 1280).to(dev)
    w8, ws = f8.weight(lin.weight)
    wb = lin.weight.detach().to(torch.bfloat16).float()
    amax = wb.abs().amax(1)
    assert torch.allclose(ws, amax / 448.0, rtol=1e-6)
    want = deq((wb / ws[:, None]).clamp(-448, 448).to(F8).view(torch.uint8))
    assert (deq(w8) == want).float().mean() > 0.999       # (1/scale as a multiply vs a divide: rare half-way flips)
    assert ((deq(w8) - want).abs() <= want.abs() * 0.126).all()
    # in-place re-quantisation after the parameter changed
    with torch.no_grad():
        lin.weight.mul_(0.5)
    from refign_amd import params
    params.refresh([lin.weight])
    p0 = w8.data_ptr()
    f8.requantize()
    w8b, wsb = f8.weight(lin.weight)
    assert w8b.data_ptr() == p0
    assert torch.allclose(wsb, amax / 896.0, rtol=1e-6)


@pytest.mark.parametrize("C", [64, 128, 320, 512, 256, 1024])
def test_layernorm_f8(C):
    from refign_amd import f8
    from refign_amd.layernorm import LayerNorm
    dev = _dev()
    torch.manual_seed(C)
    ln = LayerNorm(C, eps=1e-6).to(dev)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.uniform_(-0.5, 0.5)
    x = (torch.randn(3, 1001, C, device=dev) * 2 + 0.3).to(torch.bfloat16)
    got = deq(f8.layernorm(x, ln))
    want = torch.nn.functional.layer_norm(x.float(), (C,), ln.weight, ln.bias, 1e-6) * f8.ACT_Q
    wq = deq(want.clamp(-448, 448).to(F8).view(torch.uint8))
    assert (got == wq).float().mean() > 0.995
    assert ((got - want).abs() <= want.abs() * 0.0626 + 2 ** -9 + 1e-3).all()


@pytest.mark.parametrize("C,H,W", [(256, 17, 23), (512, 34, 60), (1280, 9, 15), (2048, 5, 7)])
def test_dwconv_gelu_f8(C, H, W):
    from refign_amd import f8
    dev = _dev()
    torch.manual_seed(C + H)
    dw = torch.nn.Conv2d(C, C, 3, 1, 1, groups=C).to(dev)
    h = torch.randn(2, H * W, C, device=dev).to(torch.bfloat16)
    h8 = f8.quantize(h)
    got = deq(f8.dwconv_gelu(h8, dw, 2, H, W))
    xin = (deq(h8) / f8.ACT_Q).view(2, H, W, C).permute(0, 3, 1, 2)
    want = torch.nn.functional.gelu(dw(xin)).permute(0, 2, 3, 1).reshape(2, H * W, C) * f8.ACT_Q
    wq = deq(want.clamp(-448, 448).to(F8).view(torch.uint8))
    assert (got == wq).float().mean() > 0.99
    assert ((got - want).abs() <= want.abs() * 0.0626 + 2 ** -9 + 2e-3).all()


@pytest.mark.parametrize("B,heads,N,Nkv", [(2, 1, 300, 64), (1, 2, 1000, 130), (2, 5, 517, 500), (3, 8, 200, 200),
                                           (1, 1, 4000, 510)])
def test_attention_f8_vs_fp32(B, heads, N, Nkv):
    """softmax(scale q k^T) v on e4m3 q / k / v; the kernel re-quantises the probabilities to e4m3 (x 256) for the P.V
    product, so the comparison with the un-quantised softmax carries that rounding (an e4m3 step is 2^-3 relative, i.e.
    3.6 % RMS per probability; the errors of a row add like its terms, so the output carries the same 3-4 % of its own
    RMS whatever the number of keys): |err| <= 4 % of max |v| plus one output step; mean error < 5 % of mean |o|."""
    from refign_amd import f8
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + heads * 100 + N)
    C = heads * 64
    q = torch.randn(B, N, C, generator=g).to(dev, torch.bfloat16)
    kv = torch.randn(B, Nkv, 2 * C, generator=g).to(dev, torch.bfloat16)
    q8, kv8 = f8.quantize(q), f8.quantize(kv)
    got = deq(f8.attention(q8, kv8, heads, 0.125)) / f8.ACT_Q
    qf = (deq(q8) / f8.ACT_Q).view(B, N, heads, 64).transpose(1, 2)
    kf, vf = (deq(kv8) / f8.ACT_Q).view(B, Nkv, 2, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
    want = torch.nn.functional.scaled_dot_product_attention(qf.double(), kf.double(), vf.double(), scale=0.125)
    want = want.transpose(1, 2).reshape(B, N, C).float()
    err = (got - want).abs()
    assert (err <= 0.04 * vf.abs().max() + 0.0626 * want.abs() + 2e-3).all(), float(err.max())
    assert float(err.mean()) < 0.05 * float(want.abs().mean()) + 1e-3


@pytest.mark.parametrize("dim,heads,sr,H,W", [(64, 1, 8, 32, 40), (128, 2, 4, 16, 20), (320, 5, 2, 8, 10), (512, 8, 1, 4, 5)])
def test_block_f8_close_to_bf16_block(dim, heads, sr, H, W):
    """One MiT block (mix_transformer.py:167-207) through the fp8 chain vs the bf16 kernels of the default mode, same
    weights: e4m3 keeps 4 significant bits per operand (3.6 % RMS rounding noise per quantised tensor, and a block
    quantises seven of them in a chain), so the block's update agrees to ~8 % of its RMS; written bound 12 %."""
    from refign_amd import f8, seg
    dev = _dev()
    torch.manual_seed(dim)
    blk = seg.Block(dim, heads, 4, True, sr_ratio=sr, norm_layer=lambda d: seg.LayerNorm(d, eps=1e-6)).to(dev).eval()
    for p in blk.parameters():
        if p.dim() > 1:
            torch.nn.init.normal_(p, std=0.05)
    x = torch.randn(2, H * W, dim, device=dev).to(torch.bfloat16)
    m32 = torch.tensor([[1.0, 1.25], [0.0, 1.1]], device=dev)           # (branch, sample) stochastic-depth scales
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        m16 = m32.to(torch.bfloat16).view(2, 2, 1, 1)
        ref = blk(x, H, W, m16, m32).float()
        f8.reset()
        with f8.teacher_f8():
            got = blk(x, H, W, m16, m32).float()
        assert f8._WEIGHTS, "the fp8 path did not run"
    d_ref = ref - x.float()
    rel = float((got - ref).pow(2).mean().sqrt() / d_ref.pow(2).mean().sqrt())
    assert rel < 0.12, rel


def test_fp8_path_has_no_fallback():
    from refign_amd import f8
    dev = _dev()
    x8 = torch.zeros(8, 24, dtype=torch.uint8, device=dev)              # K % 16 != 0
    with pytest.raises(RuntimeError):
        f8.gemm_nt(x8, x8, torch.ones(8, device=dev))


def _k5_model(dev):
    from refign_amd.align import VGG, UAWarpCHead
    from refign_amd.seg import DAFormerHead, MixVisionTransformer, PixelWeightedCrossEntropyLoss, SegFormerHead
    from refign_amd.uda import DomainAdaptationSegmentationModel
    dims = [64, 128, 320, 512]
    opt = {"class_path": "torch.optim.AdamW", "init_args": {"lr": 6e-5, "weight_decay": 0.01}}
    sch = {"class_path": "helpers.lr_scheduler.LinearWarmupPolynomialLR",
           "init_args": {"warmup_iters": 1500, "warmup_ratio": 1e-6, "power": 1.0, "max_steps": 40000}}
    torch.manual_seed(5)
    model = DomainAdaptationSegmentationModel(
        opt, sch, backbone=MixVisionTransformer("mit_b1", drop_path_rate=0.1),
        head=DAFormerHead(dims, [0, 1, 2, 3], 19, 'multiple_select', dropout_ratio=0.0),
        loss=PixelWeightedCrossEntropyLoss(),
        alignment_backbone=VGG('vgg16', out_indices=[2, 3, 4]),
        alignment_head=UAWarpCHead(in_index=[0, 1], input_transform='multiple_select', estimate_uncertainty=True),
        backbone_lr_factor=0.1, use_refign=True, adapt_to_ref=False, gamma=0.25, enable_fdist=False,
        use_hrda=True, hrda_output_stride=4,
        hrda_scale_attention=SegFormerHead(dims, [0, 1, 2, 3], 19, 'multiple_select', dropout_ratio=0.0))
    with torch.no_grad():                      # decided logits: the 19-class 1x1 of the teacher head gets a visible gain
        model.m_head.conv_seg.weight.mul_(40.0)
    return model.to(dev).train()


def test_k5_teacher_pseudo_labels_agree_with_bf16_teacher(monkeypatch):
    """K5 at step level: teacher forward (HRDA, MiT-b1 widths = MiT-B5's) + align + refine with the teacher's MiT blocks on
    the fp8 kernels vs the default bf16 kernels, same weights, same stochastic-depth draws.  Written bound: refined
    probabilities differ by < 0.03 on average, the pseudo-label argmax agrees on >= 97 % of all pixels and on >= 99.5 % of
    the pixels whose bf16 top-2 margin exceeds 0.2, the confident fraction (p > 0.968, segmentation_model.py:216-224)
    moves by < 0.02."""
    from refign_amd import f8
    monkeypatch.setenv("RFN_HIP_GRAPH", "0")
    dev = _dev()
    model = _k5_model(dev)
    g = torch.Generator(device="cpu").manual_seed(11)
    trg = torch.randn(1, 3, 256, 384, generator=g)
    ref = 0.8 * torch.roll(trg, (2, -3), (2, 3)) + 0.2 * torch.randn(1, 3, 256, 384, generator=g)
    trg, ref = trg.to(dev), ref.to(dev)
    outs = []
    for mode in (False, True):
        model.teacher_f8 = mode
        f8.reset()
        torch.manual_seed(123)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            outs.append(model._teacher_align_refine(trg, ref).float())
        if mode:
            assert f8._WEIGHTS, "the fp8 path did not run"
    p16, p8 = outs
    top2 = p16.topk(2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    agree = (p16.argmax(1) == p8.argmax(1)).float()
    conf16, conf8 = (p16.max(1).values > 0.968).float().mean(), (p8.max(1).values > 0.968).float().mean()
    print("K5 vs bf16 teacher: mean |dp| %.4f, argmax agreement %.4f (decided %.4f, decided fraction %.3f), confident "
          "fraction %.4f vs %.4f" % (float((p16 - p8).abs().mean()), float(agree.mean()),
                                     float(agree[margin > 0.2].mean()), float((margin > 0.2).float().mean()),
                                     float(conf16), float(conf8)))
    assert float((p16 - p8).abs().mean()) < 0.03
    assert float(agree.mean()) >= 0.97
    assert float(agree[margin > 0.2].mean()) >= 0.995
    assert abs(float(conf16) - float(conf8)) < 0.02

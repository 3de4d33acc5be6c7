"""GPU: the fp16 recipe (Trainer(precision=16), the reference's `--trainer.precision 16`): fp16 forms of the LayerNorm,
depthwise, upsample-concat, patchify and cast kernels against fp32 torch, the device-side loss scaler against
torch.amp.GradScaler + torch.optim.AdamW, and whole training steps against the fp32 goldens."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from conftest import golden

pytestmark = pytest.mark.gpu
H16 = torch.float16
U = 2.0 ** -11                 # fp16 unit roundoff (10 stored mantissa bits)


def _rel_err(a, b):
    return float((a.float() - b.float()).abs().max()) / max(float(b.float().abs().max()), 1e-30)


# --- kernel parity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(7, 32), (4097, 320), (513, 512), (33, 1024), (5, 160), (1000, 64)])
@pytest.mark.parametrize("in_dt,out_dt", [(H16, H16), (torch.float32, H16), (H16, torch.float32)])
def test_layernorm_fp16_fwd_bwd(dev, rows, C, in_dt, out_dt):
    """Output and dx within a few fp16 roundings of the normalised value (|y| <~ 5: 8 U |y|max), weight gradients summed in
    fp32 from fp16 inputs (rounding of x and gy: 4 U relative per term)."""
    from refign_amd import mfma
    from refign_amd.layernorm import layer_norm
    mfma.LIBRARY_CALLS.clear()
    g = torch.Generator().manual_seed(rows + C)
    x = (2 * torch.randn(rows, C, generator=g) + 0.5).to(dev).to(in_dt).requires_grad_()
    w = (1 + 0.2 * torch.randn(C, generator=g)).to(dev).requires_grad_()
    b = (0.1 * torch.randn(C, generator=g)).to(dev).requires_grad_()
    gy = torch.randn(rows, C, generator=g).to(dev).to(out_dt)
    y = layer_norm(x, w, b, 1e-6, out_dt)
    assert y.dtype == out_dt
    y.backward(gy)
    xr = x.detach().float().requires_grad_()
    wr, br = w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
    yr = F.layer_norm(xr, (C,), wr, br, 1e-6)
    yr.backward(gy.float())
    assert x.grad.dtype == in_dt
    assert _rel_err(y, yr) <= 8 * U
    assert _rel_err(x.grad, xr.grad) <= 16 * U
    assert _rel_err(w.grad, wr.grad) <= 1e-4 and _rel_err(b.grad, br.grad) <= 1e-4
    assert not mfma.LIBRARY_CALLS


@pytest.mark.parametrize("C", [64, 320, 512])
def test_layernorm_fp16_add_and_add2_sum_in_the_kernel(dev, C):
    """rfn_layernorm_bwd_add / _add2 with fp16 x and gradients == autograd's sums over the fp16 kernels."""
    from refign_amd.layernorm import LayerNorm, layer_norm_pass, layer_norm_pass2
    torch.manual_seed(C)
    ln = LayerNorm(C, eps=1e-6).to(dev)
    x = torch.randn(3, 257, C, device=dev).to(H16)
    g1, g2, g3 = torch.randn_like(x), torch.randn_like(x), torch.randn_like(x)
    xr = x.float().requires_grad_()
    yr = F.layer_norm(xr, (C,), ln.weight.detach(), ln.bias.detach(), 1e-6)
    torch.autograd.backward([yr, xr * 1.0], [g1.float() + g2.float(), g3.float()])
    xa = x.clone().requires_grad_()
    y, y2, xp = layer_norm_pass2(xa, ln.weight, ln.bias, ln.eps)
    torch.autograd.backward([y, y2, xp], [g1, g2, g3])
    assert y.dtype == H16 and _rel_err(y, yr) <= 8 * U
    assert _rel_err(xa.grad, xr.grad) <= 16 * U
    xb = x.clone().requires_grad_()
    y, xp = layer_norm_pass(xb, ln.weight, ln.bias, ln.eps)
    torch.autograd.backward([y, xp], [(g1.float() + g2.float()).to(H16), g3])
    assert _rel_err(xb.grad, xr.grad) <= 16 * U


@pytest.mark.parametrize("B,H,W,C,dil", [(2, 34, 60, 64, 1), (1, 17, 30, 320, 1), (2, 9, 13, 1280, 1), (1, 23, 31, 256, 12),
                                         (2, 19, 7, 64, 6)])
def test_dwconv_fp16_fwd_bwd_wgrad(dev, B, H, W, C, dil):
    """Depthwise 3x3 on fp16 activations (fp32 accumulation) against an fp32 conv2d of the same fp16 inputs: output and data
    gradient to 4 U of the largest value (9-term fp32 sums, one rounding to fp16), weight gradients to 1e-4."""
    from refign_amd.dwconv import dwconv3x3_nhwc
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C + dil)
    x = torch.randn(B, H, W, C, generator=g).to(dev).to(H16).requires_grad_()
    w = (0.3 * torch.randn(C, 1, 3, 3, generator=g)).to(dev).requires_grad_()
    b = (0.1 * torch.randn(C, generator=g)).to(dev).requires_grad_()
    gy = torch.randn(B, H, W, C, generator=g).to(dev).to(H16)
    y = dwconv3x3_nhwc(x, w, b, dil)
    assert y.dtype == H16
    y.backward(gy)
    xr = x.detach().float().permute(0, 3, 1, 2).requires_grad_()
    wr, br = w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
    yr = F.conv2d(xr, wr, br, padding=dil, dilation=dil, groups=C)
    yr.backward(gy.float().permute(0, 3, 1, 2))
    assert _rel_err(y, yr.permute(0, 2, 3, 1)) <= 4 * U
    assert _rel_err(x.grad, xr.grad.permute(0, 2, 3, 1)) <= 4 * U
    assert _rel_err(w.grad, wr.grad) <= 1e-4 and _rel_err(b.grad, br.grad) <= 1e-4


@pytest.mark.parametrize("B,H,W,C,dil", [(2, 20, 28, 1024, 6), (3, 9, 13, 1280, 1), (2, 17, 30, 64, 1)])
def test_dwconv_fp16_stats_and_gradient_free_bn_relu(dev, B, H, W, C, dil):
    """The statistics of the stored fp16 result (STATS) and the two-pass gradient-free depthwise + BatchNorm + ReLU on fp16."""
    import copy
    from refign_amd import bn as bnk
    from refign_amd.dwconv import dwconv3x3_bn_act_nhwc, dwconv3x3_nhwc
    g = torch.Generator().manual_seed(C + H + dil)
    x = (torch.randn(B, H, W, C, generator=g) + 0.3).to(dev).to(H16)
    w = torch.randn(C, 1, 3, 3, generator=g).to(dev)
    b = torch.randn(C, generator=g).to(dev)
    with torch.no_grad():
        want = dwconv3x3_nhwc(x, w, b, dil)
        sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
        got = dwconv3x3_nhwc(x, w, b, dil, stats=sums)
    assert got.dtype == H16 and torch.equal(got, want)
    wf = want.double().reshape(-1, C)
    assert float(sums[2 * C]) == B * H * W
    assert torch.allclose(sums[:C], wf.sum(0), rtol=1e-6, atol=1e-6 * float(wf.abs().sum(0).max()))
    assert torch.allclose(sums[C:2 * C], (wf * wf).sum(0), rtol=1e-6)
    bn_a = torch.nn.BatchNorm2d(C).to(dev).train()
    with torch.no_grad():
        bn_a.weight.copy_(torch.rand(C, generator=g).to(dev) + 0.5)
        bn_a.bias.copy_(torch.randn(C, generator=g).to(dev))
    bn_b = copy.deepcopy(bn_a)
    with torch.no_grad():
        got = dwconv3x3_bn_act_nhwc(x, w, b, dil, bn_a, True)
        ref = F.relu(bn_b(want.float().permute(0, 3, 1, 2))).permute(0, 2, 3, 1)
    assert got.dtype == H16 and _rel_err(got, ref) <= 4 * U
    assert torch.allclose(bn_a.running_mean, bn_b.running_mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(bn_a.running_var, bn_b.running_var, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("n,sizes,chans,out", [(2, [(34, 60), (17, 30), (9, 15), (5, 8)], [64, 128, 320, 512], (34, 60)),
                                               (1, [(24, 32), (12, 16), (6, 8), (3, 4)], [64, 128, 320, 512], (24, 32))])
def test_upsample_concat_fp16_fwd_bwd(dev, n, sizes, chans, out):
    """The decode head's bilinear upsample + concat in fp16 (fp32 blend) against F.interpolate in fp32 of the same inputs."""
    from refign_amd.upcat import upsample_concat
    g = torch.Generator().manual_seed(sum(chans) + out[0])
    maps = [torch.randn(n, h * w, c, generator=g).to(dev).to(H16).requires_grad_() for (h, w), c in zip(sizes, chans)]
    y = upsample_concat(maps, sizes, out)                 # (n, sum C, H, W), channels-last
    assert y is not None and y.dtype == H16
    gy = torch.randn(y.shape, generator=g).to(dev).to(H16)
    y.backward(gy)
    refs = [m.detach().float().requires_grad_() for m in maps]
    parts = [F.interpolate(r.view(n, h, w, c).permute(0, 3, 1, 2), size=out, mode="bilinear", align_corners=False)
             for r, (h, w), c in zip(refs, sizes, chans)]
    yr = torch.cat(parts, 1)
    yr.backward(gy.float())
    assert _rel_err(y, yr) <= 2 * U
    for m, r in zip(maps, refs):
        assert m.grad.dtype == H16 and _rel_err(m.grad, r.grad) <= 4 * U


@pytest.mark.parametrize("B,H,W,C,r", [(2, 68, 120, 64, 8), (1, 34, 61, 128, 4), (2, 17, 30, 320, 2)])
@pytest.mark.parametrize("cmajor", [False, True])
def test_patchify_fp16_is_the_permutation(dev, B, H, W, C, r, cmajor):
    """The spatial-reduction patchify (a pure move) on fp16 tokens == torch's reshape / permute; inverse too."""
    from refign_amd.conv import _from_patches, _to_patches
    x = torch.randn(B, H * W, C, device=dev).to(H16)
    got, Hr, Wr = _to_patches(x, H, W, r, cmajor)
    v = x.view(B, H, W, C)[:, :Hr * r, :Wr * r]
    order = (0, 1, 3, 5, 2, 4) if cmajor else (0, 1, 3, 2, 4, 5)
    want = v.reshape(B, Hr, r, Wr, r, C).permute(*order).reshape(B * Hr * Wr, r * r * C)
    assert torch.equal(got, want)
    back = _from_patches(got, B, H, W, C, r, Hr, Wr, cmajor)
    keep = torch.zeros(B, H, W, C, dtype=torch.bool, device=dev)
    keep[:, :Hr * r, :Wr * r] = True
    assert torch.equal(back.view(B, H, W, C)[keep], x.view(B, H, W, C)[keep])
    assert not back.view(B, H, W, C)[~keep].any()


def test_fp16_parameter_copies_are_bit_equal_to_torch_casts(dev):
    """params.refresh: the multi-tensor fp32 -> fp16 cast and the transposed fp16 copies == tensor.to(torch.float16),
    overflow to inf included."""
    from refign_amd.params import as_dtype, refresh, transposed
    torch.manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(n, k, device=dev) * 300.0) for n, k in
          ((64, 33), (320, 128), (7, 5), (512, 2048), (130, 66), (8, 8))]
    with torch.no_grad():
        ps[0][0, :4] = torch.tensor([70000.0, -1e-8, 65519.0, 65520.0])
    for p in ps:
        as_dtype(p, H16), transposed(p, H16)
    with torch.no_grad():
        for p in ps:
            p.mul_(1.5).add_(0.25)
            p.data[0, 0] = 1e6
    refresh(ps, plan_key=("amp16-test", 0))
    for p in ps:
        assert torch.equal(as_dtype(p, H16), p.detach().to(H16))
        assert torch.equal(transposed(p, H16), p.detach().to(H16).t().contiguous())


@pytest.mark.parametrize("S,n", [(3, 64), (64, 320), (65, 128), (8160, 512), (259, 1024)])
def test_bias_gradient_sums_of_fp16_rows(dev, S, n):
    """params.sum_rows on fp16 rows (flat S <= 64 and tall two-stage kernels) == an fp64 column sum of the same values."""
    from refign_amd.params import sum_rows
    x = (torch.randn(S, n, device=dev) * 100).to(H16)
    got = sum_rows(x)
    want = x.double().sum(0)
    assert got.dtype == torch.float32
    assert float((got.double() - want).abs().max()) <= 1e-6 * float(x.double().abs().sum(0).max())


# --- loss scaler against torch --------------------------------------------------------------------------------------------
def test_loss_scaler_and_adamw_match_torch_grad_scaler(dev):
    """The device-side scaler (unscale + check, AdamW skipped on the device, scale update) through the Trainer's optimizer proxy
    against torch.amp.GradScaler + a non-fused torch.optim.AdamW, on identical scaled gradients: clean steps, an inf and a NaN
    gradient (skipped: nothing changes), growth after growth_interval = 3 clean steps, and equal state_dicts."""
    from types import SimpleNamespace
    from refign_amd.amp import LossScaler
    from refign_amd.optim import MultiTensorAdamW
    from refign_amd.trainer import FlatGradBuffer, _OptimizerProxy
    torch.manual_seed(3)
    shapes = [(64, 33), (320,), (7, 5, 3), (1000,), (2, 2)]
    init = [torch.randn(s, device=dev) for s in shapes]
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    qs = [torch.nn.Parameter(t.clone()) for t in init]
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opt = torch.optim.AdamW([{"params": ps[:3]}, {"params": ps[3:], "lr": 5e-4}], fused=True, **kw)
    ref = torch.optim.AdamW([{"params": qs[:3]}, {"params": qs[3:], "lr": 5e-4}], foreach=False, **kw)
    grads = FlatGradBuffer(ps)
    sargs = dict(init_scale=2.0 ** 10, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    t = SimpleNamespace(grads=grads, bucket_mb=64, scaler=LossScaler(dev, **sargs), fast_step=MultiTensorAdamW(opt),
                        optimizer=opt)
    proxy = _OptimizerProxy(t)
    gs = torch.amp.GradScaler("cuda", **sargs)
    bad = {0: float("inf"), 3: float("inf"), 5: float("nan")}      # k = 0: torch's own first step, skipped on the host
    for k in range(10):
        g = [torch.randn(s, device=dev) for s in shapes]
        if k in bad:
            g[1][7] = bad[k]
        before = [p.detach().clone() for p in ps] + [opt.state[p][n].clone() for p in ps if p in opt.state
                                                      for n in ("exp_avg", "exp_avg_sq")]
        proxy.zero_grad()
        for p, gi in zip(ps, g):
            p.grad.copy_(gi * t.scaler._scale)
        for q, gi in zip(qs, g):
            q.grad = gs.scale(gi)
        proxy.step()
        gs.step(ref)
        gs.update()
        if k == 0:
            assert opt._opt_called and not opt.state          # skipped, and the LR scheduler may advance without a warning
        if k in bad:
            after = [p.detach() for p in ps] + [opt.state[p][n] for p in ps if p in opt.state for n in ("exp_avg", "exp_avg_sq")]
            assert all(torch.equal(a, b) for a, b in zip(before, after)), k
        assert t.scaler.get_scale() == gs.get_scale(), k
        for p, q in zip(ps, qs):
            torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-6, atol=1e-7)
            if q in ref.state:                            # (fused first step vs foreach: ulp-level differences)
                for n in ("exp_avg", "exp_avg_sq"):
                    want = ref.state[q][n]
                    torch.testing.assert_close(opt.state[p][n], want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))
        # after the step p.grad holds unscaled gradients, as GradScaler leaves them
        if k not in bad:
            torch.testing.assert_close(ps[0].grad, qs[0].grad, rtol=0, atol=0)
    assert t.fast_step.launches >= 6                      # the device path took the steps after torch's first
    sd = opt.state_dict()
    rd = ref.state_dict()
    assert [float(sd["state"][i]["step"]) for i in sd["state"]] == [float(rd["state"][i]["step"]) for i in rd["state"]] == [7.0] * 5
    assert t.scaler.state_dict() == gs.state_dict()
    assert t.scaler.skipped_steps() == 3
    s2 = LossScaler(dev)
    s2.load_state_dict(gs.state_dict())
    assert s2.state_dict() == gs.state_dict()


# --- whole step against the fp32 goldens -------------------------------------------------------------------------------
@pytest.mark.parametrize("use_hrda,name,blk", [(False, "step_daformer_96x128", 32), (True, "step_hrda_128x128", 64)])
def test_fp16_recipe_step_is_bounded_against_fp32_reference(dev, use_hrda, name, blk):
    """Trainer(precision=16) -- fp16 autocast entered by the trainer, loss scaled by 2^16, gradients unscaled on the device --
    through the golden training step, with the bounds of the bf16 bench-mode test (test_step_gpu.py): losses within 3 %,
    group gradient norms within 10 %, pseudo-label agreement with the fp32 run >= 97 %, confident fraction +- 0.02,
    EMA / live checksums within 1e-4.  The step must not be skipped, and fp16 sends nothing to a dense library that the
    bf16 recipe (Trainer(precision="bf16")) keeps on the hand-written kernels: the same calls, the same shapes (mit_b0's
    32- and 160-wide layers are outside the GEMM kernels' K % 64 domain in either dtype).
    Measured on an MI355X: see the printed line (losses / norms / agreement of each golden)."""
    from test_step_gpu import build, make_batch
    from refign_amd import mfma
    from refign_amd.trainer import Trainer
    g = golden(name)
    H, W = [int(v) for v in g["size"]]
    seen = {}
    lib = {}
    for mode in ("fp32", "bf16", "fp16"):
        model = build(use_hrda, dev)
        trainer = Trainer(model, fused_optimizer=False, precision={"fp32": 32, "bf16": "bf16-mixed", "fp16": "16-mixed"}[mode])
        trainer.scheduler = torch.optim.lr_scheduler.LambdaLR(trainer.optimizer, lambda s_: 1.0)
        model._scheduler = trainer.scheduler
        batch = make_batch(2, H, W, blk, dev)
        random.seed(77); np.random.seed(77); torch.manual_seed(77)
        model.global_step = 3
        norms, probs = {}, {}
        real_step, real_mix = trainer.optimizer.step, model.get_dacs_mix

        def recording_step(*a, **k):
            norms["v"] = [float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in grp["params"])))
                          for grp in trainer.optimizer.param_groups]
            return real_step(*a, **k)

        def recording_mix(images_trg, probs_trg, *a, **k):
            probs["p"] = probs_trg.detach().float().clone()
            return real_mix(images_trg, probs_trg, *a, **k)

        trainer.optimizer.step, model.get_dacs_mix = recording_step, recording_mix
        mfma.LIBRARY_CALLS.clear()
        trainer.step(batch, 0)
        lib[mode] = {(kind, shapes): n for (kind, _, shapes), n in mfma.LIBRARY_CALLS.items()}
        if mode == "fp16":
            assert trainer.scaler.skipped_steps() == 0 and "v" in norms
            assert lib["fp16"] == lib["bf16"], mfma.library_summary()
        losses = np.array([float(model.logged[k]) for k in ("train_loss_src", "train_loss_featdist_src",
                                                            "train_loss_uda_trg")])
        seen[mode] = (losses, np.array(norms["v"]), probs["p"],
                      float(sum(p.double().abs().sum() for p in model.ema_parameters())),
                      float(sum(p.double().abs().sum() for p in model.live_parameters())))
        trainer.close()
    losses, norms, probs, ema, live = seen["fp16"]
    p32 = seen["fp32"][2]
    agree = float((probs.argmax(1) == p32.argmax(1)).float().mean())
    w16 = float((probs.max(1)[0] >= 0.968).float().mean())
    w32 = float((p32.max(1)[0] >= 0.968).float().mean())
    print(f"\nfp16-recipe step vs fp32: losses {losses} (golden {g['losses']}), grad norms {norms} (golden {g['grad_norms']}), "
          f"pseudo-label agreement {agree:.4f}, confident fraction {w16:.4f} vs {w32:.4f}")
    np.testing.assert_allclose(losses, g["losses"], rtol=3e-2)
    np.testing.assert_allclose(norms, g["grad_norms"], rtol=1e-1)
    assert agree >= 0.97 and abs(w16 - w32) <= 0.02
    assert abs(ema - float(g["ema_abs_sum"])) < 1e-4 * float(g["ema_abs_sum"])
    assert abs(live - float(g["live_abs_sum"])) < 1e-4 * float(g["live_abs_sum"])

"""GPU: the fp16 recipe (Trainer(precision=16)) on the MiT-B5 golden step, under hipGraph capture and replay, and the fp16
form of the teacher's fused Mix-FFN front half."""
import random

import numpy as np
import pytest
import torch
from conftest import golden
from test_step_gpu import build, make_batch

pytestmark = pytest.mark.gpu
H16 = torch.float16


def _b5_step(dev, precision, seed=78):
    """one Trainer.step of the MiT-B5 + HRDA model on the 512 x 512 G13 batch (what test_step_gpu._b5_step records, driven
    through Trainer(precision=...)) + the pseudo-label probabilities, the dense library calls and the skipped-step count"""
    from refign_amd import mfma
    from refign_amd.trainer import Trainer
    model = build(True, dev, "mit_b5", [64, 128, 320, 512])
    trainer = Trainer(model, fused_optimizer=False, precision=precision)
    trainer.scheduler = torch.optim.lr_scheduler.LambdaLR(trainer.optimizer, lambda s_: 1.0)
    model._scheduler = trainer.scheduler
    batch = make_batch(1, 512, 512, 64, dev)
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    model.global_step = 3
    seen = {}
    real_step, real_mix = trainer.optimizer.step, model.get_dacs_mix

    def recording_step(*a, **k):
        seen["norms"] = np.array([float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in grp["params"])))
                                  for grp in trainer.optimizer.param_groups])
        seen["conv_seg"] = model.head.conv_seg.weight.grad.detach().float().flatten()[::37].cpu().numpy()
        seen["fc1"] = model.backbone.block3[20].mlp.fc1.weight.grad.detach().float().flatten()[::997].cpu().numpy()
        return real_step(*a, **k)

    def recording_mix(images_trg, probs_trg, *a, **k):
        seen["probs"] = probs_trg.detach().float().clone()
        return real_mix(images_trg, probs_trg, *a, **k)

    trainer.optimizer.step, model.get_dacs_mix = recording_step, recording_mix
    mfma.LIBRARY_CALLS.clear()
    trainer.step(batch, 0)
    seen["library"] = mfma.library_summary()
    seen["skipped"] = trainer.scaler.skipped_steps() if trainer.scaler is not None else 0
    seen["losses"] = np.array([float(model.logged.get(k, 0.0)) for k in ("train_loss_src", "train_loss_featdist_src",
                                                                         "train_loss_uda_trg")])
    seen["ema"] = float(sum(p.double().abs().sum() for p in model.ema_parameters()))
    seen["live"] = float(sum(p.double().abs().sum() for p in model.live_parameters()))
    trainer.close()
    return seen


def test_fp16_recipe_mit_b5_hrda_512_step_is_bounded(dev):
    """G13-B5 (MiT-B5 + HRDA, 512 x 512) under Trainer(precision=16), with the bounds of the bf16 bench-mode test
    (test_step_gpu.py::test_training_step_mit_b5_hrda_512_bench_mode_is_bounded) against the reference's fp32 CPU values:
      three losses                within 1 %,
      per-group gradient norms    within 5 %,
      sampled gradients           decode-head class weights within 5 %, one stage-3 fc1 within 20 % of the largest entry,
      EMA / student checksums     within 1e-4 relative,
      pseudo-labels               argmax agreement with this repo's fp32 run >= 95 %, confident fraction +- 0.02;
    no skipped step, and no dense call leaves the hand-written kernels (every MiT-B5 width is inside their domain).
    Measured on an MI355X: loss deviation 9.5e-5, 5.1e-5, 4.4e-5; gradient-norm deviation 0.001 %, 0.014 %, 0.04 %, 0.26 %;
    sampled gradients conv_seg 0.10 %, fc1 1.7 % (the bf16 map: 0.9 %, 10.6 %); agreement 0.996; checksums 1.4e-12, 7.0e-10."""
    g = golden("step_hrda_b5_512x512")
    f32 = _b5_step(dev, 32)
    hm = _b5_step(dev, 16)
    dl = np.abs(hm["losses"] / g["losses"] - 1)
    dn = np.abs(hm["norms"] / g["grad_norms"] - 1)
    dg = {k: float(np.abs(hm[k] - g["grad_" + k]).max() / np.abs(g["grad_" + k]).max()) for k in ("conv_seg", "fc1")}
    agree = float((hm["probs"].argmax(1) == f32["probs"].argmax(1)).float().mean())
    w16 = float((hm["probs"].max(1)[0] >= 0.968).float().mean())
    w32 = float((f32["probs"].max(1)[0] >= 0.968).float().mean())
    print(f"\nMiT-B5 HRDA fp16-recipe step vs reference fp32: loss deviation {dl}, grad-norm deviation {dn}, sampled gradients "
          f"{dg}, pseudo-label agreement {agree:.4f}, confident fraction {w16:.4f} vs {w32:.4f}, "
          f"checksums {hm['ema'] / float(g['ema_abs_sum']) - 1:.2e} / {hm['live'] / float(g['live_abs_sum']) - 1:.2e}")
    assert hm["skipped"] == 0
    assert hm["library"] == {}, hm["library"]
    assert dl.max() <= 1e-2 and dn.max() <= 5e-2
    assert dg["conv_seg"] <= 5e-2 and dg["fc1"] <= 2e-1
    assert agree >= 0.95 and abs(w16 - w32) <= 0.02
    assert abs(hm["ema"] - float(g["ema_abs_sum"])) < 1e-4 * float(g["ema_abs_sum"])
    assert abs(hm["live"] - float(g["live_abs_sum"])) < 1e-4 * float(g["live_abs_sum"])


# --- graphs -------------------------------------------------------------------------------------------------------------
def _fp16_steps(dev, model, trainer, steps, seed, start=0):
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    rows, scales = [], []
    for it in range(start, start + steps):
        batch = make_batch(2, 128, 128, 64, dev)
        batch["image_src"] = batch["image_src"] + 0.1 * it
        trainer.step(batch, it)
        rows.append([float(model.logged[k]) for k in ("train_loss_src", "train_loss_featdist_src", "train_loss_uda_trg")])
        scales.append(trainer.scaler.get_scale())
    return np.array(rows), scales, float(sum(p.double().abs().sum() for p in model.live_parameters()))


def test_fp16_graph_replay_equals_eager_across_scale_changes(dev, monkeypatch):
    """Under Trainer(precision=16) the student's passes are captured at step 3 with the loss scale read from device memory; the
    scale grows after every 2 clean steps (growth_interval=2), so the later steps replay with scales the capture never saw.
    6 steps graphed == 6 steps eager: the same losses, the same scale sequence, the same parameters."""
    from refign_amd.trainer import Trainer
    traj = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RFN_GRAPH_STUDENT", mode)
        model = build(True, dev)
        trainer = Trainer(model, fused_optimizer=False, precision=16, scaler_args={"init_scale": 2.0 ** 10, "growth_interval": 2})
        traj[mode] = _fp16_steps(dev, model, trainer, 6, 5)
        if mode == "1":
            for name in ("source_pass", "mixed_pass"):
                st = list(model._graphs[name].states.values())
                assert len(st) == 1 and st[0]["graph"] is not None and not st[0]["failed"], f"{name}: not captured"
        trainer.close()
    scales = traj["1"][1]
    assert scales == traj["0"][1] and len(set(scales[2:])) > 1, scales        # the scale changed after the capture
    np.testing.assert_allclose(traj["1"][0], traj["0"][0], rtol=2e-3)
    assert abs(traj["1"][2] - traj["0"][2]) < 1e-5 * traj["0"][2]


def test_fp16_steps_after_bf16_steps_equal_a_fresh_model(dev, monkeypatch):
    """4 bf16 steps (Trainer(precision="bf16"): bf16 student graphs captured, bf16 weight copies in the refresh plans), then 4
    fp16 steps on the same model == the same 4 fp16 steps on a freshly built model holding the same weights: captures are keyed
    on the autocast dtype and never replay across dtypes (the fp16 passes are captured anew), the fp16 copies are refreshed
    next to the bf16 ones."""
    from refign_amd.trainer import Trainer
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    a = build(True, dev)
    ta = Trainer(a, fused_optimizer=False, precision="bf16")
    random.seed(8); np.random.seed(8); torch.manual_seed(8)
    for it in range(4):
        ta.step(make_batch(2, 128, 128, 64, dev), it)
    ta.close()
    assert any(k for k in a._graphs["source_pass"].states), "no bf16 capture to stay away from"
    b = build(True, dev)
    b.load_state_dict(a.state_dict())
    b.global_step = a.global_step
    out = {}
    for name, m in (("after_bf16", a), ("fresh", b)):
        tr = Trainer(m, fused_optimizer=False, precision=16)
        out[name] = _fp16_steps(dev, m, tr, 4, 9, start=4)
        tr.close()
    np.testing.assert_allclose(out["after_bf16"][0], out["fresh"][0], rtol=2e-3)
    assert out["after_bf16"][1] == out["fresh"][1]
    assert abs(out["after_bf16"][2] - out["fresh"][2]) < 1e-5 * out["fresh"][2]


# --- the teacher's fused kernels in fp16 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("views,H,W,C", [(3, 17, 30, 512), (2, 34, 60, 320), (2, 7, 45, 128), (1, 135, 240, 64), (1, 1, 1, 128),
                                         (2, 68, 120, 128)])
def test_fused_mix_ffn_front_half_fp16(dev, views, H, W, C):
    """rfn_ffn_fc1_dw_gelu_f16 (fp16 MFMA, fp16 hidden tile) on the four MiT-B5 widths, ragged tiles, several views == the three
    fp16 kernels (GEMM with fp16 store, depthwise + GELU) to a few fp16 rounding steps, and == the fp32 formulation of the same
    fp16-rounded hidden map; twice, bit-identical."""
    from refign_amd import dwconv
    from refign_amd.seg import Mlp
    torch.manual_seed(C + H)
    mlp = Mlp(C, 4 * C).to(dev).eval()
    with torch.no_grad():
        for p in mlp.parameters():
            p.mul_(2.0)
        mlp.dwconv.dwconv.bias.normal_(0, 0.5)
        mlp.fc1.bias.normal_(0, 0.5)
    x = torch.randn(views, H * W, C, device=dev).to(H16)
    with torch.no_grad(), torch.autocast("cuda", dtype=H16):
        a = dwconv.ffn_fc1_dw_gelu(x, mlp.fc1, mlp.dwconv.dwconv, H, W)
        assert a is not None and a.dtype == H16 and tuple(a.shape) == (views, H * W, 4 * C)
        assert torch.equal(a, dwconv.ffn_fc1_dw_gelu(x, mlp.fc1, mlp.dwconv.dwconv, H, W))
        h = mlp.fc1(x)
        assert h.dtype == H16
        want = dwconv.dwconv3x3_gelu_tokens(h, mlp.dwconv.dwconv.weight, mlp.dwconv.dwconv.bias, H, W)
    d = (a.float() - want.float()).abs()
    scale = float(want.float().abs().max())
    assert float(d.max()) <= 2.0 ** -9 * scale and float(d.mean()) <= 3e-5 * scale, (float(d.max()), float(d.mean()), scale)
    hf = torch.nn.functional.linear(x.float(), mlp.fc1.weight, mlp.fc1.bias).to(H16).float()
    hf = hf.transpose(1, 2).reshape(views, 4 * C, H, W)
    ref = torch.nn.functional.gelu(torch.nn.functional.conv2d(hf, mlp.dwconv.dwconv.weight, mlp.dwconv.dwconv.bias, padding=1,
                                                              groups=4 * C)).flatten(2).transpose(1, 2)
    assert float((a.float() - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max())

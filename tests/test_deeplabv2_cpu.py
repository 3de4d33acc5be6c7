"""CPU: the DeepLabV2 family (refign_amd/resnet.py: ResNet-v1c, DeepLabV2Head) and its opt-in (config.FAMILIES) against the
fixtures of tests/golden/make_golden_deeplabv2.py: state_dict manifest, fp32 forward of the three depths, train-mode running
statistics, head forward and gradients on the per-branch path, the live-tap table, frozen stages / norm_eval."""
import glob
import json
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN, golden
from fill import closed_form_fill, hashed_uniform

REF_CONFIGS = sorted(glob.glob("/root/reference/configs/*/refign_deeplabv2.yaml"))
CFG = {"strides": (1, 2, 1, 1), "dilations": (1, 1, 2, 4)}
SAMPLE = (slice(None), slice(None, None, 8), slice(None, None, 2), slice(None, None, 2))

# the `model:` / `optimizer:` / `lr_scheduler:` sections of configs/cityscapes_acdc/refign_deeplabv2.yaml, pretrained files nulled
MODEL_CFG = {
    "model": {"class_path": "models.DomainAdaptationSegmentationModel", "init_args": {
        "backbone_lr_factor": 0.1, "enable_fdist": True, "use_refign": True, "adapt_to_ref": True, "gamma": 0.25,
        "backbone": {"class_path": "models.backbones.ResNet", "init_args": {
            "pretrained": None, "model_type": "resnet101_v1c", "strides": [1, 2, 1, 1], "dilations": [1, 1, 2, 4]}},
        "head": {"class_path": "models.heads.DeepLabV2Head", "init_args": {"in_channels": 2048, "in_index": 3, "num_classes": 19}},
        "alignment_backbone": {"class_path": "models.backbones.VGG", "init_args": {
            "model_type": "vgg16", "pretrained": None, "out_indices": [2, 3, 4]}},
        "alignment_head": {"class_path": "models.heads.UAWarpCHead", "init_args": {
            "in_index": [0, 1], "input_transform": "multiple_select", "estimate_uncertainty": True, "pretrained": None}},
        "loss": {"class_path": "models.losses.PixelWeightedCrossEntropyLoss"}}},
    "optimizer": {"class_path": "torch.optim.AdamW", "init_args": {"lr": 0.0006, "weight_decay": 0.01}},
    "lr_scheduler": {"class_path": "helpers.lr_scheduler.LinearWarmupPolynomialLR", "init_args": {
        "warmup_iters": 1500, "warmup_ratio": 0.000001, "power": 1.0, "max_steps": 40000}},
}


def _check_built(model):
    from refign_amd import resnet
    assert type(model).__name__ == "DomainAdaptationSegmentationModel"
    assert isinstance(model.backbone, resnet.ResNet) and isinstance(model.head, resnet.DeepLabV2Head)
    assert isinstance(model.m_backbone, resnet.ResNet) and isinstance(model.imnet_backbone, resnet.ResNet)
    (opt,), (sch,) = model.configure_optimizers()
    assert isinstance(opt, torch.optim.AdamW) and type(sch).__name__ == "LinearWarmupPolynomialLR"
    # decay / no-decay x head / backbone (lr factor 0.1): the reference's four groups, sized as its step fixture recorded them
    groups = model.optimizer_parameters()
    assert [g["name"] for g in groups] == ["head_weight", "head_bias", "backbone_weight", "backbone_bias"]
    assert [len(g["params"]) for g in groups] == [4, 4, 106, 212] == list(golden("step_deeplabv2_96x128")["groups"])
    assert groups[2]["lr"] == 0.1 * groups[0]["lr"] and groups[1]["weight_decay"] == 0 == groups[3]["weight_decay"]
    assert len(opt.param_groups) == 4
    assert not any(p.requires_grad for m in (model.m_backbone, model.m_head, model.imnet_backbone) for p in m.parameters())
    model.train()
    assert model.backbone.training and model.m_backbone.training and not model.imnet_backbone.training


def test_opt_in_builds_the_family_and_the_plain_call_still_refuses():
    from refign_amd import config
    before = dict(config.ALIASES)
    with pytest.raises(config.OutOfScopeError, match="out of scope") as e:
        config.build_model(MODEL_CFG)
    assert "deeplabv2" in str(e.value) and "families" in str(e.value)          # the refusal names the opt-in
    _check_built(config.build_model(MODEL_CFG, families=("deeplabv2",)))
    assert config.ALIASES == before                                            # nothing remembered: the next plain call refuses again
    with pytest.raises(config.OutOfScopeError, match="out of scope"):
        config.build_model(MODEL_CFG)
    with pytest.raises(config.OutOfScopeError, match="out of scope"):
        config.build_model(MODEL_CFG, families=())
    with pytest.raises(ValueError, match="unknown model family"):
        config.build_model(MODEL_CFG, families=("deeplabv3",))
    assert set(config.FAMILIES) == {"deeplabv2"}
    assert config.FAMILIES["deeplabv2"] == {"models.backbones.ResNet": "refign_amd.resnet.ResNet",
                                            "models.heads.DeepLabV2Head": "refign_amd.resnet.DeepLabV2Head"}


@pytest.mark.parametrize("name", ["cityscapes_acdc", "cityscapes_darkzurich", "cityscapes_robotcar"])
def test_reference_deeplabv2_yaml_builds_through_the_opt_in(name):
    path = next((p for p in REF_CONFIGS if f"/{name}/" in p), None)
    if path is None:
        pytest.skip(f"reference checkout not present (configs/{name}/refign_deeplabv2.yaml)")
    from refign_amd import config
    cfg = config.load_config(path)
    over = {f"{k}.init_args.pretrained": None for k in ("backbone", "alignment_backbone", "alignment_head")}
    with pytest.raises(config.OutOfScopeError, match="out of scope"):
        config.build_model(cfg, over)
    _check_built(config.build_model(cfg, over, families=("deeplabv2",)))


def _manifest():
    with open(os.path.join(GOLDEN, "deeplabv2_manifest.json")) as f:
        return json.load(f)


def _models():
    from refign_amd import resnet
    return {"resnet101_v1c": lambda: resnet.ResNet("resnet101_v1c", **CFG), "resnet18_v1c": lambda: resnet.ResNet("resnet18_v1c"),
            "deeplabv2_head": lambda: resnet.DeepLabV2Head(2048, 3, 19)}


@pytest.mark.parametrize("which", ["resnet101_v1c", "resnet18_v1c", "deeplabv2_head"])
def test_state_dict_keys_and_shapes_equal_the_reference(which):
    want = _manifest()[which]
    sd = _models()[which]().state_dict()
    assert list(sd) == list(want)                                              # same keys in the same order
    assert {k: list(v.shape) for k, v in sd.items()} == want


def test_reference_layout_state_dict_round_trips_strict(tmp_path):
    from refign_amd import resnet
    want = _manifest()["resnet18_v1c"]
    sd = {k: torch.full(shape, float(i % 7) + 0.5) if "num_batches" not in k else torch.tensor(3)
          for i, (k, shape) in enumerate(want.items())}
    m = resnet.ResNet("resnet18_v1c")
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd) and list(back) == list(sd)
    # an ImageNet file: a `state_dict` entry with the classifier's fc.* keys, which are dropped
    path = str(tmp_path / "resnet18_v1c.pth")
    torch.save({"state_dict": dict(sd, **{"fc.weight": torch.zeros(1000, 512), "fc.bias": torch.zeros(1000)})}, path)
    m2 = resnet.ResNet("resnet18_v1c", pretrained=path)
    assert all(torch.equal(m2.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(FileNotFoundError):
        resnet.ResNet("resnet18_v1c", pretrained=str(tmp_path / "missing.pth"))


def test_init_follows_the_reference():
    from refign_amd import resnet
    torch.manual_seed(0)
    m = resnet.ResNet("resnet50_v1c")
    for mod in m.modules():
        if isinstance(mod, resnet.Bottleneck):
            assert float(mod.bn3.weight.abs().max()) == 0.0 and float(mod.bn1.weight.min()) == 1.0
    w = m.layer3[0].conv2.weight                                              # Kaiming normal, fan_out = 256 * 9
    assert abs(float(w.std()) / (2.0 / (256 * 9)) ** 0.5 - 1) < 0.02
    m = resnet.ResNet("resnet18_v1c", zero_init_residual=False)
    assert float(m.layer1[0].bn2.weight.min()) == 1.0
    h = resnet.DeepLabV2Head(256, 3, 19)
    assert all(float(c.bias.abs().max()) == 0.0 and abs(float(c.weight.std()) / 0.01 - 1) < 0.05 for c in h.conv2d_list)
    assert [c.dilation for c in h.conv2d_list] == [(6, 6), (12, 12), (18, 18), (24, 24)]
    from refign_amd.config import OutOfScopeError
    with pytest.raises(OutOfScopeError):
        resnet.ResNet("resnet18_v1c", with_cp=True)


def _x():
    return torch.from_numpy((hashed_uniform((2, 3, 64, 96), "g14/x") * 4 - 2).astype(np.float32))


def _check_stages(outs, g, prefix, rtol):
    for i, o in enumerate(outs):
        a = o.detach().float().cpu().numpy()
        assert list(a.shape) == list(g[f"{prefix}_c{i + 1}_shape"])
        ref = g[f"{prefix}_c{i + 1}_sample"]
        assert np.abs(a[SAMPLE] - ref).max() <= rtol * np.abs(ref).max(), (prefix, i)
        np.testing.assert_allclose(np.abs(a.astype(np.float64)).sum(), float(g[f"{prefix}_c{i + 1}_abs_sum"]), rtol=rtol)


@pytest.mark.parametrize("model_type", ["resnet18_v1c", "resnet50_v1c", "resnet101_v1c"])
def test_fp32_eval_forward_matches_reference(model_type):
    """rtol 1e-5 (the issue allows 1e-4, the MiT CPU tests' bar): the same ATen ops in the same order as the reference measured
    0 here, the margin is for another BLAS."""
    from refign_amd import resnet
    g = golden("resnet_v1c_64x96")
    m = closed_form_fill(resnet.ResNet(model_type, **({} if model_type == "resnet18_v1c" else CFG)), "backbone.").eval()
    with torch.no_grad():
        outs = m(_x())
    assert isinstance(outs, tuple) and len(outs) == 4
    _check_stages(outs, g, model_type + "_eval", 1e-5)
    with torch.no_grad():                                                      # out_indices picks the stages
        m.out_indices = (1, 3)
        two = m(_x())
    assert len(two) == 2 and torch.equal(two[0], outs[1]) and torch.equal(two[1], outs[3])


def _running(m, leaf):
    return torch.cat([b.flatten() for k, b in m.state_dict().items() if k.endswith(leaf)]).double().cpu().numpy()


def test_train_mode_forward_and_running_statistics_match_reference():
    from refign_amd import resnet
    g = golden("resnet_v1c_64x96")
    m = closed_form_fill(resnet.ResNet("resnet101_v1c", **CFG), "backbone.").train()
    with torch.no_grad():
        outs = m(_x())
    _check_stages(outs, g, "resnet101_v1c_train", 1e-4)
    for leaf in ("running_mean", "running_var"):
        v = _running(m, leaf)
        ref = g[f"resnet101_v1c_train_{leaf}_sample"]
        assert np.abs(v[::16] - ref).max() <= 1e-4 * np.abs(ref).max()
        np.testing.assert_allclose(np.abs(v).sum(), float(g[f"resnet101_v1c_train_{leaf}_abs_sum"]), rtol=1e-5)
    assert int(m.layer3[22].bn3.num_batches_tracked) == 1


def test_head_forward_and_gradients_on_the_cpu_path_match_reference():
    from refign_amd import resnet
    g = golden("deeplabv2_head")
    for i in range(3):
        b, c, h, w = [int(v) for v in g[f"s{i}_shape"]]
        head = closed_form_fill(resnet.DeepLabV2Head(c, 0, 19), "head.")
        x = torch.from_numpy((hashed_uniform((b, c, h, w), f"g14/head{i}/x") - 0.5).astype(np.float32)).requires_grad_()
        gy = torch.from_numpy((hashed_uniform((b, 19, h, w), f"g14/head{i}/g") - 0.5).astype(np.float32))
        y = head([x])
        (y * gy).sum().backward()
        cs = int(g[f"s{i}_gx_cstride"])
        got = {"out": y.detach().numpy(), "gx": x.grad.numpy()[:, ::cs]}
        for r, conv in enumerate(head.conv2d_list):
            got[f"gw{r}"], got[f"gb{r}"] = conv.weight.grad.numpy()[:, ::2], conv.bias.grad.numpy()
        for k, a in got.items():
            ref = g[f"s{i}_{k}"]
            assert a.shape == ref.shape and np.abs(a - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-30), (i, k)
    # in_index / input_transform as BaseHead: an index into the stage tuple
    head = resnet.DeepLabV2Head(8, 3, 5)
    f = [None, None, None, torch.randn(1, 8, 5, 5)]
    assert head(f).shape == (1, 5, 5, 5)


@pytest.mark.parametrize("H,W,n", [(7, 9, 12), (25, 13, 24), (33, 41, 36), (5, 5, 4), (49, 50, 36)])
def test_live_tap_table(H, W, n):
    from refign_amd import resnet
    taps = resnet.live_taps(H, W, (6, 12, 18, 24))
    assert len(taps) == n
    assert taps == sorted(taps) and all(abs(dy) < H and abs(dx) < W and (dy, dx) == ((ky - 1) * d, (kx - 1) * d)
                                        for (r, ky, kx, dy, dx) in taps for d in [(6, 12, 18, 24)[r]])
    # every branch keeps its centre tap; the boxes name the same taps
    assert {r for r, ky, kx, _, _ in taps if (ky, kx) == (1, 1)} == {0, 1, 2, 3}
    boxes = resnet._live_boxes(H, W, (6, 12, 18, 24))
    assert [(r, ky, kx) for r, (y0, y1, x0, x1) in enumerate(boxes) for ky in range(y0, y1) for kx in range(x0, x1)] == \
        [t[:3] for t in taps]


def test_tap_sum_identity_in_fp64():
    """sum_r conv_r(x) == the shifted sum over the live taps of x @ Wt^T, on the CPU in fp64 (what the fused path computes)."""
    from refign_amd import resnet
    torch.manual_seed(1)
    for C, H, W in ((16, 7, 9), (8, 5, 5), (8, 33, 41)):
        x = torch.randn(2, C, H, W, dtype=torch.float64)
        ws = [torch.randn(5, C, 3, 3, dtype=torch.float64) for _ in range(4)]
        want = sum(torch.nn.functional.conv2d(x, w, None, 1, d, d) for w, d in zip(ws, (6, 12, 18, 24)))
        got = torch.zeros_like(want)
        for r, ky, kx, dy, dx in resnet.live_taps(H, W, (6, 12, 18, 24)):
            z = torch.einsum("bchw,kc->bkhw", x, ws[r][:, :, ky, kx])
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
            got[:, :, ys, xs] += z[:, :, ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_frozen_stages_and_norm_eval_after_train():
    from refign_amd import resnet
    m = resnet.ResNet("resnet18_v1c", frozen_stages=2)
    m.train()
    assert not m.stem.training and not m.layer1.training and not m.layer2.training and m.layer3.training and m.layer4.training
    assert not any(p.requires_grad for mod in (m.stem, m.layer1, m.layer2) for p in mod.parameters())
    assert all(p.requires_grad for mod in (m.layer3, m.layer4) for p in mod.parameters())
    assert not m.layer2[1].bn2.training and m.layer3[0].bn1.training
    m = resnet.ResNet("resnet18_v1c", norm_eval=True)
    m.train()
    assert m.training and m.layer1[0].conv1.training
    assert not any(mod.training for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d))
    m = resnet.ResNet("resnet18_v1c")
    m.train()
    assert all(mod.training for mod in m.modules())
    m.eval()
    assert not any(mod.training for mod in m.modules())


def test_geometry_follows_the_reference_rules():
    from refign_amd import resnet
    m = resnet.ResNet("resnet50_v1c", strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4), contract_dilation=True)
    # stride on the 3x3 (style 'pytorch'), padding == dilation, the first block of a dilated stage at half the dilation
    b = m.layer2[0]
    assert b.conv1.stride == (1, 1) and b.conv2.stride == (2, 2) and b.downsample[0].stride == (2, 2) and b.downsample[0].kernel_size == (1, 1)
    assert m.layer3[0].conv2.dilation == (1, 1) and m.layer3[1].conv2.dilation == (2, 2) == m.layer3[1].conv2.padding
    assert m.layer4[0].conv2.dilation == (2, 2) and m.layer4[2].conv2.dilation == (4, 4) == m.layer4[2].conv2.padding
    assert m.layer3[0].downsample is not None and m.layer3[1].downsample is None
    c = resnet.ResNet("resnet50_v1c", style='caffe').layer2[0]
    assert c.conv1.stride == (2, 2) and c.conv2.stride == (1, 1)
    assert resnet.ResNet("resnet18_v1c", max_pool_ceil_mode=True).maxpool.ceil_mode


def _expected_stack(ws, boxes, n_pad, rows, dtype):
    C = ws[0].shape[1]
    want, t = torch.zeros(rows, C, dtype=dtype), 0
    for w, (y0, y1, x0, x1) in zip(ws, boxes):
        for ky in range(y0, y1):
            for kx in range(x0, x1):
                want[t * n_pad:t * n_pad + w.shape[0]] = w[:, :, ky, kx].detach().to(dtype)
                t += 1
    return want


def test_tap_stack_and_bias_stack_share_one_buffer_and_follow_their_parameters():
    """params.tap_stack / bias_stack on CPU tensors: the layout, one buffer for the four weights' entries, re-filled in place by
    refresh(); an in-place change of ONE weight (a version bump) re-fills that weight's slot in the same buffer; a second map
    size gets a buffer of its own and leaves the first alone."""
    from refign_amd import params, resnet
    torch.manual_seed(3)
    K, C, dt = 5, 16, torch.bfloat16
    ws = [torch.nn.Parameter(torch.randn(K, C, 3, 3)) for _ in range(4)]
    bs = [torch.nn.Parameter(torch.randn(K)) for _ in range(4)]
    plan = resnet._Plan(7, 9, (6, 12, 18, 24), K)                       # 12 live taps: branch 0 whole, the others' centres
    assert (plan.T, plan.Np, plan.Nz) == (12, 8, 128)
    Wt = params.tap_stack(ws, dt, plan.boxes, plan.Np, plan.Nz)
    assert Wt.shape == (128, C) and torch.equal(Wt, _expected_stack(ws, plan.boxes, plan.Np, plan.Nz, dt))
    assert float(Wt[12 * 8:].abs().max()) == 0.0 and float(Wt[:8][K:].abs().max()) == 0.0      # padding rows stay zero
    WtT = params.tap_stack(ws, dt, plan.boxes, plan.Np, plan.Nz, transpose=True)
    assert WtT.shape == (C, 128) and torch.equal(WtT, Wt.t())
    bias = params.bias_stack(bs, plan.Np)
    assert bias.shape == (4, 8) and bias.dtype == torch.float32
    assert torch.equal(bias[:, :K], torch.stack([b.detach() for b in bs])) and float(bias[:, K:].abs().max()) == 0.0
    # a second call hands out the same buffers: one entry per weight, all pointing at one tensor
    assert params.tap_stack(ws, dt, plan.boxes, plan.Np, plan.Nz) is Wt and params.bias_stack(bs, plan.Np) is bias
    # an optimizer / EMA update through .data (no version bump), then refresh: re-filled in place
    with torch.no_grad():
        for p in ws + bs:
            p.data.mul_(1.5).add_(0.25)
    assert not torch.equal(Wt, _expected_stack(ws, plan.boxes, plan.Np, plan.Nz, dt))
    params.refresh(ws + bs)
    assert torch.equal(Wt, _expected_stack(ws, plan.boxes, plan.Np, plan.Nz, dt)) and torch.equal(WtT, Wt.t())
    assert torch.equal(bias[:, :K], torch.stack([b.detach() for b in bs]))
    assert params.tap_stack(ws, dt, plan.boxes, plan.Np, plan.Nz) is Wt
    # a version bump on ONE weight only (an in-place op outside refresh): its slot is re-made in the same buffer
    with torch.no_grad():
        ws[2].mul_(-2.0)
    got = params.tap_stack(ws, dt, plan.boxes, plan.Np, plan.Nz)
    assert got is Wt and torch.equal(Wt, _expected_stack(ws, plan.boxes, plan.Np, plan.Nz, dt))
    # ... and on the FIRST weight, which owns the allocation: a new buffer, and every entry follows it
    with torch.no_grad():
        ws[0].add_(1.0)
    new = params.tap_stack(ws, dt, plan.boxes, plan.Np, plan.Nz)
    assert new is not Wt and torch.equal(new, _expected_stack(ws, plan.boxes, plan.Np, plan.Nz, dt))
    with torch.no_grad():
        for p in ws:
            p.data.sub_(0.5)
    params.refresh(ws)
    assert torch.equal(new, _expected_stack(ws, plan.boxes, plan.Np, plan.Nz, dt))
    # another map size: all 36 taps, a buffer of its own under its own key
    big = resnet._Plan(33, 41, (6, 12, 18, 24), K)
    assert (big.T, big.Nz) == (36, 320)
    Wb = params.tap_stack(ws, dt, big.boxes, big.Np, big.Nz)
    assert Wb.shape == (320, C) and torch.equal(Wb, _expected_stack(ws, big.boxes, big.Np, big.Nz, dt))
    assert params.tap_stack(ws, dt, plan.boxes, plan.Np, plan.Nz) is new
    with torch.no_grad():
        for p in ws:
            p.data.mul_(0.5)
    params.refresh(ws)
    assert torch.equal(Wb, _expected_stack(ws, big.boxes, big.Np, big.Nz, dt))
    assert torch.equal(new, _expected_stack(ws, plan.boxes, plan.Np, plan.Nz, dt))

"""GPU: the DeepLabV2 family on the device -- ResNet-v1c under bf16 autocast on the hand-written kernels against the fixtures of
tests/golden/make_golden_deeplabv2.py, one UDA training step against the reference's, and the checkpoint of that step.

Tolerance of the bf16 passes: the same modules are run through the torch library path on the device (mfma.ENABLED = False: library
convolutions, torch BatchNorm, bf16 autocast) against the same fixture, and the kernel path is allowed twice that error, per
stage and per measure.  The two measures of a stage: max |a - ref| over the fixture's strided sample, relative to the sample's
largest magnitude, and the relative error of the abs-sum; each is held to twice the library path's figure of the same measure.
tools/deeplabv2_parity.py writes the figures into profiles/deeplabv2_parity.txt."""
import os
import random

import numpy as np
import pytest
import torch
from conftest import GOLDEN, golden
from fill import closed_form_fill, hashed_uniform

pytestmark = pytest.mark.gpu

CFG = {"strides": (1, 2, 1, 1), "dilations": (1, 1, 2, 4)}
SAMPLE = (slice(None), slice(None, None, 8), slice(None, None, 2), slice(None, None, 2))
OPT = {"class_path": "torch.optim.AdamW", "init_args": {"lr": 6e-5, "weight_decay": 0.01}}
SCH = {"class_path": "helpers.lr_scheduler.LinearWarmupPolynomialLR",
       "init_args": {"warmup_iters": 1500, "warmup_ratio": 1e-6, "power": 1.0, "max_steps": 40000}}


def _backbone(model_type, dev):
    from refign_amd import resnet
    return closed_form_fill(resnet.ResNet(model_type, **({} if model_type == "resnet18_v1c" else CFG)), "backbone.").to(dev)


def _x(dev):
    return torch.from_numpy((hashed_uniform((2, 3, 64, 96), "g14/x") * 4 - 2).astype(np.float32)).to(dev)


def _stage_errors(outs, g, prefix):
    """[(sample error, abs-sum error)] per stage, both relative"""
    errs = []
    for i, o in enumerate(outs):
        a = o.detach().float().cpu().numpy()
        assert list(a.shape) == list(g[f"{prefix}_c{i + 1}_shape"])
        ref = g[f"{prefix}_c{i + 1}_sample"]
        s = float(g[f"{prefix}_c{i + 1}_abs_sum"])
        errs.append((float(np.abs(a[SAMPLE] - ref).max() / np.abs(ref).max()), abs(float(np.abs(a.astype(np.float64)).sum()) / s - 1)))
    return errs


def _running(m, leaf):
    return torch.cat([b.flatten() for k, b in m.state_dict().items() if k.endswith(leaf)]).double().cpu().numpy()


class library_path:
    """the torch library path on the device: no hand-written GEMM / convolution / BatchNorm kernel"""

    def __enter__(self):
        from refign_amd import mfma
        self.saved = (mfma.ENABLED, os.environ.get("RFN_BN_KERNEL"))
        mfma.ENABLED = False
        os.environ["RFN_BN_KERNEL"] = "0"

    def __exit__(self, *exc):
        from refign_amd import mfma
        mfma.ENABLED = self.saved[0]
        if self.saved[1] is None:
            os.environ.pop("RFN_BN_KERNEL", None)
        else:
            os.environ["RFN_BN_KERNEL"] = self.saved[1]
        return False


def eval_errors(model_type, dev, kernels):
    """stage errors of the eval-mode forward under bf16 autocast, and the library-call table of the pass"""
    from refign_amd import mfma
    g = golden("resnet_v1c_64x96")
    m = _backbone(model_type, dev).eval()
    mfma.LIBRARY_CALLS.clear()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        if kernels:
            outs = m(_x(dev))
        else:
            with library_path():
                outs = m(_x(dev))
    torch.cuda.synchronize()
    calls = dict(mfma.LIBRARY_CALLS)
    mfma.LIBRARY_CALLS.clear()
    return _stage_errors(outs, g, model_type + "_eval"), calls


def train_errors(dev, kernels):
    """ResNet-101 in train mode under bf16 autocast (gradient-free, as the EMA teacher runs it): stage errors, the relative errors
    of the running statistics after the pass, the library-call table"""
    from refign_amd import mfma
    g = golden("resnet_v1c_64x96")
    m = _backbone("resnet101_v1c", dev).train()
    mfma.LIBRARY_CALLS.clear()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        if kernels:
            outs = m(_x(dev))
        else:
            with library_path():
                outs = m(_x(dev))
    torch.cuda.synchronize()
    calls = dict(mfma.LIBRARY_CALLS)
    mfma.LIBRARY_CALLS.clear()
    stats = {}
    for leaf in ("running_mean", "running_var"):
        v = _running(m, leaf)
        ref = g[f"resnet101_v1c_train_{leaf}_sample"]
        stats[leaf] = (float(np.abs(v[::16] - ref).max() / np.abs(ref).max()),
                       abs(float(np.abs(v).sum()) / float(g[f"resnet101_v1c_train_{leaf}_abs_sum"]) - 1))
    return _stage_errors(outs, g, "resnet101_v1c_train"), stats, calls


def _hold(kernel, library, what):
    for i, ((ks, ka), (ls, la)) in enumerate(zip(kernel, library)):
        print(f"{what} [{i}]: kernels sample {ks:.3e} abs-sum {ka:.3e} | library sample {ls:.3e} abs-sum {la:.3e}")
    for i, ((ks, ka), (ls, la)) in enumerate(zip(kernel, library)):
        assert ks <= 2 * ls, f"{what} [{i}]: sample error {ks:.3e} on the kernels > 2 x {ls:.3e} on the library path"
        assert ka <= 2 * la, f"{what} [{i}]: abs-sum error {ka:.3e} on the kernels > 2 x {la:.3e} on the library path"


@pytest.mark.parametrize("model_type", ["resnet18_v1c", "resnet50_v1c", "resnet101_v1c"])
def test_eval_forward_bf16_on_the_kernels_within_twice_the_library_error(dev, model_type):
    kern, calls = eval_errors(model_type, dev, kernels=True)
    lib, lib_calls = eval_errors(model_type, dev, kernels=False)
    assert any(k[0].startswith("conv2d") for k in lib_calls)                 # the comparison run did take the library path
    assert not calls, calls                                                  # folded convolutions only: nothing fell back
    _hold(kern, lib, model_type + " eval")


def test_train_mode_bf16_pass_no_fallback_and_running_statistics(dev):
    kern, kstats, calls = train_errors(dev, kernels=True)
    lib, lstats, lib_calls = train_errors(dev, kernels=False)
    assert {k[0] for k in lib_calls} >= {"conv2d", "batch_norm"}
    assert not calls, calls                                                  # no dense-conv and no BatchNorm fallback
    _hold(kern, lib, "resnet101_v1c train")
    _hold([kstats["running_mean"], kstats["running_var"]], [lstats["running_mean"], lstats["running_var"]], "running statistics")


def test_autograd_pass_on_the_kernels_records_no_fallback(dev):
    """the student's pass: forward + backward of ResNet-101 and the fused head under bf16 autocast"""
    from refign_amd import mfma, resnet
    m = _backbone("resnet101_v1c", dev).train()
    head = closed_form_fill(resnet.DeepLabV2Head(2048, 3, 19), "head.").to(dev).train()
    mfma.LIBRARY_CALLS.clear()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = head(m(_x(dev)))
    assert y.shape == (2, 19, 8, 12)
    y.float().square().mean().backward()
    torch.cuda.synchronize()
    assert not mfma.LIBRARY_CALLS, mfma.library_summary()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in list(m.parameters()) + list(head.parameters()))


def make_batch(b, H, W, blk, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    img = lambda k: (hashed_uniform((b, 3, H, W), k) * 4 - 2).astype(np.float32)  # noqa: E731
    trg = img("g13/trg")
    ref = (0.8 * np.roll(trg, (2, -3), (2, 3)) + 0.2 * img("g13/ref")).astype(np.float32)
    lbl = (hashed_uniform((b, H // blk, W // blk), "g13/lbl") * 19).astype(np.int64)
    lbl = np.repeat(np.repeat(lbl, blk, axis=1), blk, axis=2)
    lbl[hashed_uniform((b, H, W), "g13/ign") < 0.05] = 255
    return {"image_src": t(img("g13/src")), "semantic_src": t(lbl), "image_trg": t(trg), "image_ref": t(ref)}


def build_model(dev):
    from refign_amd.align import VGG, UAWarpCHead
    from refign_amd.resnet import DeepLabV2Head, ResNet
    from refign_amd.seg import PixelWeightedCrossEntropyLoss
    from refign_amd.uda import DomainAdaptationSegmentationModel
    model = DomainAdaptationSegmentationModel(
        OPT, SCH, backbone=ResNet("resnet101_v1c", **CFG), head=DeepLabV2Head(2048, 3, 19), loss=PixelWeightedCrossEntropyLoss(),
        alignment_backbone=VGG('vgg16', out_indices=[2, 3, 4]),
        alignment_head=UAWarpCHead(in_index=[0, 1], input_transform='multiple_select', estimate_uncertainty=True),
        backbone_lr_factor=0.1, use_refign=True, adapt_to_ref=False, gamma=0.25, enable_fdist=True, color_jitter_p=1.0, blur=False)
    closed_form_fill(model)
    return model.to(dev).train()


def run_step(dev, autocast=False):
    """one Trainer.step of the golden batch -> (losses, per-group gradient norms, model, trainer)"""
    from refign_amd.trainer import Trainer
    g = golden("step_deeplabv2_96x128")
    H, W = [int(v) for v in g["size"]]
    model = build_model(dev)
    trainer = Trainer(model, fused_optimizer=False)
    trainer.scheduler = torch.optim.lr_scheduler.LambdaLR(trainer.optimizer, lambda s: 1.0)   # as in the golden run
    model._scheduler = trainer.scheduler
    batch = make_batch(2, H, W, 32, dev)
    random.seed(77); np.random.seed(77); torch.manual_seed(77)
    model.global_step = 3
    norms = {}
    real_step = trainer.optimizer.step

    def recording_step(*a, **k):
        norms["v"] = [float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in grp["params"])))
                      for grp in trainer.optimizer.param_groups]
        return real_step(*a, **k)

    trainer.optimizer.step = recording_step
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        trainer.step(batch)
    torch.cuda.synchronize()
    losses = np.array([float(model.logged[k]) for k in ("train_loss_src", "train_loss_featdist_src", "train_loss_uda_trg")])
    return losses, np.array(norms["v"]), model, trainer


def test_training_step_matches_reference_and_its_checkpoint_loads(dev, tmp_path):
    """The reference's step (G14S) in the fp32 parity mode, as test_step_gpu.test_training_step_matches_reference runs the
    DAFormer one: losses rtol 2e-3, gradient norms rtol 2e-2, EMA / student checksums; then the BatchNorm statistics of student
    and teacher (the teacher's layers run in training mode under no_grad, as in the reference), and the checkpoint."""
    import json
    g = golden("step_deeplabv2_96x128")
    losses, norms, model, trainer = run_step(dev)
    try:
        print("losses", losses, g["losses"], "norms", norms, g["grad_norms"])
        np.testing.assert_allclose(losses, g["losses"], rtol=2e-3)
        np.testing.assert_allclose(norms, g["grad_norms"], rtol=2e-2)
        ema = float(sum(p.double().abs().sum() for p in model.ema_parameters()))
        live = float(sum(p.double().abs().sum() for p in model.live_parameters()))
        assert abs(ema - float(g["ema_abs_sum"])) < 1e-5 * float(g["ema_abs_sum"])
        assert abs(live - float(g["live_abs_sum"])) < 1e-5 * float(g["live_abs_sum"])
        assert model.global_step == 4
        for name, mod in (("backbone", model.backbone), ("m_backbone", model.m_backbone)):
            for leaf in ("running_mean", "running_var"):
                v = _running(mod, leaf)
                ref = g[f"{name}_{leaf}_sample"]
                assert np.abs(v[::16] - ref).max() <= 2e-3 * np.abs(ref).max(), (name, leaf)
                np.testing.assert_allclose(np.abs(v).sum(), float(g[f"{name}_{leaf}_abs_sum"]), rtol=2e-3)
        path = str(tmp_path / "last.ckpt")
        trainer.save_checkpoint(path)
        sd = torch.load(path, map_location="cpu", weights_only=False)["state_dict"]
        # reference-keyed: every network of the model under the reference's names
        with open(os.path.join(GOLDEN, "deeplabv2_manifest.json")) as f:
            man = json.load(f)
        for prefix, which in (("backbone.", "resnet101_v1c"), ("m_backbone.", "resnet101_v1c"), ("imnet_backbone.", "resnet101_v1c"),
                              ("head.", "deeplabv2_head"), ("m_head.", "deeplabv2_head")):
            got = {k[len(prefix):]: list(v.shape) for k, v in sd.items() if k.startswith(prefix)}
            assert got == man[which], prefix
        fresh = build_model(torch.device("cpu"))
        fresh.load_state_dict(sd, strict=True)
        for (k, a), b in zip(fresh.state_dict().items(), model.state_dict().values()):
            assert torch.equal(a, b.cpu()), k
        from refign_amd.resnet import ResNet
        bb = ResNet("resnet101_v1c", **CFG)
        bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=True)
    finally:
        trainer.close()


def test_fit_and_validate_from_dataset_folders_through_the_command_line(dev, tmp_path):
    """`python -m refign_amd.run fit --config refign_deeplabv2.yaml --data_dir D` on a tiny tree of PNG files
    (tests/golden/datamodule_tree.py): the model section of configs/cityscapes_acdc/refign_deeplabv2.yaml (ResNet-18 and a
    512-channel head for the test's time: the BasicBlock path) with the tree's data section; five bf16 steps, then `validate` from the checkpoint.  The run goes through the
    opt-in, the student passes -- BatchNorm statistics inside the backbone -- are captured and replayed (no validation inside fit:
    train() after it drops the graphs), and nothing falls back to a library."""
    import copy
    import json
    import yaml
    from datamodule_tree import build_tree, data_section
    from refign_amd import mfma, run
    from refign_amd.datasets import write_class_stats
    from test_deeplabv2_cpu import MODEL_CFG
    with open(os.path.join(GOLDEN, "datamodule_ref.json")) as f:
        recipe = json.load(f)["recipe"]
    tree = str(tmp_path / "data")
    os.makedirs(tree)
    build_tree(tree, recipe)
    write_class_stats(os.path.join(tree, "Cityscapes"))
    cfg = copy.deepcopy(MODEL_CFG)
    cfg["model"]["init_args"]["backbone"]["init_args"]["model_type"] = "resnet18_v1c"
    cfg["model"]["init_args"]["head"]["init_args"]["in_channels"] = 512
    cfg["model"]["init_args"]["adapt_to_ref"] = False
    iou = [{"class_path": "helpers.metrics.IoU", "init_args": {"ignore_index": 255, "num_classes": 19, "compute_on_step": False}}]
    cfg["model"]["init_args"]["metrics"] = {"val": {"ACDC": iou}}
    cfg["seed_everything"] = 0
    cfg["data"] = data_section("ACDC", (128, 128), (128, 256), (136, 240), batch_size=4, num_workers=4)
    cfg["trainer"] = {"max_steps": 5, "sync_batchnorm": True, "precision": "bf16",
                      "callbacks": [{"class_path": "helpers.callbacks.ValEveryNSteps", "init_args": {"every_n_steps": None}},
                                    {"class_path": "pytorch_lightning.callbacks.ModelCheckpoint", "init_args": {"save_last": True}}]}
    path = tmp_path / "refign_deeplabv2_tiny.yaml"
    path.write_text(yaml.safe_dump(cfg, sort_keys=False))
    handles = {}
    mfma.LIBRARY_CALLS.clear()
    hist = run.main(["fit", "--config", str(path), "--data_dir", tree, "--save_dir", str(tmp_path / "ckpt")], handles=handles)
    tr, dm = handles["trainer"], handles["datamodule"]
    try:
        from refign_amd.resnet import DeepLabV2Head, ResNet
        assert isinstance(tr.model.backbone, ResNet) and isinstance(tr.model.head, DeepLabV2Head)
        assert hist == [] and tr.model.global_step == 5
        for name in ("source_pass", "mixed_pass"):
            g = tr.model._graphs[name]
            assert not any(s["failed"] for s in g.states.values()), f"{name}: a capture failed"
            assert g.captured(), f"{name}: the last step did not replay its graph"
        assert not mfma.LIBRARY_CALLS, mfma.library_summary()
        assert torch.load(str(tmp_path / "ckpt" / "last.ckpt"), map_location="cpu", weights_only=False)["global_step"] == 5
    finally:
        dm.close()
        tr.close()
    metrics = run.main(["validate", "--config", str(path), "--data_dir", tree, "--ckpt_path", str(tmp_path / "ckpt" / "last.ckpt")])
    assert set(metrics) == {"val_ACDC_IoU"} and np.isfinite(metrics["val_ACDC_IoU"])
    assert not mfma.LIBRARY_CALLS, mfma.library_summary()                    # the eval-mode student: folded convolutions

"""tests/golden/make_golden_deeplabv2.py -- golden vectors of the DeepLabV2 family (G14), captured from the imported
reference with closed-form weights (fill.closed_form_fill: a pure function of the state_dict keys, so the fixtures hold the
reference's keys / shapes and its outputs only).

  deeplabv2_manifest.json       state_dict keys and shapes of ResNet-101-v1c (the configs' strides / dilations), ResNet-18-v1c
                                and DeepLabV2Head(2048, 3, 19)
  resnet_v1c_64x96.npz          eval-mode stage maps of ResNet-18 / 50 / 101-v1c on a hashed 2 x 3 x 64 x 96 image (strided
                                samples + abs-sums), ResNet-101 in train mode, and its running statistics after that pass
  deeplabv2_head.npz            DeepLabV2Head outputs and (channel-strided) input / weight / bias gradients at three map sizes
  step_deeplabv2_96x128.npz     one reference training_step as make_golden_step.g13 runs it, ResNet-101-v1c + DeepLabV2Head

Run from this directory:  python make_golden_deeplabv2.py [G14M G14B G14H G14S]"""
import json
import os
import random
import sys

import numpy as np
import torch

import _ref_import as R
from fill import closed_form_fill, hashed_uniform

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = {"strides": (1, 2, 1, 1), "dilations": (1, 1, 2, 4)}          # configs/*/refign_deeplabv2.yaml
HEAD_SHAPES = ((2, 64, 7, 9), (1, 128, 25, 13), (2, 64, 33, 41))
SAMPLE = (slice(None), slice(None, None, 8), slice(None, None, 2), slice(None, None, 2))
STAT_STRIDE = 16


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrays.items()})
    print(f"  wrote {name}.npz  ({os.path.getsize(path) / 1024:.1f} kB)")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def backbone(model_type):
    rn = R.ref_module("models.backbones.resnet")
    kw = {} if model_type == "resnet18_v1c" else CFG
    return closed_form_fill(rn.ResNet(model_type, **kw), "backbone.")


def stage_summary(prefix, outs):
    out = {}
    for i, o in enumerate(outs):
        a = o.detach().numpy()
        out[f"{prefix}_c{i + 1}_sample"] = a[SAMPLE]
        out[f"{prefix}_c{i + 1}_abs_sum"] = np.float64(np.abs(a.astype(np.float64)).sum())
        out[f"{prefix}_c{i + 1}_shape"] = np.array(a.shape)
    return out


def running_stats(m):
    """every BatchNorm running_mean / running_var of `m` in state_dict order, flattened: strided sample and abs-sum"""
    out = {}
    for leaf in ("running_mean", "running_var"):
        v = torch.cat([b.flatten() for k, b in m.state_dict().items() if k.endswith(leaf)]).numpy()
        out[f"{leaf}_sample"] = v[::STAT_STRIDE]
        out[f"{leaf}_abs_sum"] = np.float64(np.abs(v.astype(np.float64)).sum())
    return out


def g14_manifest():
    rn = R.ref_module("models.backbones.resnet")
    dl = R.ref_module("models.heads.deeplabv2")
    shapes = lambda m: {k: list(v.shape) for k, v in m.state_dict().items()}  # noqa: E731
    man = {"resnet101_v1c": shapes(rn.ResNet("resnet101_v1c", **CFG)), "resnet18_v1c": shapes(rn.ResNet("resnet18_v1c")),
           "deeplabv2_head": shapes(dl.DeepLabV2Head(2048, 3, 19))}
    path = os.path.join(HERE, "deeplabv2_manifest.json")
    with open(path, "w") as f:
        json.dump(man, f, indent=0, sort_keys=False)
    print(f"  wrote deeplabv2_manifest.json  ({os.path.getsize(path) / 1024:.1f} kB)")


def g14_backbone():
    x = t((hashed_uniform((2, 3, 64, 96), "g14/x") * 4 - 2).astype(np.float32))
    arrays = {}
    for mt in ("resnet18_v1c", "resnet50_v1c", "resnet101_v1c"):
        m = backbone(mt)
        m.eval()                                                 # (the reference's train() returns None)
        arrays.update(stage_summary(mt + "_eval", m(x)))
    m = backbone("resnet101_v1c")
    m.train()
    arrays.update(stage_summary("resnet101_v1c_train", m(x)))
    arrays.update({"resnet101_v1c_train_" + k: v for k, v in running_stats(m).items()})
    save("resnet_v1c_64x96", **arrays)


def g14_head():
    dl = R.ref_module("models.heads.deeplabv2")
    arrays = {}
    torch.set_grad_enabled(True)
    for i, (b, c, h, w) in enumerate(HEAD_SHAPES):
        head = closed_form_fill(dl.DeepLabV2Head(c, 0, 19), "head.")
        x = t((hashed_uniform((b, c, h, w), f"g14/head{i}/x") - 0.5).astype(np.float32)).requires_grad_()
        g = t((hashed_uniform((b, 19, h, w), f"g14/head{i}/g") - 0.5).astype(np.float32))
        y = head([x])
        (y * g).sum().backward()
        # (1 MiB per fixture: the larger maps keep every second / fourth channel of the input gradient, the weight gradients every
        # second input channel)
        cs = 1 if x.numel() < 30000 else 2 if x.numel() < 100000 else 4
        arrays.update({f"s{i}_shape": np.array([b, c, h, w]), f"s{i}_out": y.detach().numpy(),
                       f"s{i}_gx": x.grad.numpy()[:, ::cs], f"s{i}_gx_cstride": np.int64(cs)})
        for r, conv in enumerate(head.conv2d_list):
            arrays[f"s{i}_gw{r}"] = conv.weight.grad.numpy()[:, ::2]
            arrays[f"s{i}_gb{r}"] = conv.bias.grad.numpy()
    torch.set_grad_enabled(False)
    save("deeplabv2_head", **arrays)


def g14_step():
    import make_golden_step as S
    sm = R.ref_module("models.segmentation_model")
    rn = R.ref_module("models.backbones.resnet")
    dl = R.ref_module("models.heads.deeplabv2")
    ls = R.ref_module("models.losses")
    vg = R.ref_module("models.backbones.vgg")
    ua = R.ref_module("models.heads.uawarpc")

    class Model(sm.DomainAdaptationSegmentationModel):
        global_step = 0
        logged = {}

        def optimizers(self):
            return self._rec

        def lr_schedulers(self):
            return self._sch

        def manual_backward(self, loss, retain_graph=False):
            loss.backward(retain_graph=retain_graph)

        def log(self, k, v, **kw):
            self.logged[k] = float(v)

        @property
        def device(self):
            return torch.device("cpu")

    torch.set_grad_enabled(True)
    model = Model(S.OPT, S.SCH, backbone=rn.ResNet("resnet101_v1c", **CFG), head=dl.DeepLabV2Head(2048, 3, 19),
                  loss=ls.PixelWeightedCrossEntropyLoss(), alignment_backbone=vg.VGG('vgg16', out_indices=[2, 3, 4]),
                  alignment_head=ua.UAWarpCHead(in_index=[0, 1], input_transform='multiple_select', estimate_uncertainty=True),
                  backbone_lr_factor=0.1, use_refign=True, adapt_to_ref=False, gamma=0.25, enable_fdist=True,
                  color_jitter_p=1.0, blur=False)
    closed_form_fill(model)
    model.train()
    opt = torch.optim.AdamW(model.optimizer_parameters(), lr=6e-5, weight_decay=0.01)
    model._rec = S.Recorder(opt)
    model._sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
    H, W = 96, 128
    batch = S.make_batch(2, H, W, 32)
    random.seed(77); np.random.seed(77); torch.manual_seed(77)
    model.global_step = 3
    model.training_step(batch, 0)
    ema = float(sum(p.double().abs().sum() for p in model.ema_parameters()))
    live = float(sum(p.double().abs().sum() for p in model.live_parameters()))
    stats = {"backbone_" + k: v for k, v in running_stats(model.backbone).items()}
    stats.update({"m_backbone_" + k: v for k, v in running_stats(model.m_backbone).items()})
    save("step_deeplabv2_96x128", losses=np.array([model.logged["train_loss_src"], model.logged["train_loss_featdist_src"],
                                                   model.logged["train_loss_uda_trg"]]),
         grad_norms=np.array(model._rec.norms), groups=np.array([len(g["params"]) for g in opt.param_groups]),
         ema_abs_sum=ema, live_abs_sum=live, size=np.array([H, W]), **stats)
    print("   ", model.logged, model._rec.norms)
    torch.set_grad_enabled(False)


GROUPS = {"G14M": g14_manifest, "G14B": g14_backbone, "G14H": g14_head, "G14S": g14_step}

if __name__ == "__main__":
    R.setup()
    torch.set_grad_enabled(False)
    for name in (sys.argv[1:] or list(GROUPS)):
        print(name)
        GROUPS[name]()

"""N3 -- checkpoint interchange (models/segmentation_model.py:421-436, models/heads/uawarpc.py:282-305,
models/backbones/mix_transformer.py:445-479): Lightning-format `.ckpt` files ({'state_dict': ...}) written by the
reference load into refign_amd with strict=True and the other way round, with identical tensors; the sub-module loaders
strip the prefixes the reference strips (`alignment_head.`, `backbone.`, drop `head.*`)."""
import json
import os

import pytest
import torch

DIMS = [32, 64, 160, 256]
OPT = {"class_path": "torch.optim.AdamW", "init_args": {"lr": 6e-5, "weight_decay": 0.01}}
SCH = {"class_path": "helpers.lr_scheduler.LinearWarmupPolynomialLR",
       "init_args": {"warmup_iters": 1500, "warmup_ratio": 1e-6, "power": 1.0, "max_steps": 40000}}


def ours(use_hrda=True, pretrained=None):
    from refign_amd.align import VGG, UAWarpCHead
    from refign_amd.seg import DAFormerHead, MixVisionTransformer, PixelWeightedCrossEntropyLoss, SegFormerHead
    from refign_amd.uda import DomainAdaptationSegmentationModel
    return DomainAdaptationSegmentationModel(
        OPT, SCH, backbone=MixVisionTransformer("mit_b0"), head=DAFormerHead(DIMS, [0, 1, 2, 3], 19, 'multiple_select'),
        loss=PixelWeightedCrossEntropyLoss(), alignment_backbone=VGG('vgg16', out_indices=[2, 3, 4]),
        alignment_head=UAWarpCHead(in_index=[0, 1], input_transform='multiple_select', estimate_uncertainty=True),
        use_refign=True, use_hrda=use_hrda, hrda_scale_attention=SegFormerHead(DIMS, [0, 1, 2, 3], 19, 'multiple_select'),
        pretrained=pretrained)


def test_lightning_checkpoint_round_trip(tmp_path):
    """save -> load(strict) -> identical state, through the `pretrained=` constructor keyword of the reference; the
    UAWarpC head and the MiT backbone pick their sub-trees out of the same file."""
    from fill import closed_form_fill
    from refign_amd.align import UAWarpCHead
    from refign_amd.seg import MixVisionTransformer
    a = closed_form_fill(ours())
    path = str(tmp_path / "model.ckpt")
    torch.save({"state_dict": a.state_dict(), "global_step": 7, "pytorch-lightning_version": "1.5.10"}, path)
    b = ours(pretrained=path)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    head = UAWarpCHead(in_index=[0, 1], input_transform='multiple_select', estimate_uncertainty=True, pretrained=path)
    assert all(torch.equal(v, sa["alignment_head." + k]) for k, v in head.state_dict().items())
    mit = MixVisionTransformer("mit_b0", pretrained=path)
    assert all(torch.equal(v, sa["backbone." + k]) for k, v in mit.state_dict().items())
    # a key that does not belong makes the strict load fail, like the reference
    sd = dict(sa)
    sd["backbone.bogus"] = torch.zeros(1)
    torch.save({"state_dict": sd}, path)
    with pytest.raises(RuntimeError, match="bogus"):
        ours(pretrained=path)


def _reference_state_dict():
    """The state_dict of the REFERENCE's HRDA model with closed-form weights (make_golden_step.run_reference(True)), rebuilt
    from tests/golden/ref_checkpoint_hrda_mit_b0.json (make_golden_refcheck.py): keys in the reference's order, shapes and
    dtypes as it has them, closed_form_fill values for the floating entries and the recorded values for the others."""
    import types
    from fill import closed_form_fill
    with open(os.path.join(os.path.dirname(__file__), "golden", "ref_checkpoint_hrda_mit_b0.json")) as f:
        entries = json.load(f)
    sd = {e["key"]: (torch.tensor(e["value"], dtype=getattr(torch, e["dtype"])) if "value" in e else
                     torch.empty(e["shape"], dtype=getattr(torch, e["dtype"]))) for e in entries}
    closed_form_fill(types.SimpleNamespace(state_dict=lambda: sd))
    return sd


def test_checkpoints_interchange_with_the_reference(tmp_path):
    """A checkpoint written from the REFERENCE's module tree loads here with strict=True, one written here has what the
    reference's loader (segmentation_model.py:421-436: load_state_dict(strict=True)) takes: the same keys, shapes and
    dtypes, tensor for tensor."""
    sr = _reference_state_dict()          # HRDA variant, closed-form weights
    path = str(tmp_path / "ref.ckpt")
    torch.save({"state_dict": sr}, path)
    mine = ours(pretrained=path)
    sm = mine.state_dict()
    assert set(sr) == set(sm), sorted(set(sr) ^ set(sm))[:10]
    assert all(sr[k].shape == sm[k].shape and torch.equal(sr[k], sm[k]) for k in sr)
    # and back: perturb ours, save, and load the file the way the reference's strict loader does
    with torch.no_grad():
        for p in mine.parameters():
            p.mul_(1.5)
    back = str(tmp_path / "ours.ckpt")
    torch.save({"state_dict": mine.state_dict()}, back)
    loaded = torch.load(back)["state_dict"]
    assert list(loaded) == list(mine.state_dict())
    assert set(loaded) == set(sr), sorted(set(loaded) ^ set(sr))[:10]
    assert all(loaded[k].shape == sr[k].shape and loaded[k].dtype == sr[k].dtype for k in sr)
    assert all(torch.equal(loaded[k], v) for k, v in mine.state_dict().items())

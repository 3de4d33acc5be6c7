"""GPU: the fused evaluation tail (csrc/evaltail.hip, refign_amd/evaltail.py) -- from low-resolution crop logits to arg-max
labels and confusion counts in one kernel -- against a float64 restatement written here: per box
F.interpolate(logits.double(), size=box size, bilinear, align_corners=False) on the CPU, summed into a float64 image, divided
by the cover count; arg-max and the gap between the two largest classes (the margin) from that.

A pixel is DECIDED when its margin exceeds 1e-4 * max|logit|.  The threshold is derived, not tuned: the fp32 form of the same
sums differs from float64 by at most 9e-7 on these inputs (measured on the CPU, logits up to 13), so the threshold is more
than a hundred times the rounding error and a correct kernel cannot disagree on a decided pixel.  On decided pixels labels
and counts are compared EXACTLY; at most 1 % of the pixels may be undecided on the synthetic inputs (0.08-0.25 % measured)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from fill import hashed_uniform
from test_step_gpu import build

pytestmark = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def slide_boxes(H, W, crop, stride):
    (hc, wc), (hs, ws) = crop, stride
    boxes = []
    for iy in range(max(H - hc + hs - 1, 0) // hs + 1):
        for ix in range(max(W - wc + ws - 1, 0) // ws + 1):
            y2, x2 = min(iy * hs + hc, H), min(ix * ws + wc, W)
            boxes.append((max(y2 - hc, 0), y2, max(x2 - wc, 0), x2))
    return boxes


def restate(logits, boxes, H, W):
    """float64 on the CPU -> (arg-max (B, H, W) int64, decided (B, H, W) bool); logits (nbox * B, C, h, w) in any dtype."""
    lg = logits.detach().cpu().double()
    B = lg.shape[0] // len(boxes)
    acc = torch.zeros(B, lg.shape[1], H, W, dtype=torch.float64)
    cnt = torch.zeros(B, 1, H, W, dtype=torch.float64)
    for k, (y1, y2, x1, x2) in enumerate(boxes):
        acc[:, :, y1:y2, x1:x2] += F.interpolate(lg[k * B:(k + 1) * B], size=(y2 - y1, x2 - x1), mode="bilinear",
                                                 align_corners=False)
        cnt[:, :, y1:y2, x1:x2] += 1
    assert int((cnt == 0).sum()) == 0
    mean = acc / cnt
    top = mean.topk(2, dim=1).values
    return mean.argmax(1), (top[:, 0] - top[:, 1]) > 1e-4 * float(lg.abs().max())


def count(target, pred, C, ignore_index=255):
    """Brute-force confusion matrix (rows = target) of the pixels with target != ignore_index and inside [0, C)."""
    t, p = target.reshape(-1).cpu(), pred.reshape(-1).cpu()
    keep = (t != ignore_index) & (t >= 0) & (t < C)
    return torch.bincount(t[keep] * C + p[keep], minlength=C * C).view(C, C)


def random_target(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[:, H // 3:H // 3 + max(H // 8, 1)] = 255                       # a band of ignored pixels
    return y


CASES = [
    (2, 19, 120, 200, (64, 64), (40, 48), (16, 16), "f32"),
    (2, 19, 120, 200, (64, 64), (40, 48), (16, 16), "bf16"),
    (2, 19, 120, 200, (64, 64), (40, 48), (16, 16), "f16"),
    (1, 19, 270, 480, (256, 256), (105, 105), (64, 64), "f32"),
    (2, 7, 97, 131, (64, 48), (33, 29), (16, 12), "f32"),            # ragged: the last boxes clamped to the border
    (1, 19, 540, 960, (540, 540), (210, 210), (135, 135), "bf16"),   # the bench geometry at half size
    (1, 19, 48, 80, None, None, (12, 20), "f32"),                     # whole image: one box
    # beyond the table of the issue: the kernel's other code paths
    (1, 27, 97, 131, (64, 48), (33, 29), (16, 12), "f16"),           # more than 19 classes: the 32-class instantiation
    (2, 19, 40, 56, (32, 32), (8, 24), (32, 32), "f32"),             # scale 1: the footprint is read from global memory
    (1, 5, 40, 56, (32, 32), (8, 24), (64, 80), "bf16"),             # logits finer than the image (scale 2 and 2.5)
    (1, 27, 97, 131, (64, 48), (33, 29), (16, 12), "f32"),           # the 32-class instantiation in the other two dtypes
    (1, 27, 97, 131, (64, 48), (33, 29), (16, 12), "bf16"),
]


@pytest.mark.parametrize("B,C,H,W,crop,stride,lo,dtype", CASES)
def test_kernel_matches_the_float64_restatement(dev, B, C, H, W, crop, stride, lo, dtype):
    from refign_amd import evaltail
    boxes = [(0, H, 0, W)] if crop is None else slide_boxes(H, W, crop, stride)
    g = torch.Generator().manual_seed(0)
    logits = (3 * torch.randn(len(boxes) * B, C, *lo, generator=g)).to(DTYPES[dtype])
    want, decided = restate(logits, boxes, H, W)
    undecided = 1 - float(decided.float().mean())
    print(f"\n{B}x{C}x{H}x{W} {dtype}: {len(boxes)} boxes, undecided {100 * undecided:.3f} %")
    assert undecided <= 0.01
    target = random_target(B, C, H, W, 1)
    target[~decided] = 255
    confmat = torch.zeros(C, C, dtype=torch.int64, device=dev)
    labels = evaltail.slide_argmax_confmat(logits.to(dev), boxes, (H, W), target.to(dev), 255, confmat=confmat)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (B, H, W)
    labels = labels.cpu().long()
    assert torch.equal(labels[decided], want[decided])
    assert torch.equal(confmat.cpu(), count(target, want, C))
    assert int(confmat.sum()) == int((target != 255).sum())


def test_targets_ignore_out_of_range_accumulate(dev):
    from refign_amd import evaltail
    B, C, H, W = 2, 19, 120, 200
    boxes = slide_boxes(H, W, (64, 64), (40, 48))
    g = torch.Generator().manual_seed(3)
    logits = (3 * torch.randn(len(boxes) * B, C, 16, 16, generator=g)).to(dev)
    want, decided = restate(logits, boxes, H, W)
    target = random_target(B, C, H, W, 4)
    target[~decided] = 255
    once = count(target, want, C)
    # all pixels ignored: the matrix keeps what it held
    cm = torch.full((C, C), 5, dtype=torch.int64, device=dev)
    evaltail.slide_argmax_confmat(logits, boxes, (H, W), torch.full((B, H, W), 255, device=dev), 255, False, cm)
    assert torch.equal(cm.cpu(), torch.full((C, C), 5))
    # two calls add
    cm.zero_()
    for _ in range(2):
        out = evaltail.slide_argmax_confmat(logits, boxes, (H, W), target.to(dev), 255, want_labels=False, confmat=cm)
        assert out is None                                           # confmat only
    assert torch.equal(cm.cpu(), 2 * once)
    # target values C and -1 are skipped like ignore_index; another ignore_index counts the 255 band out through the range
    odd = target.clone()
    odd[:, :, :7] = C
    odd[:, :, 7:13] = -1
    cm.zero_()
    evaltail.slide_argmax_confmat(logits, boxes, (H, W), odd.to(dev), 255, False, cm)
    assert torch.equal(cm.cpu(), count(odd, want, C)) and int(cm.sum()) < int(once.sum())
    cm.zero_()
    evaltail.slide_argmax_confmat(logits, boxes, (H, W), target.to(dev), 3, False, cm)
    assert torch.equal(cm.cpu(), count(target, want, C, ignore_index=3)) and int(cm[3].sum()) == 0
    # labels only
    labels = evaltail.slide_argmax_confmat(logits, boxes, (H, W)).cpu().long()
    assert torch.equal(labels[decided], want[decided])


def test_argument_checks_return_errors_and_launch_nothing(dev):
    from refign_amd import evaltail
    B, C, H, W = 1, 19, 96, 160
    good = slide_boxes(H, W, (64, 64), (40, 48))
    logits = torch.zeros(1, C, 16, 16, device=dev)
    logits[:, 1] = 1.0                                               # (a launch would write label 1 everywhere)
    target = torch.zeros(B, H, W, dtype=torch.int64, device=dev)
    cm = torch.zeros(C, C, dtype=torch.int64, device=dev)

    def call(boxes, confmat=cm):
        return evaltail.slide_argmax_confmat(logits[:1].expand(len(boxes) * B, C, 16, 16), boxes, (H, W), target, 255,
                                             False, confmat)

    outside = list(good)
    outside[-1] = (40, 104, 96, 160)
    with pytest.raises(RuntimeError, match="not inside"):
        call(outside)
    two_sizes = list(good)
    two_sizes[0] = (0, 64, 0, 48)
    with pytest.raises(RuntimeError, match="box 0 is"):
        call(two_sizes[::-1])
    with pytest.raises(RuntimeError, match="uncovered"):
        call(good[:-1])
    with pytest.raises(RuntimeError, match="uncovered"):
        call([b for b in good if b != good[1]])
    with pytest.raises(RuntimeError, match="C=33"):
        evaltail.slide_argmax_confmat(torch.zeros(len(good), 33, 16, 16, device=dev), good, (H, W), target, 255, False,
                                      torch.zeros(33, 33, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="both NULL"):
        call(good, confmat=None)
    with pytest.raises(RuntimeError, match="boxes"):
        call([good[0]] * 65)
    torch.cuda.synchronize()
    assert int(cm.sum()) == 0, "a rejected call launched the kernel"
    call(good)                                                       # and the same arguments, valid, do count
    assert int(cm[0, 1]) == B * H * W


def _segmentation_batch(dev, seed=5):
    x = torch.from_numpy((hashed_uniform((2, 3, 96, 160), "g15/img") * 4 - 2).astype(np.float32)).to(dev)
    return x, random_target(2, 19, 96, 160, seed).to(dev)


def _sliding(model):
    model.use_slide_inference, model.inference_batched_slide = True, True
    model.inference_crop_size, model.inference_stride = [64, 64], [40, 48]
    return model


def _recorded(model, name):
    """Wrap model.<name>: every call's result is appended to the returned list."""
    rec, real = [], getattr(model, name)

    def wrapped(*a, **k):
        out = real(*a, **k)
        rec.append(out)
        return out
    setattr(model, name, wrapped)
    return rec


def _validate_confmat(tr, batch):
    """Trainer.validate on one batch -> (the IoU metric's confusion matrix just before epoch end, the returned dict)."""
    model, seen = tr.model, {}
    real = model.validation_epoch_end

    def end(outs=None):
        seen["cm"] = model.valid_metrics["val_ACDC_IoU"].confmat.clone().cpu()
        return real(outs)
    model.validation_epoch_end = end
    try:
        out = tr.validate({"ACDC": [batch]})
    finally:
        del model.validation_epoch_end
    return seen["cm"], out


@pytest.mark.parametrize("precision", [32, "bf16"])
@pytest.mark.parametrize("use_hrda", [False, True])
def test_trainer_validate_on_the_fused_path(dev, monkeypatch, use_hrda, precision):
    """Trainer.validate through the fused tail == the restatement applied to what model.crop_logits returned; with
    RFN_EVAL_FUSED=0 the same call goes through validation_step and, without autocast, counts the same matrix.  (Under 16-bit
    autocast validation_step rounds every up-sampled crop to 16 bits before averaging, the fused tail does not: there the two
    are compared through the restatement only.)"""
    from refign_amd.metrics import IoU, MyMetricCollection
    from refign_amd.trainer import Trainer
    monkeypatch.delenv("RFN_EVAL_FUSED", raising=False)
    model = _sliding(build(use_hrda, dev))
    model.valid_metrics = MyMetricCollection({"val_ACDC_IoU": IoU(num_classes=19, ignore_index=255),
                                              "val_DarkZurich_IoU": IoU(num_classes=19, ignore_index=255)}).to(dev)
    tr = Trainer(model, precision=precision)
    x, y0 = _segmentation_batch(dev)
    crops, steps = _recorded(model, "crop_logits"), _recorded(model, "validation_step")
    _validate_confmat(tr, {"image": x, "semantic": y0})
    assert len(crops) == 1 and not steps, "validate did not take the fused path"
    logits, boxes = crops[0]
    assert boxes == slide_boxes(96, 160, (64, 64), (40, 48)) and logits.shape[0] == 2 * len(boxes)
    want, decided = restate(logits, boxes, 96, 160)
    undecided = 1 - float(decided.float().mean())
    print(f"\nhrda={use_hrda} precision={precision}: logits {tuple(logits.shape)} {logits.dtype}, undecided {100 * undecided:.2f} %")
    assert undecided <= 0.5
    y = y0.clone()
    y[~decided.to(dev)] = 255
    cm, out = _validate_confmat(tr, {"image": x.cpu(), "semantic": y.cpu()})       # host batches are moved to the device
    assert len(crops) == 2 and not steps
    want, decided = restate(crops[1][0], boxes, 96, 160)             # the logits of THIS call
    assert bool(decided[y.cpu() != 255].all()), "a counted pixel is undecided in the second forward"
    assert torch.equal(cm, count(y, want, 19)) and int(cm.sum()) == int((y != 255).sum())
    ref = IoU(num_classes=19, ignore_index=255)
    ref.add_confusion(cm)
    assert set(out) == {"val_ACDC_IoU", "val_DarkZurich_IoU"} and out["val_DarkZurich_IoU"] == 0.0
    assert abs(out["val_ACDC_IoU"] - float(ref.compute())) < 1e-6
    assert model.training and not model.alignment_head.training
    monkeypatch.setenv("RFN_EVAL_FUSED", "0")
    cm0, out0 = _validate_confmat(tr, {"image": x, "semantic": y})
    assert len(crops) == 2 and len(steps) == 1, "RFN_EVAL_FUSED=0 did not go through validation_step"
    if precision == 32:
        assert torch.equal(cm0, cm) and out0 == out
    tr.close()


def test_trainer_predict_writes_the_fused_labels(dev, tmp_path, monkeypatch):
    from PIL import Image
    from refign_amd import evaltail
    from refign_amd.trainer import Trainer
    monkeypatch.delenv("RFN_EVAL_FUSED", raising=False)
    model = _sliding(build(False, dev))
    tr = Trainer(model, precision=32)
    x, _ = _segmentation_batch(dev)
    steps = _recorded(model, "predict_step")
    n = tr.predict({"ACDC": [{"image": x, "filename": ["a.png", "sub/b.png"]}]}, str(tmp_path), orig_size=(96, 160))
    assert n == 4 and not steps
    model.eval()
    crops = _recorded(model, "crop_logits")
    labels = evaltail.labels(model, x, out_size=(96, 160))
    want, decided = restate(*crops[0], 96, 160)
    assert torch.equal(labels.cpu().long()[decided], want[decided])
    labels = labels.cpu().numpy()
    for i, name in enumerate(("a.png", "sub/b.png")):
        ids = np.array(Image.open(tmp_path / "preds" / "ACDC" / name))
        assert ids.dtype == np.uint8 and np.array_equal(ids, labels[i])
        col = Image.open(tmp_path / "color_preds" / "ACDC" / name)
        assert col.mode == "P" and np.array_equal(np.array(col), labels[i])
        assert tuple(col.getpalette()[:3]) == (128, 64, 128)          # road
    with pytest.raises(ValueError, match="image size"):
        evaltail.labels(model, x, out_size=(120, 200))
    # another output size is not the fused path's: predict_step writes, into the same layout
    model.train()
    n = tr.predict({"DarkZurich": [{"image": x, "filename": ["c.png", "d.png"]}]}, str(tmp_path), orig_size=(120, 200))
    assert n == 4 and len(steps) == 1
    assert np.array(Image.open(tmp_path / "preds" / "DarkZurich" / "c.png")).shape == (120, 200)
    tr.close()


@pytest.mark.parametrize("use_hrda", [False, True])
def test_fused_step_enqueues_without_host_synchronisation(dev, monkeypatch, use_hrda):
    from refign_amd import evaltail
    from refign_amd.metrics import IoU, MyMetricCollection
    monkeypatch.delenv("RFN_EVAL_FUSED", raising=False)
    model = _sliding(build(use_hrda, dev)).eval()
    metrics = MyMetricCollection({"val_ACDC_IoU": IoU(num_classes=19, ignore_index=255)}).to(dev)
    x, y = _segmentation_batch(dev)
    batch = {"image": x, "semantic": y}
    with torch.no_grad():
        assert evaltail.eval_step(model, metrics, batch, "ACDC")      # first call: caches are filled, the library is loaded
        torch.cuda.synchronize()
        first = metrics["val_ACDC_IoU"].confmat.clone()
        torch.cuda.set_sync_debug_mode("error")
        try:
            assert evaltail.eval_step(model, metrics, batch, "ACDC")
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(metrics["val_ACDC_IoU"].confmat, 2 * first) and int(first.sum()) == int((y != 255).sum())

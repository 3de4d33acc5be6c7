"""The tail of the evaluation forward as one HIP kernel (csrc/evaltail.hip, rfn_slide_argmax_confmat): from the head's
low-resolution crop logits (DomainAdaptationSegmentationModel.crop_logits) straight to arg-max labels and confusion counts.

Semantics, per image pixel: for every crop box that contains it the bilinear sample (align_corners=False, ATen's rule) of
that crop's logits; the mean over those boxes in fp32; the first largest class.  With a target, pixels whose target is
`ignore_index` or outside [0, C) are skipped, the others counted in a (C, C) int64 matrix (rows = target).  That is what
forward() -> arg-max -> IoU.update computes when the label size equals the image size, without the up-sampled logits, the
image-sized sum and count tensors and the host synchronisation of slide_inference's cover assert (the cover is checked on
the host from the box list).

Labels or predictions at ANOTHER size (the `test:` sections that resize the image only, predict_step's orig_dims):
rfn_slide_argmax_confmat_resized does the second interpolation of forward(x, out_size) as well -- per output pixel the bilinear
sample (align_corners=False, scale H / Ho, clamped) of those fp32 means on the image grid, then the first largest class -- so
neither the image-sized nor the label-sized logits exist.  With equal sizes it is bit-equal to the first entry, which is the
one such calls keep launching.

One difference, in both stages: under 16-bit autocast forward() rounds its intermediate tensors to 16 bits (every up-sampled
crop before the averaging, the averaged logits before the second interpolation, its result); the kernel keeps fp32 from the crop
logits to the arg-max.

The matcher (AlignmentModel) has a fused step of its own: after its forward, SparseEPE.update is one kernel per batch
(csrc/sparseepe.hip through refign_amd/sparse_epe.py) instead of a hundred-odd small launches and a host synchronisation per
sample; _matcher_eval_step lists its conditions.

`RFN_EVAL_FUSED=0` keeps Trainer.validate / test / predict on validation_step / test_step / predict_step, for both models."""
import ctypes
import os

import torch

from . import _lib
from ._tensor import DTYPE_CODE, ptr

MAX_CLASSES = 32
_BOXES = {}


def enabled():
    return os.environ.get("RFN_EVAL_FUSED", "1") != "0"


def _c_boxes(boxes):
    key = tuple(int(v) for b in boxes for v in b)
    arr = _BOXES.get(key)
    if arr is None:
        if len(_BOXES) > 256:
            _BOXES.clear()
        arr = _BOXES[key] = (ctypes.c_int * len(key))(*key)
    return arr


def slide_argmax_confmat(crop_logits, boxes, size, target=None, ignore_index=255, want_labels=True, confmat=None, out_size=None):
    """The kernel call.  crop_logits (nbox * B, C, h, w) on the device, crop k of image b at row k * B + b; boxes: nbox x
    (y1, y2, x1, x2); size = (H, W), the image.  `out_size` = (Ho, Wo): the size of target, labels and counts -- None or the
    image's: rfn_slide_argmax_confmat; another: rfn_slide_argmax_confmat_resized, the second interpolation of
    forward(x, out_size) inside the kernel.  -> labels (B, Ho, Wo) uint8 or None; with `confmat` (C, C) int64 the counts
    against `target` (B, Ho, Wo) int64 are ADDED to it.  Nothing here waits for the device."""
    if not crop_logits.is_cuda:
        raise RuntimeError("evaltail: crop_logits must be a HIP (cuda:N) tensor: refign_amd has no CPU path")
    if crop_logits.dtype not in DTYPE_CODE or crop_logits.dim() != 4:
        raise RuntimeError(f"evaltail: crop_logits (N, C, h, w) in fp32 / bf16 / fp16 expected, got "
                           f"{tuple(crop_logits.shape)} {crop_logits.dtype}")
    nbox = len(boxes)
    N, C, h, w = crop_logits.shape
    if nbox == 0 or N % nbox:
        raise RuntimeError(f"evaltail: {N} crop logits for {nbox} boxes")
    B, (H, W) = N // nbox, (int(v) for v in size)
    Ho, Wo = (H, W) if out_size is None else (int(v) for v in out_size)
    lg = crop_logits.contiguous()
    dev = lg.device
    if target is not None:
        if target.dtype != torch.int64 or tuple(target.shape) != (B, Ho, Wo) or target.device != dev:
            raise RuntimeError(f"evaltail: target ({B}, {Ho}, {Wo}) int64 on {dev} expected, got {tuple(target.shape)} "
                               f"{target.dtype} on {target.device}")
        target = target.contiguous()
    if confmat is not None and (confmat.dtype != torch.int64 or tuple(confmat.shape) != (C, C) or confmat.device != dev
                                or not confmat.is_contiguous()):
        raise RuntimeError(f"evaltail: confmat ({C}, {C}) int64 contiguous on {dev} expected")
    labels =torch.empty((B, Ho, Wo), dtype=torch.uint8, device=dev) if want_labels else None
    if (Ho, Wo) == (H, W):
        _lib.call("rfn_slide_argmax_confmat", dev, ptr(lg), DTYPE_CODE[lg.dtype], B, C, h, w, _c_boxes(boxes), nbox, H, W,
                  ptr(target), int(ignore_index), ptr(labels), ptr(confmat))
    else:
        _lib.call("rfn_slide_argmax_confmat_resized", dev, ptr(lg), DTYPE_CODE[lg.dtype], B, C, h, w, _c_boxes(boxes), nbox, H, W,
                  Ho, Wo, ptr(target), int(ignore_index), ptr(labels), ptr(confmat))
    return labels


def _size(x, out_size):
    H, W = x.shape[-2:]
    if out_size is not None and tuple(int(v) for v in out_size) != (H, W):
        raise ValueError(f"evaltail: output size {tuple(out_size)} != image size {(H, W)}: the second interpolation of "
                         f"forward(x, out_size) is not the identity; use labels_resized()")
    return H, W


@torch.no_grad()
def labels(model, x, out_size=None):
    """-> (B, H, W) uint8: arg-max of model.forward(x) without the full-resolution logits.  `out_size`: None or the image size
    (another size: labels_resized)."""
    size = _size(x, out_size)
    logits, boxes = model.crop_logits(x)
    return slide_argmax_confmat(logits, boxes, size)


@torch.no_grad()
def labels_resized(model, x, out_size):
    """-> (B, Ho, Wo) uint8: arg-max of model.forward(x, out_size) without the logits at the image's or at the output size."""
    logits, boxes = model.crop_logits(x)
    return slide_argmax_confmat(logits, boxes, x.shape[-2:], out_size=out_size)


@torch.no_grad()
def confusion(model, x, target, ignore_index=255):
    """-> (C, C) int64 on the device: counts of (target, arg-max of model.forward(x, target.shape[-2:])); a target of any size."""
    logits, boxes = model.crop_logits(x)
    out = torch.zeros((logits.shape[1],) * 2, dtype=torch.int64, device=logits.device)
    slide_argmax_confmat(logits, boxes, x.shape[-2:], target, ignore_index, want_labels=False, confmat=out,
                         out_size=target.shape[-2:])
    return out


def _model_ok(model, x):
    return enabled() and hasattr(model, "crop_logits") and torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and \
        getattr(getattr(model, "head", None), "num_classes", MAX_CLASSES + 1) <= MAX_CLASSES


def _matcher_eval_step(model, metrics, batch, src_name):
    """eval_step for an AlignmentModel: its forward as alignment_model._eval_step runs it, then SparseEPE.update as ONE kernel
    (refign_amd/sparse_epe.py) whose rows every selected metric adds.  -> False when a condition does not hold: RFN_EVAL_FUSED=0;
    images or points not on the device; the points not `batch size` (n, 2) fp32 tensors with n <= 8192 (and a batch of at most
    64); a selected metric that is not exactly a SparseEPE; no metric selected."""
    from . import sparse_epe
    from .metrics import SparseEPE
    img, ref = batch.get('image'), batch.get('image_ref')
    if not enabled() or not all(torch.is_tensor(t) and t.is_cuda and t.dim() == 4 for t in (img, ref)) or ref.device != img.device:
        return False
    B, dev = img.shape[0], img.device
    pts_ref, pts = batch.get('corr_pts_ref'), batch.get('corr_pts')
    if B > sparse_epe.MAX_BATCH or not (sparse_epe.points_ok(pts_ref, B, dev) and sparse_epe.points_ok(pts, B, dev)) or \
            any(a.shape[0] != b.shape[0] for a, b in zip(pts_ref, pts)):
        return False
    chosen = [m for k, m in metrics.items() if src_name in k]
    if not chosen or any(type(m) is not SparseEPE for m in chosen):
        return False
    flow, uncert = model.forward(img, ref)                 # (the same call, hence the same bits, as _eval_step's)
    if tuple(flow.shape[-2:]) != tuple(ref.shape[-2:]):
        raise AssertionError("AlignmentModel.forward: the flow is not at the reference image's resolution")
    if uncert is None and any(m.uncertainty_estimation for m in chosen):
        raise RuntimeError("SparseEPE(uncertainty_estimation=True) on a matcher whose head estimates no uncertainty")
    rows = sparse_epe.sparse_epe_rows(flow.float(), pts_ref, pts, None if uncert is None else uncert.float())
    for m in chosen:
        m.add_rows(rows)
    return True


def eval_step(model, metrics, batch, src_name):
    """The fused validation / test step: one kernel call, its count matrix added to every metric of this dataset.  -> True when
    it ran; False when a condition does not hold (RFN_EVAL_FUSED=0; not a segmentation model with crop_logits; tensors not on
    the device; more than 32 classes; the label not a (B, Ho, Wo) int64 tensor with 0 < B * Ho * Wo < 2^31 -- Ho x Wo need not
    be the image's size; a selected metric that is not an IoU over the head's classes with one common ignore_index; no metric
    selected) -- the caller then runs the model's own step.  An AlignmentModel takes the matcher's fused step
    (_matcher_eval_step: one sparse-EPE kernel per batch) under its own conditions."""
    from .alignment_model import AlignmentModel
    from .metrics import IoU
    if isinstance(model, AlignmentModel):
        return _matcher_eval_step(model, metrics, batch, src_name)
    x, y = batch.get('image'), batch.get('semantic')
    if not _model_ok(model, x) or not torch.is_tensor(y) or not y.is_cuda or y.dtype != torch.int64 or y.dim() != 3 or \
            y.shape[0] != x.shape[0] or not 0 < y.numel() < 2 ** 31:
        return False
    chosen = [m for k, m in metrics.items() if src_name in k]
    C = model.head.num_classes
    if not chosen or any(not isinstance(m, IoU) or m.num_classes != C or m.ignore_index is None for m in chosen) or \
            len({int(m.ignore_index) for m in chosen}) != 1:
        return False
    delta = confusion(model, x, y, chosen[0].ignore_index)
    for m in chosen:
        m.add_confusion(delta)
    return True


def predict_step(model, batch, save_dir, orig_size=None, dataset_name=None, resize=False):
    """The fused predict step -> the (B, H, W) uint8 label maps written (numpy), or None when a condition does not hold.
    `orig_size` other than the image size: with `resize` the maps come from labels_resized() at that size, without it None."""
    x = batch.get('image')
    if not _model_ok(model, x):
        return None
    if orig_size is None or tuple(int(v) for v in orig_size) == tuple(x.shape[-2:]):
        preds = labels(model, x)
    elif resize:
        preds = labels_resized(model, x, orig_size)
    else:
        return None
    preds = preds.cpu().numpy()
    if save_dir is not None:
        model.write_label_pngs(preds, batch['filename'], save_dir, dataset_name)
    return preds

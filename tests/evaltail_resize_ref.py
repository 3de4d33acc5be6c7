"""The float64 restatement of forward(x, out_size) for the resized evaluation tail (a plain helper module like guardband.py; used
by test_evaltail_resize_gpu.py, test_evaltail_resize_guardband_gpu.py and test_evaltail_resize_cpu.py).

Stage one is test_evaltail_gpu.restate's mean: per box F.interpolate(logits.double(), size=box size, bilinear,
align_corners=False) on the CPU, summed into a float64 image, divided by the cover count.  Stage two is
F.interpolate(mean, size=(Ho, Wo), bilinear, align_corners=False) in float64.  A pixel of the (Ho, Wo) grid is DECIDED when the
gap between its two largest classes exceeds 1e-4 * max|logit| -- the rule of test_evaltail_gpu.py.  The fp32 form of the same
chain differs from float64 by at most 4.8e-5 on the inputs of the GPU tests (measured on the CPU, per case in CASES' comments)
while the threshold there is 1.0e-3 to 1.4e-3: a correct kernel cannot disagree on a decided pixel.

Every result is computed once per distinct input and shared (the cache is keyed by the case, the tensors are not modified)."""
import torch
import torch.nn.functional as F
from test_evaltail_gpu import DTYPES, slide_boxes      # (that module needs no device to be imported)


def mean64(logits, boxes, H, W):
    """float64 on the CPU -> the mean over the covering boxes of the up-sampled crop logits, (B, C, H, W)."""
    lg = logits.detach().cpu().double()
    B = lg.shape[0] // len(boxes)
    acc = torch.zeros(B, lg.shape[1], H, W, dtype=torch.float64)
    cnt = torch.zeros(B, 1, H, W, dtype=torch.float64)
    for k, (y1, y2, x1, x2) in enumerate(boxes):
        acc[:, :, y1:y2, x1:x2] += F.interpolate(lg[k * B:(k + 1) * B], size=(y2 - y1, x2 - x1), mode="bilinear",
                                                 align_corners=False)
        cnt[:, :, y1:y2, x1:x2] += 1
    assert int((cnt == 0).sum()) == 0
    return acc / cnt


def restate_resized(logits, boxes, H, W, Ho, Wo):
    """-> (arg-max (B, Ho, Wo) int64, decided (B, Ho, Wo) bool) of the two-stage float64 restatement."""
    out = F.interpolate(mean64(logits, boxes, H, W), size=(Ho, Wo), mode="bilinear", align_corners=False)
    top = out.topk(2, dim=1).values
    return out.argmax(1), (top[:, 0] - top[:, 1]) > 1e-4 * float(logits.detach().abs().max())


_CASES = {}


def case(B, C, H, W, crop, stride, lo, out, dtype):
    """The seeded inputs of one table row and their restatement -> (logits on the CPU, boxes, want, decided); shared, read-only."""
    key = (B, C, H, W, crop, stride, lo, out, dtype)
    if key not in _CASES:
        boxes = [(0, H, 0, W)] if crop is None else slide_boxes(H, W, crop, stride)
        g = torch.Generator().manual_seed(0)
        logits = (3 * torch.randn(len(boxes) * B, C, *lo, generator=g)).to(DTYPES[dtype])
        _CASES[key] = (logits, boxes, *restate_resized(logits, boxes, H, W, *out))
    return _CASES[key]

"""tests/golden/make_golden_rotate.py -- golden of the labelled RobotCar section's geometry and draws
(configs/cityscapes_robotcar/refign_*.yaml: RandomRotation -> ToTensor -> RandomCrop -> ColorJitter -> RandomHorizontalFlip).

Part 1, Pillow alone: `Image.rotate(angle, NEAREST)` of seeded uint8 images (fill 0), label maps (fill 255) and the all-zero
mode-"1" mask (fill 1) at 5 x 7, 37 x 53 and 64 x 16 (720 x 720 is checked against Pillow where it is installed, and against the
restatement on the device: its pixels would not fit a committed file).

Part 2, the reference's own classes (data_modules/transforms.py:206-247, 282-413) run as that pipeline, two samples in a row per
seed, imported as make_golden_data.py imports them (_ref_import + its stubs()).  torchvision is not installed; the bases are
STAND-INS for third-party behaviour: RandomRotation.get_params draws float(torch.empty(1).uniform_(lo, hi).item()) over
(-degrees, degrees) and functional.rotate calls PIL's Image.rotate, as torchvision documents for a PIL image; ColorJitter draws
torch.randperm(4), then torch.empty(1).uniform_(lo, hi) for brightness, contrast, saturation and hue (get_params' order),
records them and returns the image untouched -- the pixel arithmetic is not part of this golden; pil_to_tensor is
torch.as_tensor(np.array(pic)) with the channels first.  What is the reference's own -- the key dispatch, the rotation of
image, label (fill 255) and normalize_mask (fill 1), RandomCrop with its category-ratio re-draws, the flip coin -- runs as it
stands.  Recorded: the draws, the rotated + cropped + mirrored image, label and mask, and where both streams stand afterwards.
    python tests/golden/make_golden_rotate.py      ->  rotate_pillow.npz"""
import os
import random
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SHAPES = ((5, 7), (37, 53), (64, 16))
ANGLES = (10.0, -10.0, 0.5, -0.001, 3.3333, 45.0, -37.2)
N_SEEDED = 12                                                  # more of U(-10, 10), seeded
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
SAMPLES = 2
DIMS, CROP, DEGREES, CAT_MAX_RATIO = (40, 56), (32, 48), 10, 0.75
JITTER = dict(brightness=0.25, contrast=0.25, saturation=0.25, hue=0.1)
LOG = {"angle": [], "order": [], "factors": [], "coin": []}


def rotations():
    rng = np.random.default_rng(2024)
    angles = np.concatenate([np.array(ANGLES), rng.uniform(-10.0, 10.0, N_SEEDED)])
    out = {"angles": angles}
    for h, w in SHAPES:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        lbl = rng.integers(0, 19, (h, w), dtype=np.uint8)
        out[f"image_{h}x{w}"], out[f"label_{h}x{w}"] = img, lbl
        ri, rl, rm = [], [], []
        for a in angles.tolist():
            ri.append(np.asarray(Image.fromarray(img).rotate(a, Image.NEAREST, False, None, fillcolor=0)))
            rl.append(np.asarray(Image.fromarray(lbl).rotate(a, Image.NEAREST, False, None, fillcolor=255)))
            rm.append(np.asarray(Image.new("1", (w, h), 0).rotate(a, Image.NEAREST, False, None, fillcolor=1)))
        out[f"rot_image_{h}x{w}"], out[f"rot_label_{h}x{w}"] = np.stack(ri), np.stack(rl)
        out[f"rot_mask_{h}x{w}"] = np.stack(rm).astype(bool)
    return out


class RotationStandIn(torch.nn.Module):
    def __init__(self, degrees, expand=False, center=None, fill=0):
        super().__init__()
        self.degrees, self.resample, self.expand, self.center, self.fill = (-float(degrees), float(degrees)), Image.NEAREST, expand, \
            center, fill

    @staticmethod
    def get_params(degrees):
        angle = float(torch.empty(1).uniform_(float(degrees[0]), float(degrees[1])).item())
        LOG["angle"].append(angle)
        return angle


class JitterStandIn(torch.nn.Module):
    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        super().__init__()
        self.ranges = [(max(0.0, 1.0 - v), 1.0 + v) for v in (brightness, contrast, saturation)] + [(-hue, hue)]

    def forward(self, img):
        LOG["order"].append(torch.randperm(4).tolist())
        LOG["factors"].append([float(torch.empty(1).uniform_(lo, hi)) for lo, hi in self.ranges])
        return img


def pil_to_tensor(pic):
    a = torch.as_tensor(np.array(pic, copy=True))
    return a.view(pic.size[1], pic.size[0], len(pic.getbands())).permute(2, 0, 1)


def sample_set(n):
    """decoded samples at DIMS: label maps of 8 x 8 blocks with a dominant class (so that RandomCrop re-draws) and ignore pixels"""
    rng = np.random.default_rng(7)
    out = []
    for i in range(n):
        coarse = rng.integers(0, 6, (DIMS[0] // 8, DIMS[1] // 8), dtype=np.uint8)
        coarse[rng.random(coarse.shape) < 0.6] = i % 3
        lbl = np.repeat(np.repeat(coarse, 8, 0), 8, 1)
        lbl[rng.random(DIMS) < 0.03] = 255
        out.append((rng.integers(0, 256, (*DIMS, 3), dtype=np.uint8), lbl))
    return out


def draws():
    import _ref_import as R
    from make_golden_data import stubs
    R.setup()
    stubs()
    tt, tf = sys.modules["torchvision.transforms"], sys.modules["torchvision.transforms.functional"]
    tt.RandomRotation, tt.ColorJitter = RotationStandIn, JitterStandIn
    tf.rotate = lambda img, angle, resample, expand, center, fill: img.rotate(angle, resample, expand, center, fillcolor=fill)
    tf.pil_to_tensor = pil_to_tensor
    tr = R.ref_module("data_modules.transforms")
    pipeline = [tr.RandomRotation(degrees=DEGREES), tr.ToTensor(), tr.RandomCrop(size=list(CROP), cat_max_ratio=CAT_MAX_RATIO),
                tr.ColorJitter(**JITTER), tr.RandomHorizontalFlip()]
    data = sample_set(len(SEEDS) * SAMPLES)
    real_random = random.random

    def coin():
        v = real_random()
        LOG["coin"].append(v)
        return v

    images, labels, masks, random_tail, torch_tail = [], [], [], [], []
    for i, seed in enumerate(SEEDS):
        random.seed(seed)
        torch.manual_seed(seed)
        random.random = coin
        try:
            for j in range(SAMPLES):
                img, lbl = data[i * SAMPLES + j]
                sample = {"image": Image.fromarray(img), "semantic": Image.fromarray(lbl)}
                for t in pipeline:
                    sample = t(sample)
                images.append(sample["image"].numpy().copy())
                labels.append(sample["semantic"].numpy().copy())
                masks.append(sample["normalize_mask"].numpy().copy())
        finally:
            random.random = real_random
        random_tail.append([random.random() for _ in range(4)])
        torch_tail.append(torch.rand(4).numpy())
    n = len(SEEDS)
    return dict(seeds=np.array(SEEDS), dims=np.array(DIMS), crop=np.array(CROP), degrees=np.float64(DEGREES),
                cat_max_ratio=np.float64(CAT_MAX_RATIO), jitter=np.array([JITTER[k] for k in ("brightness", "contrast", "saturation", "hue")]),
                in_images=np.stack([d[0] for d in data]).reshape(n, SAMPLES, *DIMS, 3),
                in_labels=np.stack([d[1] for d in data]).reshape(n, SAMPLES, *DIMS),
                angle=np.array(LOG["angle"], np.float64).reshape(n, SAMPLES), order=np.array(LOG["order"], np.int64).reshape(n, SAMPLES, 4),
                factors=np.array(LOG["factors"], np.float64).reshape(n, SAMPLES, 4), coin=np.array(LOG["coin"], np.float64).reshape(n, SAMPLES),
                out_images=np.stack(images).reshape(n, SAMPLES, 3, *CROP), out_labels=np.stack(labels).reshape(n, SAMPLES, *CROP),
                out_masks=np.stack(masks).reshape(n, SAMPLES, *CROP).astype(bool),
                random_tail=np.array(random_tail), torch_tail=np.stack(torch_tail))


def main():
    arrays = rotations()
    arrays.update({"draw_" + k: v for k, v in draws().items()})
    assert arrays["draw_out_masks"].any() and (arrays["draw_coin"] < 0.5).any() and (arrays["draw_coin"] >= 0.5).any()
    path = os.path.join(HERE, "rotate_pillow.npz")
    np.savez_compressed(path, **arrays)
    print(f"  wrote rotate_pillow.npz  ({os.path.getsize(path) / 1000:.1f} kB)")


if __name__ == "__main__":
    main()

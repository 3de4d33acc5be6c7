"""tests/golden/make_golden_photometric.py -- golden of the photometric chain's DRAWS: the reference's own ColorJitter,
ChannelShuffle and RandomGaussianBlur (data_modules/transforms.py:393-519) run as a pipeline on a 3 x 2 x 2 ramp, two samples
in a row per seed.  The reference's modules are imported as make_golden_data.py imports them (_ref_import + its stubs()).

torchvision is not installed.  The reference's three classes are thin subclasses of torchvision's; what is the reference's
own -- the key dispatch, `random.shuffle(indices); val[indices]`, the coin `random.random() < self.p` -- runs here as it stands.
The torchvision bases are STAND-INS for third-party behaviour: they make the draws torchvision's get_params document
(ColorJitter: torch.randperm(4), then torch.empty(1).uniform_(lo, hi) for each enabled factor over [max(0, 1 - v), 1 + v];
GaussianBlur: torch.empty(1).uniform_(sigma_min, sigma_max)), record them and return the image untouched: the pixel arithmetic
is not part of this golden.  random.random is wrapped to record the coin.
    python tests/golden/make_golden_photometric.py      ->  photometric_draws.npz"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
SAMPLES = 2
JITTER = dict(brightness=0.6, contrast=0.6, saturation=0.6, hue=0)
BLUR = dict(p=0.5, kernel_size=7, sigma=(0.2, 2.0))           # p 0.5: both outcomes of the coin among the seeds
LOG = {"order": [], "factors": [], "sigma": [], "coin": []}


def ramp():
    return torch.arange(12, dtype=torch.uint8).reshape(3, 2, 2)


class JitterStandIn(torch.nn.Module):
    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        super().__init__()
        assert hue == 0
        self.ranges = [None if v == 0 else (max(0.0, 1.0 - v), 1.0 + v) for v in (brightness, contrast, saturation)]

    def forward(self, img):
        LOG["order"].append(torch.randperm(4).tolist())
        LOG["factors"].append([float("nan") if r is None else float(torch.empty(1).uniform_(r[0], r[1])) for r in self.ranges])
        return img


class BlurStandIn(torch.nn.Module):
    def __init__(self, kernel_size, sigma=(0.1, 2.0)):
        super().__init__()
        self.kernel_size, self.sigma = kernel_size, sigma

    def forward(self, img):
        LOG["sigma"][-1] = torch.empty(1).uniform_(self.sigma[0], self.sigma[1]).item()
        return img


def main():
    import _ref_import as R
    from make_golden_data import stubs
    R.setup()
    stubs()
    tt = sys.modules["torchvision.transforms"]
    tt.ColorJitter, tt.GaussianBlur = JitterStandIn, BlurStandIn
    tr = R.ref_module("data_modules.transforms")
    keys = ["image_prime"]
    pipeline = [tr.ColorJitter(apply_keys=keys, **JITTER), tr.ChannelShuffle(apply_keys=keys),
                tr.RandomGaussianBlur(apply_keys=keys, **BLUR)]
    real_random = random.random

    def coin():
        v = real_random()
        LOG["coin"].append(v)
        LOG["sigma"].append(float("nan"))
        return v

    shuffled, random_tail, torch_tail = [], [], []
    for seed in SEEDS:
        random.seed(seed)
        torch.manual_seed(seed)
        random.random = coin
        try:
            for _ in range(SAMPLES):
                sample = {"image_prime": ramp()}
                for t in pipeline:
                    sample = t(sample)
                shuffled.append(sample["image_prime"].numpy().copy())
        finally:
            random.random = real_random
        random_tail.append([random.random() for _ in range(4)])
        torch_tail.append(torch.rand(4).numpy())
    n = len(SEEDS)
    arrays = dict(seeds=np.array(SEEDS), brightness=np.float64(JITTER["brightness"]), contrast=np.float64(JITTER["contrast"]),
                  saturation=np.float64(JITTER["saturation"]), p=np.float64(BLUR["p"]), kernel_size=np.int64(BLUR["kernel_size"]),
                  sigma_range=np.array(BLUR["sigma"], np.float64),
                  order=np.array(LOG["order"], np.int64).reshape(n, SAMPLES, 4),
                  factors=np.array(LOG["factors"], np.float64).reshape(n, SAMPLES, 3),
                  shuffled=np.stack(shuffled).reshape(n, SAMPLES, 3, 2, 2),
                  coin=np.array(LOG["coin"], np.float64).reshape(n, SAMPLES),
                  sigma=np.array(LOG["sigma"], np.float64).reshape(n, SAMPLES),
                  random_tail=np.array(random_tail), torch_tail=np.stack(torch_tail))
    blurred = int(np.isfinite(arrays["sigma"]).sum())
    assert 0 < blurred < n * SAMPLES, "the seeds must show both outcomes of the coin"
    path = os.path.join(HERE, "photometric_draws.npz")
    np.savez_compressed(path, **arrays)
    print(f"  wrote photometric_draws.npz  ({os.path.getsize(path) / 1000:.1f} kB; {blurred} of {n * SAMPLES} samples blurred)")


if __name__ == "__main__":
    main()

"""The photometric chain on the matcher's `image_prime` on the device (csrc/photometric.hip): data_modules/transforms.py's
ColorJitter (brightness, contrast, saturation; hue 0), ChannelShuffle and RandomGaussianBlur on the uint8 image, followed by
ConvertImageDtype and Normalize -- one fused pass that stores nothing but the normalised fp32 image flowsynth.synthesize reads.
In the reference this runs per sample in the data-loader workers on the CPU.

Host side (this file): the DRAWS, where the pipeline makes them and in its order, so that both random streams stand afterwards
where the reference leaves them.  One sample:
    torch.randperm(4)                                 the order of the four jitter steps
    torch.empty(1).uniform_(lo, hi)                   brightness, contrast, saturation -- each enabled one, in this order
    random.shuffle of [0, 1, 2]                       ChannelShuffle
    random.random()                                   RandomGaussianBlur's coin, and only if it is < p:
    torch.empty(1).uniform_(sigma_lo, sigma_hi)       the blur's sigma
and the 7 x 7 blur weights, formed with the fp32 torch calls on the CPU that torchvision makes.
Device side: a dozen scalars and 49 weights per sample go up through pinned memory as one record each; one launch sums gray()
per sample as integers (only when some sample has a contrast step), one applies the chain.  Nothing here waits for the device.

The three classes are thin subclasses of torchvision's; the pixel arithmetic is torchvision's tensor path for uint8 images
(functional_tensor.py, 0.9 to 0.15) RESTATED.  torchvision is installed neither where this was written nor where it was
tested: parity with torchvision itself is NOT verified.  Two places where bits may differ from it: the contrast mean is the
exact integer sum divided once (torch's fp32 mean of a large image is a cascade sum that is not), and the order of the blur's
49-tap fp32 sum (row-major here, unspecified inside conv2d)."""
import random

import numpy as np
import torch

from . import _lib
from ._tensor import ptr, upload_async
from .datastep import IMNET_MEAN, IMNET_STD

STEPS = ("brightness", "contrast", "saturation", "hue")    # ColorJitter.forward's step numbers
MAX_KERNEL = 7
RECORD_WORDS = 80                                          # include/refign_hip.h: the record's words


class PhotoParams:
    """One sample's parameters.  order: the four step numbers as drawn; brightness / contrast / saturation: the factor as the
    Python float of the fp32 draw, or None (no step); perm: out[c] = in[perm[c]]; coin: RandomGaussianBlur's draw or None;
    sigma: the blur's sigma or None (no blur); kernel_size; kernel: the (7, 7) fp32 weights (a smaller kernel centred in zeros)
    or None; mean / std: Normalize's statistics."""

    def __init__(self, order, brightness, contrast, saturation, perm, sigma, kernel_size=MAX_KERNEL, coin=None,
                 mean=IMNET_MEAN, std=IMNET_STD):
        self.order, self.perm = [int(v) for v in order], [int(v) for v in perm]
        if sorted(self.order) != [0, 1, 2, 3]:
            raise ValueError(f"photometric: order {self.order} is no permutation of the four steps {STEPS}")
        if sorted(self.perm) != [0, 1, 2]:
            raise ValueError(f"photometric: perm {self.perm} is no permutation of the three channels")
        self.brightness, self.contrast, self.saturation = (None if v is None else float(v) for v in (brightness, contrast, saturation))
        self.coin, self.sigma, self.kernel_size = coin, None if sigma is None else float(sigma), int(kernel_size)
        self.kernel = None if sigma is None else blur_kernel(self.sigma, self.kernel_size)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3:
            raise ValueError("photometric: mean and std have three entries")

    @property
    def factors(self):
        return (self.brightness, self.contrast, self.saturation)

    def record(self):
        """the kernel's record: RECORD_WORDS 32-bit words (int32 array; the float fields hold their bits)"""
        rec = np.zeros(RECORD_WORDS, np.int32)
        flt = rec.view(np.float32)
        rec[0:4] = self.order
        for s, f in enumerate(self.factors):
            if f is not None:
                rec[4 + s] = 1
                flt[8 + s], flt[11 + s] = np.float32(f), np.float32(1.0 - f)      # 1.0 - f in double, rounded once
        rec[14:17] = self.perm
        flt[18:21], flt[21:24] = np.asarray(self.mean, np.float32), np.asarray(self.std, np.float32)
        if self.kernel is not None:
            rec[17] = 1
            flt[24:73] = self.kernel.reshape(-1).numpy()
        return rec


def blur_kernel(sigma, kernel_size=MAX_KERNEL):
    """torchvision's _get_gaussian_kernel2d for a square kernel, with its fp32 torch calls on the CPU: exp(-0.5 (x / sigma)^2)
    over linspace(-(k - 1) / 2, (k - 1) / 2, k), normalised, the outer product through torch.mm -- as a (7, 7) tensor, a
    smaller kernel centred in zeros (its zero taps add nothing to the sum)."""
    k = int(kernel_size)
    if k < 1 or k % 2 == 0 or k > MAX_KERNEL:
        raise ValueError(f"photometric: kernel_size {kernel_size} (odd, at most {MAX_KERNEL})")
    if not float(sigma) > 0.0:
        raise ValueError(f"photometric: sigma {sigma} (> 0)")
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k)
    pdf = torch.exp(-0.5 * (x / float(sigma)).pow(2))
    k1 = pdf / pdf.sum()
    out = torch.zeros(MAX_KERNEL, MAX_KERNEL, dtype=torch.float32)
    pad = (MAX_KERNEL - k) // 2
    out[pad:pad + k, pad:pad + k] = torch.mm(k1[:, None], k1[None, :])
    return out


def draw(plan):
    """One sample's PhotoParams, drawn as the pipeline ColorJitter -> ChannelShuffle -> RandomGaussianBlur draws them (the
    order: this module's docstring).  plan: config.photometric_plan(cfg)."""
    order = torch.randperm(4).tolist()
    factors = [None if plan.get(k) is None else float(torch.empty(1).uniform_(plan[k][0], plan[k][1]))
               for k in ("brightness", "contrast", "saturation")]
    perm = list(range(3))
    if plan.get("shuffle", True):
        random.shuffle(perm)
    blur, coin, sigma, ksize = plan.get("blur"), None, None, MAX_KERNEL
    if blur is not None:
        ksize = blur.get("kernel_size", MAX_KERNEL)
        coin = random.random()
        if coin < blur["p"]:
            sigma = torch.empty(1).uniform_(blur["sigma"][0], blur["sigma"][1]).item()
    return PhotoParams(order, *factors, perm, sigma, ksize, coin=coin, mean=plan.get("mean", IMNET_MEAN),
                       std=plan.get("std", IMNET_STD))


def params_from(order, brightness, contrast, saturation, perm, sigma, kernel_size=MAX_KERNEL, mean=IMNET_MEAN, std=IMNET_STD):
    """PhotoParams from explicit values, bypassing the draws: order a permutation of (0, 1, 2, 3); each factor a float or None
    (no such step); perm a permutation of (0, 1, 2); sigma a float or None (no blur)."""
    return PhotoParams(order, brightness, contrast, saturation, perm, sigma, kernel_size, mean=mean, std=std)


def _batch(image_u8, params, what):
    if not (torch.is_tensor(image_u8) and image_u8.is_cuda and image_u8.dtype == torch.uint8 and image_u8.dim() in (3, 4) and
            image_u8.shape[-3] == 3):
        raise RuntimeError(f"photometric.{what}: image must be a (B, 3, h, w) or (3, h, w) uint8 HIP (cuda:N) tensor: "
                           f"refign_amd has no CPU path")
    img = (image_u8 if image_u8.dim() == 4 else image_u8.unsqueeze(0)).contiguous()
    params = [params] if isinstance(params, PhotoParams) else list(params)
    B, _, h, w = img.shape
    if len(params) != B or B < 1:
        raise RuntimeError(f"photometric.{what}: {B} samples need as many parameter sets ({len(params)} given)")
    if min(h, w) < MAX_KERNEL // 2 + 1 and any(p.sigma is not None for p in params):
        raise RuntimeError(f"photometric.{what}: a {h} x {w} image cannot be blurred: reflect padding by {MAX_KERNEL // 2} needs "
                           f"at least {MAX_KERNEL // 2 + 1} pixels each way")
    records = upload_async(np.stack([p.record() for p in params]), torch.int32, img.device)
    return img, params, records


def _sums(img, params, records):
    """the (B,) int64 sums of gray() in front of each sample's contrast step, or None when no sample has one"""
    if all(p.contrast is None for p in params):
        return None
    B, _, h, w = img.shape
    sums = torch.empty(B, dtype=torch.int64, device=img.device)          # zeroed by the call, with a kernel
    _lib.call("rfn_photometric_gray_sums_u8", img.device, ptr(img), ptr(records), B, h, w, ptr(sums))
    return sums


def gray_sums(image_u8, params):
    """The contrast step's whole-image quantity alone: (B,) int64 on the device, per sample the integer sum of gray() of the image
    as it stands in front of the contrast step (0 for a sample without one).  The step's mean is (float)sum / (float)(h w)."""
    img, params, records = _batch(image_u8, params, "gray_sums")
    sums = _sums(img, params, records)
    return torch.zeros(len(params), dtype=torch.int64, device=img.device) if sums is None else sums


def apply(image_u8, params, out=None):
    """The chain over a batch: image_u8 (B, 3, h, w) or (3, h, w) uint8 on the device, params B PhotoParams (or one) ->
    (B, 3, h, w) fp32, ((u8 / 255) - mean) / std of the jittered, shuffled and (where the sample's sigma is set) blurred image.
    out: a contiguous fp32 (B, 3, h, w) tensor on the same device to write into.  No host synchronisation."""
    img, params, records = _batch(image_u8, params, "apply")
    B, _, h, w = img.shape
    if out is None:
        out = torch.empty((B, 3, h, w), dtype=torch.float32, device=img.device)
    elif not (torch.is_tensor(out) and out.device == img.device and out.dtype == torch.float32 and out.is_contiguous() and
              tuple(out.shape) == (B, 3, h, w)):
        raise RuntimeError(f"photometric.apply: out must be a contiguous float32 ({B}, 3, {h}, {w}) tensor on {img.device}")
    sums = _sums(img, params, records)
    _lib.call("rfn_photometric_apply_u8", img.device, ptr(img), ptr(records), ptr(sums), B, h, w, ptr(out))
    return out

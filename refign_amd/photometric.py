"""The photometric chain on the matcher's `image_prime` on the device (csrc/photometric.hip): data_modules/transforms.py's
ColorJitter (brightness, contrast, saturation, hue), ChannelShuffle and RandomGaussianBlur on the uint8 image, followed by
ConvertImageDtype and Normalize -- one fused pass that stores nothing but the normalised fp32 image flowsynth.synthesize reads.
In the reference this runs per sample in the data-loader workers on the CPU.  The labelled RobotCar section
(configs/cityscapes_robotcar/refign_*.yaml) runs the same ColorJitter behind RandomRotation and RandomCrop and in front of
RandomHorizontalFlip: `apply(..., geometry=)` gathers through the three (RotateCrop) in the same pass.

Host side (this file): the DRAWS, where the pipeline makes them and in its order, so that both random streams stand afterwards
where the reference leaves them.  One sample:
    torch.randperm(4)                                 the order of the four jitter steps
    torch.empty(1).uniform_(lo, hi)                   brightness, contrast, saturation, hue -- each enabled one, in this order
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
    or None; mean / std: Normalize's statistics; hue: the hue step's factor in [-0.5, 0.5], or None (no step)."""

    def __init__(self, order, brightness, contrast, saturation, perm, sigma, kernel_size=MAX_KERNEL, coin=None,
                 mean=IMNET_MEAN, std=IMNET_STD, hue=None):
        self.order, self.perm = [int(v) for v in order], [int(v) for v in perm]
        if sorted(self.order) != [0, 1, 2, 3]:
            raise ValueError(f"photometric: order {self.order} is no permutation of the four steps {STEPS}")
        if sorted(self.perm) != [0, 1, 2]:
            raise ValueError(f"photometric: perm {self.perm} is no permutation of the three channels")
        self.brightness, self.contrast, self.saturation = (None if v is None else float(v) for v in (brightness, contrast, saturation))
        self.hue = None if hue is None else float(hue)
        if self.hue is not None and not -0.5 <= self.hue <= 0.5:
            raise ValueError(f"photometric: hue {self.hue} (adjust_hue takes a factor in [-0.5, 0.5])")
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
        if self.hue is not None:
            rec[7], flt[73] = 1, np.float32(self.hue)
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
    hue = None if plan.get("hue") is None else float(torch.empty(1).uniform_(plan["hue"][0], plan["hue"][1]))
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
                       std=plan.get("std", IMNET_STD), hue=hue)


def params_from(order, brightness, contrast, saturation, perm, sigma, kernel_size=MAX_KERNEL, mean=IMNET_MEAN, std=IMNET_STD,
                hue=None):
    """PhotoParams from explicit values, bypassing the draws: order a permutation of (0, 1, 2, 3); each factor a float or None
    (no such step); perm a permutation of (0, 1, 2); sigma a float or None (no blur); hue a float in [-0.5, 0.5] or None."""
    return PhotoParams(order, brightness, contrast, saturation, perm, sigma, kernel_size, mean=mean, std=std, hue=hue)


GEOM_WORDS = 12                                            # include/refign_hip.h: the geometry record's words


class RotateCrop:
    """One sample's geometry in front of the chain: RandomRotation's angle in degrees (Pillow's NEAREST rotation about the
    centre, fill 0), RandomCrop's box (top, left, h, w) of the rotated image, RandomHorizontalFlip's outcome."""

    def __init__(self, angle, top, left, h, w, flip):
        self.angle, self.flip = float(angle), bool(flip)
        self.top, self.left, self.h, self.w = int(top), int(left), int(h), int(w)

    def record(self, H, W):
        """the kernel's geometry record for an (H, W) source: GEOM_WORDS int32"""
        from .resample import rotation_coefficients
        if not (0 <= self.top and 0 <= self.left and self.h >= 1 and self.w >= 1 and self.top + self.h <= H and
                self.left + self.w <= W):
            raise RuntimeError(f"photometric: the crop (top {self.top}, left {self.left}, {self.h} x {self.w}) does not lie in the "
                               f"{H} x {W} image")
        rec = np.zeros(GEOM_WORDS, np.int32)
        rec[0:6] = rotation_coefficients(self.angle, H, W)
        rec[6:9] = self.top, self.left, int(self.flip)
        return rec


def _batch(image_u8, params, what, geometry=None):
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
    if geometry is None:
        return img, params, records, None, (h, w)
    geometry = [geometry] if isinstance(geometry, RotateCrop) else list(geometry)
    if len(geometry) != B:
        raise RuntimeError(f"photometric.{what}: {B} samples need as many RotateCrop ({len(geometry)} given)")
    if any(p.sigma is not None or p.perm != [0, 1, 2] for p in params):
        raise RuntimeError(f"photometric.{what}: geometry goes with neither a blur (its tile assumes unrotated neighbours) nor a "
                           f"channel shuffle: no config combines them")
    if len({(g.h, g.w) for g in geometry}) != 1:
        raise RuntimeError(f"photometric.{what}: the samples of a batch share one crop size")
    geom = upload_async(np.stack([g.record(h, w) for g in geometry]), torch.int32, img.device)
    return img, params, records, geom, (geometry[0].h, geometry[0].w)


def _sums(img, params, records, geom=None, size=None):
    """the (B,) int64 sums of gray() in front of each sample's contrast step, or None when no sample has one"""
    if all(p.contrast is None for p in params):
        return None
    B, _, h, w = img.shape
    sums = torch.empty(B, dtype=torch.int64, device=img.device)          # zeroed by the call, with a kernel
    if geom is None:
        _lib.call("rfn_photometric_gray_sums_u8", img.device, ptr(img), ptr(records), B, h, w, ptr(sums))
    else:
        _lib.call("rfn_photometric_gray_sums_geom_u8", img.device, ptr(img), ptr(records), ptr(geom), B, h, w, size[0], size[1],
                  ptr(sums))
    return sums


def gray_sums(image_u8, params, geometry=None):
    """The contrast step's whole-image quantity alone: (B,) int64 on the device, per sample the integer sum of gray() of the image
    as it stands in front of the contrast step (0 for a sample without one).  The step's mean is (float)sum / (float)(h w).
    geometry: as in apply -- the sum runs over the gathered crop, fill pixels included."""
    img, params, records, geom, size = _batch(image_u8, params, "gray_sums", geometry)
    sums = _sums(img, params, records, geom, size)
    return torch.zeros(len(params), dtype=torch.int64, device=img.device) if sums is None else sums


def apply(image_u8, params, out=None, geometry=None):
    """The chain over a batch: image_u8 (B, 3, h, w) or (3, h, w) uint8 on the device, params B PhotoParams (or one) ->
    (B, 3, h, w) fp32, ((u8 / 255) - mean) / std of the jittered, shuffled and (where the sample's sigma is set) blurred image.
    out: a contiguous fp32 (B, 3, h, w) tensor on the same device to write into.  No host synchronisation.
    geometry: B RotateCrop (or one).  image_u8 is then the UNROTATED (B, 3, H, W) image and the result is (B, 3, h, w) of the
    crop: both launches gather each pixel through rotation, crop and mirror, so the rotated image is never stored.  A pixel whose
    source falls outside the image is the fill 0 in front of the chain (it counts in the contrast mean) and exactly 0.0 in the
    output, all three channels -- Normalize's normalize_mask write.  RuntimeError together with a blur or a channel shuffle."""
    img, params, records, geom, (h, w) = _batch(image_u8, params, "apply", geometry)
    B, _, H, W = img.shape
    if out is None:
        out = torch.empty((B, 3, h, w), dtype=torch.float32, device=img.device)
    elif not (torch.is_tensor(out) and out.device == img.device and out.dtype == torch.float32 and out.is_contiguous() and
              tuple(out.shape) == (B, 3, h, w)):
        raise RuntimeError(f"photometric.apply: out must be a contiguous float32 ({B}, 3, {h}, {w}) tensor on {img.device}")
    sums = _sums(img, params, records, geom, (h, w))
    if geom is None:
        _lib.call("rfn_photometric_apply_u8", img.device, ptr(img), ptr(records), ptr(sums), B, h, w, ptr(out))
    else:
        _lib.call("rfn_photometric_apply_geom_u8", img.device, ptr(img), ptr(records), ptr(geom), ptr(sums), B, H, W, h, w, ptr(out))
    return out

"""refign_amd/resample.py -- N4, third part: the LOAD-TIME resize of the reference's data sets on the device, bit-equal to Pillow.

What the reference does on the host before a sample reaches its transform pipeline:
  * every data set reader resizes at load time: datasets/cityscapes.py:119-127 is `Image.resize(dims[::-1], BILINEAR)` for images
    and NEAREST for labels (acdc.py, darkzurich.py, robotcar.py alike);
  * every `test:` / `predict:` section starts with data_modules.transforms.Resize (transforms.py:57-74,120-203).
Pillow's 8-bit resize is integer arithmetic over two small tables per axis (libImaging/Resample.c: `precompute_coeffs`,
`normalize_coeffs_8bpc`, `ImagingResampleHorizontal_8bpc` / `Vertical_8bpc`; NEAREST: Geometry.c `ImagingScaleAffine`), so it can be
restated exactly: the tables are made HERE on the host, in double as Pillow makes them, and the pixel work is csrc/resample.hip:
  resize_crop_flip_normalize   decoded uint8 HWC image -> the fp32 (3, h, w) crop of the RESIZED image that
                               datastep.crop_flip_normalize would give, in one kernel that reads only the crop's footprint;
  resize_u8 / resize_nearest_u8  Pillow's pixels themselves (image -> (3, Hd, Wd) uint8, label map -> (Hd, Wd) uint8).
`resize_reference` / `resize_nearest_reference` are numpy restatements: the documentation of the arithmetic and the tests' operand
(tests/test_resample_*.py against tests/golden/resample_pillow.npz, made with Pillow alone)."""
import math

import numpy as np
import torch

from . import _lib
from ._tensor import ptr
from .datastep import IMNET_MEAN, IMNET_STD

PRECISION_BITS = 32 - 8 - 2      # Resample.c: 8 bits of pixel, 2 spare bits for the accumulation


# ------------------------------------------------------------------ host tables
def bilinear_tables(in_size, out_size):
    """Pillow's `precompute_coeffs` (bilinear: support 1) + `normalize_coeffs_8bpc` for one axis ->
    (xmin[out] int32, n[out] int32, coef[out, kmax] int32): output pixel xx = (sum_k in[xmin[xx] + k] * coef[xx, k] + 2^21) >> 22
    over k < n[xx]; coef beyond n is 0.  kmax = ceil(support) * 2 + 1 with support = max(in / out, 1)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("bilinear_tables: sizes must be positive")
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    kmax = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xmin = np.zeros(out_size, np.int32)
    n = np.zeros(out_size, np.int32)
    coef = np.zeros((out_size, kmax), np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)                       # C's (int): truncation (the operands are >= 0 after max)
        hi = min(int(center + support + 0.5), in_size)
        cnt = hi - lo
        w = [max(1.0 - abs((x + lo - center + 0.5) * ss), 0.0) for x in range(cnt)]
        ww = 0.0
        for v in w:                                                    # left to right, in double
            ww += v
        for x in range(cnt):
            k = w[x] / ww if ww != 0.0 else w[x]
            coef[xx, x] = int(-0.5 + k * one) if k < 0 else int(0.5 + k * one)   # half away from zero
        xmin[xx], n[xx] = lo, cnt
    return xmin, n, coef


def nearest_table(in_size, out_size):
    """ImagingScaleAffine's `xintab` (Geometry.c): xo = a * 0.5; out[x] = (int)xo; xo += a with a = in / out in double.  The
    ACCUMULATION is the point: at some sizes it lands one pixel away from the product (x + 0.5) * a."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("nearest_table: sizes must be positive")
    a = float(in_size) / out_size
    tab = np.zeros(out_size, np.int32)
    xo = a * 0.5
    for x in range(out_size):
        tab[x] = min(int(xo), in_size - 1)
        xo += a
    return tab


def target_size(h, w, size, only_if_larger=False):
    """The size arithmetic of transforms.Resize.__call__ / imresize (transforms.py:57-74,142-152) -> (new_h, new_w) of an (h, w)
    image.  `size`: int = the shorter side (the longer one int(size * long / short)), or (h, w).  only_if_larger (size a pair):
    unchanged when min(size[0] / h, size[1] / w) >= 1, else both sides scaled by that ratio and rounded."""
    h, w = int(h), int(w)
    if only_if_larger:
        ratio = min(size[0] / h, size[1] / w)
        if ratio >= 1:
            return h, w
        size = (int(round(ratio * h)), int(round(ratio * w)))
    if isinstance(size, (list, tuple)) and len(size) == 1:
        size = size[0]
    if isinstance(size, int):
        short, long = (w, h) if w <= h else (h, w)
        if short == size:
            return h, w
        new_short, new_long = size, int(size * long / short)
        new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
        return new_h, new_w
    return int(size[0]), int(size[1])


# ------------------------------------------------------------------ numpy restatements (tests, documentation)
def _pass_reference(img, axis, out_size):
    """one 8-bit pass along `axis` of an (H, W, C) uint8 array: uint8 out, rounded and clipped as Pillow does between the passes"""
    xmin, n, coef = bilinear_tables(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.int64)
    for xx in range(out_size):
        k = coef[xx, :n[xx]].astype(np.int64).reshape((-1,) + (1,) * (src.ndim - 1))
        out[xx] = ((src[xmin[xx]:xmin[xx] + n[xx]] * k).sum(0) + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize_reference(img_hwc_u8, size):
    """`Image.fromarray(img).resize((w, h), BILINEAR)` of an (H, W, C) uint8 array -> (h, w, C) uint8: the horizontal pass to a
    uint8 intermediate, then the vertical one; a pass is skipped when its axis keeps its size."""
    img = np.ascontiguousarray(img_hwc_u8)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError("resize_reference: an (H, W, C) uint8 array is required")
    h, w = int(size[0]), int(size[1])
    if img.shape[1] != w:
        img = _pass_reference(img, 1, w)
    if img.shape[0] != h:
        img = _pass_reference(img, 0, h)
    return np.ascontiguousarray(img)


def resize_nearest_reference(lbl_u8, size):
    """`Image.fromarray(lbl).resize((w, h), NEAREST)` of an (H, W) uint8 array -> (h, w) uint8"""
    lbl = np.asarray(lbl_u8)
    if lbl.dtype != np.uint8 or lbl.ndim != 2:
        raise ValueError("resize_nearest_reference: an (H, W) uint8 array is required")
    h, w = int(size[0]), int(size[1])
    if lbl.shape == (h, w):
        return lbl.copy()
    return np.ascontiguousarray(lbl[nearest_table(lbl.shape[0], h)][:, nearest_table(lbl.shape[1], w)])


# ------------------------------------------------------------------ device tables
_TABLES = {}


def _device_tables(kind, in_size, out_size, device):
    """cached per (kind, in, out, device).  bilinear: (bounds int32 [out, 2] = (xmin, n), coef int32 [out, kmax], kmax);
    nearest: int32 [out]"""
    key = (kind, int(in_size), int(out_size), device)
    t = _TABLES.get(key)
    if t is None:
        if kind == "bilinear":
            xmin, n, coef = bilinear_tables(in_size, out_size)
            t = (torch.from_numpy(np.stack([xmin, n], 1).copy()).to(device), torch.from_numpy(coef).to(device), coef.shape[1])
        else:
            t = torch.from_numpy(nearest_table(in_size, out_size)).to(device)
        if len(_TABLES) < 1024:      # cached tables are never freed (streams other than the one they were made on may be reading
            _TABLES[key] = t         # them); past that many size pairs a table lives for its call, on the current stream
    return t


def _check_image(image, who):
    if not image.is_cuda:
        raise RuntimeError(f"{who}: device tensors required (the product path has no CPU fallback)")
    if not (image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3 and image.is_contiguous()):
        raise RuntimeError(f"{who}: image must be a contiguous (H, W, 3) uint8 tensor (the decoded image, channels last)")


# ------------------------------------------------------------------ device functions
def resize_u8(image_hwc_u8, size):
    """Pillow's bilinear resize of a decoded (H, W, 3) uint8 DEVICE image -> (3, h, w) uint8 (what ToTensor would leave)"""
    _check_image(image_hwc_u8, "resize_u8")
    H, W, _ = image_hwc_u8.shape
    Hd, Wd = int(size[0]), int(size[1])
    dev = image_hwc_u8.device
    bx, cx, kx = _device_tables("bilinear", W, Wd, dev)
    by, cy, ky = _device_tables("bilinear", H, Hd, dev)
    out = torch.empty((3, Hd, Wd), dtype=torch.uint8, device=dev)
    _lib.call("rfn_resize_u8", dev, ptr(image_hwc_u8), H, W, Hd, Wd, ptr(bx), ptr(cx), kx, ptr(by), ptr(cy), ky, ptr(out))
    return out


def resize_nearest_u8(label_u8, size):
    """Pillow's NEAREST resize of an (H, W) uint8 DEVICE label map -> (h, w) uint8"""
    if not label_u8.is_cuda:
        raise RuntimeError("resize_nearest_u8: device tensors required (the product path has no CPU fallback)")
    if not (label_u8.dtype == torch.uint8 and label_u8.dim() == 2 and label_u8.is_contiguous()):
        raise RuntimeError("resize_nearest_u8: label must be a contiguous (H, W) uint8 tensor")
    H, W = label_u8.shape
    Hd, Wd = int(size[0]), int(size[1])
    dev = label_u8.device
    ty, tx = _device_tables("nearest", H, Hd, dev), _device_tables("nearest", W, Wd, dev)
    out = torch.empty((Hd, Wd), dtype=torch.uint8, device=dev)
    _lib.call("rfn_resize_nearest_u8", dev, ptr(label_u8), H, W, Hd, Wd, ptr(ty), ptr(tx), ptr(out))
    return out


def resize_crop_flip_normalize(image_hwc_u8, dims, top, left, h, w, flip, out_image=None, mean=IMNET_MEAN, std=IMNET_STD):
    """load-time resize to `dims` = (Hd, Wd) + crop (top, left, h, w) of the RESIZED image + RandomHorizontalFlip +
    ConvertImageDtype + Normalize of a decoded (H, W, 3) uint8 DEVICE image in one kernel, written into `out_image` (3, h, w)
    fp32 (a slot of a batch tensor) or a fresh tensor: bit for bit datastep.crop_flip_normalize of Pillow's resized image."""
    _check_image(image_hwc_u8, "resize_crop_flip_normalize")
    H, W, _ = image_hwc_u8.shape
    Hd, Wd = int(dims[0]), int(dims[1])
    dev = image_hwc_u8.device
    if out_image is None:
        out_image = torch.empty((3, h, w), dtype=torch.float32, device=dev)
    if not (out_image.dtype == torch.float32 and tuple(out_image.shape) == (3, h, w) and out_image.is_contiguous()):
        raise RuntimeError("resize_crop_flip_normalize: out_image must be a contiguous (3, h, w) float32 tensor")
    bx, cx, kx = _device_tables("bilinear", W, Wd, dev)
    by, cy, ky = _device_tables("bilinear", H, Hd, dev)
    m = np.asarray(mean, dtype=np.float32).copy()
    s = np.asarray(std, dtype=np.float32).copy()
    _lib.call("rfn_resize_crop_flip_norm_u8", dev, ptr(image_hwc_u8), H, W, Hd, Wd, ptr(bx), ptr(cx), kx, ptr(by), ptr(cy), ky,
              int(top), int(left), int(h), int(w), 1 if flip else 0, m.ctypes.data, s.ctypes.data, ptr(out_image))
    return out_image


class EvalIngest:
    """The val / test / predict pipelines of the reference's configs from decoded files to the tensors Trainer.validate / test /
    predict take: load-time `dims` (image bilinear, label nearest), an optional transforms.Resize (`resize`: int or (h, w);
    `img_only`: the label keeps its size, as in refign_*.yaml `test:`), ConvertImageDtype, Normalize.  Two successive resizes are
    two Pillow resizes with a uint8 image in between (they are NOT merged: the intermediate rounding is part of the result); the
    last one is fused with the conversion (a whole-image crop, no flip).
    __call__(image, semantic=None, image_ref=None) -> {"image" (1, 3, h, w) fp32[, "image_ref"][, "semantic" (1, h', w') int64]};
    images are (H, W, 3) uint8, the label (H, W) uint8, host arrays / tensors (uploaded) or device tensors."""

    def __init__(self, dims=None, resize=None, img_only=False, mean=IMNET_MEAN, std=IMNET_STD, only_if_larger=False, device=None):
        self.device = torch.device(device) if device is not None else None      # None: the input's device, else the current one
        self.dims = None if dims is None else (int(dims[0]), int(dims[1]))
        self.resize, self.img_only, self.only_if_larger = resize, bool(img_only), bool(only_if_larger)
        self.mean, self.std = mean, std

    def _sizes(self, h, w):
        """the chain of sizes an (h, w) input runs through (identity steps dropped)"""
        chain = []
        for step in (self.dims, self.resize):
            if step is None:
                continue
            nh, nw = target_size(h, w, step, self.only_if_larger) if step is self.resize else step
            if (nh, nw) != (h, w):
                chain.append((nh, nw))
                h, w = nh, nw
        return chain

    def _upload(self, x):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.is_cuda:
            return x
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError("EvalIngest: a HIP device is required (the product path has no CPU fallback)")
        return x.to(dev, non_blocking=True)

    def image(self, image_hwc_u8):
        x = self._upload(image_hwc_u8)
        _check_image(x, "EvalIngest")
        chain = self._sizes(x.shape[0], x.shape[1])
        for size in chain[:-1]:                                         # Pillow's uint8 image in between, channels last again
            x = resize_u8(x, size).permute(1, 2, 0).contiguous()
        h, w = chain[-1] if chain else (x.shape[0], x.shape[1])
        return resize_crop_flip_normalize(x, (h, w), 0, 0, h, w, False, None, self.mean, self.std).unsqueeze(0)

    def label(self, label_u8):
        y = self._upload(label_u8)
        steps = (self.dims,) if self.img_only else (self.dims, self.resize)
        for step in steps:
            if step is None:
                continue
            size = target_size(y.shape[0], y.shape[1], step, self.only_if_larger) if step is self.resize else step
            if tuple(size) != tuple(y.shape):
                y = resize_nearest_u8(y, size)
        return y.to(torch.int64).unsqueeze(0)

    def __call__(self, image, semantic=None, image_ref=None):
        out = {"image": self.image(image)}
        if image_ref is not None:
            out["image_ref"] = self.image(image_ref)
        if semantic is not None:
            out["semantic"] = self.label(semantic)
        return out

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
(tests/test_resample_*.py against tests/golden/resample_pillow.npz, made with Pillow alone).

The matcher's side (datasets/megadepth.py, robotcarmatching.py; the `test:` sections of megadepth/uawarpc_*.yaml) resizes with
Pillow's LANCZOS filter and ends in transforms.PadBottomRight: `filter_tables(in, out, "lanczos")` are the same tables for that
filter (negative taps: every row is checked against the int32 accumulator), `filter="lanczos"` / `pad_to=` select them in the
device functions, `lanczos_reference` restates the pixels (tests/test_lanczos_*.py against tests/golden/lanczos_pillow.npz), and
EvalIngest scales the sparse correspondences the way the reference does (`scale_points`).

transforms.RandomRotation (transforms.py:206-247; the labelled RobotCar section) rotates the PIL image, the label map and an
all-zero mask with `Image.rotate(angle, NEAREST)`: Pillow's fixed-point affine transform (Geometry.c `affine_fixed`), integer
arithmetic again.  `rotation_coefficients` makes its six 16.16 integers as Pillow does, `rotate_nearest_u8` (csrc/rotate.hip)
gives Pillow's pixels and the mask (tests/test_rotate_cpu.py, tests/test_robotcar_ingest_gpu.py against
tests/golden/rotate_pillow.npz), and photometric.apply(geometry=) gathers through the same integers."""
import math

import numpy as np
import torch

from . import _lib
from ._tensor import ptr
from .datastep import IMNET_MEAN, IMNET_STD

PRECISION_BITS = 32 - 8 - 2      # Resample.c: 8 bits of pixel, 2 spare bits for the accumulation


# ------------------------------------------------------------------ host tables
def _bilinear_filter(x):
    return max(1.0 - abs(x), 0.0)


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos_filter(x):
    """Resample.c `lanczos_filter`: the truncated sinc, a = 3, on the HALF-OPEN interval [-3, 3)"""
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"bilinear": (_bilinear_filter, 1.0), "lanczos": (_lanczos_filter, 3.0)}     # name -> (kernel, support)
FILTER_CODE = {"bilinear": 0, "lanczos": 1}                                            # the C ABI's `filter` argument


def check_accumulator(coef):
    """every row of a coefficient table must keep a pass inside int32: 255 * sum |coef| + 2^21 < 2^31.  Automatic for a
    non-negative filter (the row sums to 2^22); with Lanczos' negative lobes it is a condition, checked when a table is built."""
    worst = int(np.abs(np.asarray(coef, dtype=np.int64)).sum(-1).max()) if np.size(coef) else 0
    if 255 * worst + (1 << (PRECISION_BITS - 1)) >= 1 << 31:
        raise ValueError(f"resample tables: a row with sum |coef| = {worst} overflows the int32 accumulator "
                         f"(255 * sum |coef| + 2^{PRECISION_BITS - 1} must stay below 2^31)")


def _tables(in_size, out_size, kernel, filter_support, who):
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"{who}: sizes must be positive")
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = filter_support * filterscale
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
        w = [kernel((x + lo - center + 0.5) * ss) for x in range(cnt)]
        ww = 0.0
        for v in w:                                                    # left to right, in double
            ww += v
        for x in range(cnt):
            k = w[x] / ww if ww != 0.0 else w[x]
            coef[xx, x] = int(-0.5 + k * one) if k < 0 else int(0.5 + k * one)   # half away from zero
        xmin[xx], n[xx] = lo, cnt
    check_accumulator(coef)
    return xmin, n, coef


def bilinear_tables(in_size, out_size):
    """Pillow's `precompute_coeffs` (bilinear: support 1) + `normalize_coeffs_8bpc` for one axis ->
    (xmin[out] int32, n[out] int32, coef[out, kmax] int32): output pixel xx = (sum_k in[xmin[xx] + k] * coef[xx, k] + 2^21) >> 22
    over k < n[xx]; coef beyond n is 0.  kmax = ceil(support) * 2 + 1 with support = max(in / out, 1)."""
    return _tables(in_size, out_size, _bilinear_filter, 1.0, "bilinear_tables")


def filter_tables(in_size, out_size, filter="bilinear"):
    """bilinear_tables for any filter of FILTERS: "bilinear" (exactly bilinear_tables) or "lanczos" (Pillow's LANCZOS:
    sinc(x) sinc(x / 3) on [-3, 3), support 3, negative taps).  kmax = ceil(support * max(in / out, 1)) * 2 + 1.  Raises
    ValueError when a row could overflow the int32 accumulation of a pass (check_accumulator)."""
    if filter not in FILTERS:
        raise ValueError(f"filter_tables: filter {filter!r} (one of {sorted(FILTERS)})")
    kernel, support = FILTERS[filter]
    return _tables(in_size, out_size, kernel, support, "filter_tables")


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


ROTATE_MAX_SIDE = 32767          # Geometry.c: the fixed-point path is taken below 32768 pixels a side


def rotation_coefficients(angle, H, W):
    """(a0, a1, a2, a3, a4, a5): the 16.16 fixed-point coefficients with which `Image.rotate(angle, NEAREST, expand=False,
    center=None)` of an (H, W) image reads its source -- Image.rotate's matrix (entries rounded to 15 decimals, the centre
    (W / 2, H / 2)) in Python floats, then affine_fixed's FIX(v) = floor(v * 65536 + 0.5) with the half-pixel offset folded into
    a2 / a5.  Output pixel (y, x) reads source (yy >> 16, xx >> 16), xx = a2 + a1 y + a0 x, yy = a5 + a4 y + a3 x.
    ValueError for a multiple of 90 degrees other than 0 (Pillow transposes there instead) and for a size at which |xx| or |yy|
    could pass 2^31."""
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H > ROTATE_MAX_SIDE or W > ROTATE_MAX_SIDE:
        raise ValueError(f"rotation_coefficients: a {H} x {W} image (each side 1 ... {ROTATE_MAX_SIDE}: Pillow's limit for its "
                         f"fixed-point transform)")
    ang = float(angle) % 360.0
    if ang in (90.0, 180.0, 270.0):
        raise ValueError(f"rotation_coefficients: angle {angle!r}: Pillow rotates by a multiple of 90 degrees with a transpose, "
                         f"which is not built")
    r = -math.radians(ang)
    cx, cy = W / 2, H / 2
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    m[2] = m[0] * (-cx) + m[1] * (-cy) + m[2] + cx
    m[5] = m[3] * (-cx) + m[4] * (-cy) + m[5] + cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))  # noqa: E731
    a = (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))
    for a_c, a_y, a_x in ((a[2], a[1], a[0]), (a[5], a[4], a[3])):
        if abs(a_c) + abs(a_y) * (H - 1) + abs(a_x) * (W - 1) >= 1 << 31:
            raise ValueError(f"rotation_coefficients: at {H} x {W} the fixed-point coordinates could pass 2^31")
    return a


# ------------------------------------------------------------------ numpy restatements (tests, documentation)
def _pass_reference(img, axis, out_size, filter="bilinear"):
    """one 8-bit pass along `axis` of an (H, W, C) uint8 array: uint8 out, rounded and clipped as Pillow does between the passes"""
    xmin, n, coef = filter_tables(img.shape[axis], out_size, filter)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.int64)
    for xx in range(out_size):
        k = coef[xx, :n[xx]].astype(np.int64).reshape((-1,) + (1,) * (src.ndim - 1))
        out[xx] = ((src[xmin[xx]:xmin[xx] + n[xx]] * k).sum(0) + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize_reference(img_hwc_u8, size, filter="bilinear"):
    """`Image.fromarray(img).resize((w, h), BILINEAR)` (or LANCZOS: filter="lanczos") of an (H, W, C) uint8 array -> (h, w, C)
    uint8: the horizontal pass to a uint8 intermediate, then the vertical one; a pass is skipped when its axis keeps its size.
    With Lanczos the sums overshoot [0, 255] near edges of the image content: the clip of each pass is part of the result."""
    img = np.ascontiguousarray(img_hwc_u8)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError("resize_reference: an (H, W, C) uint8 array is required")
    h, w = int(size[0]), int(size[1])
    if img.shape[1] != w:
        img = _pass_reference(img, 1, w, filter)
    if img.shape[0] != h:
        img = _pass_reference(img, 0, h, filter)
    return np.ascontiguousarray(img)


def lanczos_reference(img_hwc_u8, size):
    """`Image.fromarray(img).resize((w, h), LANCZOS)` -> (h, w, C) uint8"""
    return resize_reference(img_hwc_u8, size, "lanczos")


def pad_bottom_right_reference(chw, size, fill=0.0):
    """transforms.PadBottomRight.pad of a (C, h, w) array to (C, size[0], size[1])"""
    out = np.full((chw.shape[0], int(size[0]), int(size[1])), fill, dtype=chw.dtype)
    out[:, :chw.shape[1], :chw.shape[2]] = chw
    return out


def scale_points(pts, h, w, new_h, new_w):
    """what a resize of an (h, w) image to (new_h, new_w) does to its (n, 2) fp32 (x, y) points, as the readers
    (datasets/megadepth.py:378-395) and transforms.Resize (transforms.py:163-198) do it: the factor is formed in double and
    multiplies the fp32 coordinates as an fp32 number.  -> a new host tensor"""
    pts = torch.as_tensor(pts).detach().cpu().to(torch.float32).clone()
    x_scale, y_scale = new_w / float(w), new_h / float(h)
    pts[:, 0] = x_scale * pts[:, 0]
    pts[:, 1] = y_scale * pts[:, 1]
    return pts


def _check_lut_host(lut, who):
    lut = np.asarray(lut)
    if lut.dtype != np.uint8 or lut.shape != (256,):
        raise ValueError(f"{who}: lut must be a 256-element uint8 table")
    return lut


def resize_nearest_reference(lbl_u8, size, lut=None):
    """`Image.fromarray(lbl).resize((w, h), NEAREST)` of an (H, W) uint8 array -> (h, w) uint8.  lut (256 uint8 codes): the map is
    encoded first, lut[lbl], as a reader with raw label ids does in front of its resize (RobotCar.encode_semantic_map)"""
    lbl = np.asarray(lbl_u8)
    if lbl.dtype != np.uint8 or lbl.ndim != 2:
        raise ValueError("resize_nearest_reference: an (H, W) uint8 array is required")
    if lut is not None:
        lbl = _check_lut_host(lut, "resize_nearest_reference")[lbl]
    h, w = int(size[0]), int(size[1])
    if lbl.shape == (h, w):
        return lbl.copy()
    return np.ascontiguousarray(lbl[nearest_table(lbl.shape[0], h)][:, nearest_table(lbl.shape[1], w)])


# ------------------------------------------------------------------ device tables
_TABLES = {}


def _device_tables(kind, in_size, out_size, device):
    """cached per (kind, in, out, device).  bilinear / lanczos: (bounds int32 [out, 2] = (xmin, n), coef int32 [out, kmax], kmax);
    nearest: int32 [out]"""
    key = (kind, int(in_size), int(out_size), device)
    t = _TABLES.get(key)
    if t is None:
        if kind in FILTERS:
            xmin, n, coef = filter_tables(in_size, out_size, kind)
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
def _filter(filter, who):
    if filter not in FILTERS:
        raise ValueError(f"{who}: filter {filter!r} (one of {sorted(FILTERS)})")
    return filter


def resize_u8(image_hwc_u8, size, filter="bilinear"):
    """Pillow's bilinear (or, filter="lanczos", LANCZOS) resize of a decoded (H, W, 3) uint8 DEVICE image -> (3, h, w) uint8
    (what ToTensor would leave)"""
    _check_image(image_hwc_u8, "resize_u8")
    _filter(filter, "resize_u8")
    H, W, _ = image_hwc_u8.shape
    Hd, Wd = int(size[0]), int(size[1])
    dev = image_hwc_u8.device
    bx, cx, kx = _device_tables(filter, W, Wd, dev)
    by, cy, ky = _device_tables(filter, H, Hd, dev)
    out = torch.empty((3, Hd, Wd), dtype=torch.uint8, device=dev)
    if filter == "bilinear":
        _lib.call("rfn_resize_u8", dev, ptr(image_hwc_u8), H, W, Hd, Wd, ptr(bx), ptr(cx), kx, ptr(by), ptr(cy), ky, ptr(out))
    else:
        _lib.call("rfn_resize_filter_u8", dev, ptr(image_hwc_u8), H, W, Hd, Wd, FILTER_CODE[filter], ptr(bx), ptr(cx), kx, ptr(by),
                  ptr(cy), ky, ptr(out))
    return out


def resize_nearest_u8(label_u8, size, lut=None):
    """Pillow's NEAREST resize of an (H, W) uint8 DEVICE label map -> (h, w) uint8.  lut: a contiguous 256-element uint8 DEVICE
    tensor; the output is lut[label] resized -- encode and resize in one launch, the encoded map at the input's size is never
    stored; size == the input's size is the encode alone.  lut=None launches the plain gather."""
    if not label_u8.is_cuda:
        raise RuntimeError("resize_nearest_u8: device tensors required (the product path has no CPU fallback)")
    if not (label_u8.dtype == torch.uint8 and label_u8.dim() == 2 and label_u8.is_contiguous()):
        raise RuntimeError("resize_nearest_u8: label must be a contiguous (H, W) uint8 tensor")
    H, W = label_u8.shape
    Hd, Wd = int(size[0]), int(size[1])
    dev = label_u8.device
    if lut is not None and not (torch.is_tensor(lut) and lut.dtype == torch.uint8 and tuple(lut.shape) == (256,) and
                                lut.is_contiguous() and lut.device == dev):
        raise RuntimeError("resize_nearest_u8: lut must be a contiguous 256-element uint8 tensor on the label's device")
    ty, tx = _device_tables("nearest", H, Hd, dev), _device_tables("nearest", W, Wd, dev)
    out = torch.empty((Hd, Wd), dtype=torch.uint8, device=dev)
    if lut is None:
        _lib.call("rfn_resize_nearest_u8", dev, ptr(label_u8), H, W, Hd, Wd, ptr(ty), ptr(tx), ptr(out))
    else:
        _lib.call("rfn_resize_nearest_lut_u8", dev, ptr(label_u8), H, W, Hd, Wd, ptr(ty), ptr(tx), ptr(lut), ptr(out))
    return out


def device_lut(lut, device):
    """a 256-entry uint8 code table (numpy / tensor) as the contiguous device tensor resize_nearest_u8(lut=) takes"""
    t = torch.as_tensor(np.ascontiguousarray(_check_lut_host(lut.cpu().numpy() if torch.is_tensor(lut) else lut, "device_lut")))
    return t.to(device).contiguous()


def rotate_nearest_u8(image_u8, angle, fill=0):
    """`PIL.Image.rotate(angle, NEAREST, expand=False, center=None, fillcolor=fill)` of a (3, H, W) or (H, W) uint8 DEVICE
    tensor -> (rotated, outside): the same shape, and an (H, W) bool mask that is True where the source falls outside the image
    (there the pixel is `fill`, in every channel) -- what RandomRotation makes of an image (fill 0), a label map (fill 255) and its
    normalize_mask.  angle % 360 == 0 is a copy with an all-False mask; 90, 180 and 270 raise ValueError."""
    if not (torch.is_tensor(image_u8) and image_u8.is_cuda):
        raise RuntimeError("rotate_nearest_u8: device tensors required (the product path has no CPU fallback)")
    if not (image_u8.dtype == torch.uint8 and image_u8.dim() in (2, 3) and image_u8.is_contiguous() and
            (image_u8.dim() == 2 or image_u8.shape[0] == 3)):
        raise RuntimeError("rotate_nearest_u8: a contiguous (3, H, W) or (H, W) uint8 tensor is required")
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError(f"rotate_nearest_u8: fill {fill} (0 ... 255)")
    H, W = image_u8.shape[-2:]
    a = rotation_coefficients(angle, H, W)
    dev = image_u8.device
    out = torch.empty_like(image_u8)
    outside = torch.empty((H, W), dtype=torch.bool, device=dev)
    _lib.call("rfn_rotate_nearest_u8", dev, ptr(image_u8), 1 if image_u8.dim() == 2 else 3, H, W, *a, fill, ptr(out), ptr(outside))
    return out, outside


def resize_crop_flip_normalize(image_hwc_u8, dims, top, left, h, w, flip, out_image=None, mean=IMNET_MEAN, std=IMNET_STD,
                               filter="bilinear", pad_to=None):
    """load-time resize to `dims` = (Hd, Wd) + crop (top, left, h, w) of the RESIZED image + RandomHorizontalFlip +
    ConvertImageDtype + Normalize of a decoded (H, W, 3) uint8 DEVICE image in one kernel, written into `out_image` (3, h, w)
    fp32 (a slot of a batch tensor) or a fresh tensor: bit for bit datastep.crop_flip_normalize of Pillow's resized image.
    filter: "bilinear" or "lanczos".  pad_to = (Hf, Wf) >= (h, w): the output is (3, Hf, Wf), the crop at its top left and 0.0
    everywhere else -- transforms.PadBottomRight after Normalize -- written by the same launch."""
    _check_image(image_hwc_u8, "resize_crop_flip_normalize")
    _filter(filter, "resize_crop_flip_normalize")
    H, W, _ = image_hwc_u8.shape
    Hd, Wd = int(dims[0]), int(dims[1])
    dev = image_hwc_u8.device
    Hf, Wf = (int(h), int(w)) if pad_to is None else (int(pad_to[0]), int(pad_to[1]))
    if out_image is None:
        out_image = torch.empty((3, Hf, Wf), dtype=torch.float32, device=dev)
    if not (out_image.dtype == torch.float32 and tuple(out_image.shape) == (3, Hf, Wf) and out_image.is_contiguous()):
        raise RuntimeError("resize_crop_flip_normalize: out_image must be a contiguous (3, h, w) float32 tensor (h, w: pad_to "
                           "when given)")
    bx, cx, kx = _device_tables(filter, W, Wd, dev)
    by, cy, ky = _device_tables(filter, H, Hd, dev)
    m = np.asarray(mean, dtype=np.float32).copy()
    s = np.asarray(std, dtype=np.float32).copy()
    if filter == "bilinear" and pad_to is None:
        _lib.call("rfn_resize_crop_flip_norm_u8", dev, ptr(image_hwc_u8), H, W, Hd, Wd, ptr(bx), ptr(cx), kx, ptr(by), ptr(cy), ky,
                  int(top), int(left), int(h), int(w), 1 if flip else 0, m.ctypes.data, s.ctypes.data, ptr(out_image))
    else:
        _lib.call("rfn_resize_filter_crop_flip_norm_pad_u8", dev, ptr(image_hwc_u8), H, W, Hd, Wd, FILTER_CODE[filter], ptr(bx),
                  ptr(cx), kx, ptr(by), ptr(cy), ky, int(top), int(left), int(h), int(w), 1 if flip else 0, m.ctypes.data,
                  s.ctypes.data, ptr(out_image), Hf, Wf)
    return out_image


class EvalIngest:
    """The val / test / predict pipelines of the reference's configs from decoded files to the tensors Trainer.validate / test /
    predict take: load-time `dims` (image `dims_interpolation`, label nearest), an optional transforms.Resize (`resize`: int or
    (h, w) with `interpolation`; `img_only`: the label and the points keep their size, as in refign_*.yaml `test:`),
    ConvertImageDtype, Normalize, an optional transforms.PadBottomRight (`pad`: "same" = `image` and `image_ref` both at
    (max h, max w), or a fixed (h, w); the fill is 0 AFTER the normalisation).  Two successive resizes are two Pillow resizes with
    a uint8 image in between (they are NOT merged: the intermediate rounding is part of the result); the last one is fused with
    the conversion and the padding (a whole-image crop, no flip).  The filters are "bilinear" (the segmentation data sets) or
    "lanczos" (the matcher's: MegaDepth / RobotCarMatching readers and `test:` sections).
    label_lut: a 256-entry uint8 table the label map's codes go through (RobotCar's raw ids -> train ids), fused into the label's
    first NEAREST resize, or one launch at the file's size when there is none.
    __call__(image, semantic=None, image_ref=None, corr_pts=None, corr_pts_ref=None) -> {"image" (1, 3, h, w) fp32
    [, "image_ref"][, "semantic" (1, h', w') int64][, "corr_pts" / "corr_pts_ref": [(n, 2) fp32]]}; images are (H, W, 3) uint8,
    the label (H, W) uint8, host arrays / tensors (uploaded) or device tensors.  The points are (n, 2) fp32 (x, y) of `image`
    (corr_pts) and of `image_ref` (corr_pts_ref): every resize step scales them by its own image's size change, on the host in
    fp32 as the reference does (scale_points); padding and normalisation leave them alone; they are uploaded afterwards and come
    back as one-element lists, the way the reference's my_collate batches them."""

    def __init__(self, dims=None, resize=None, img_only=False, mean=IMNET_MEAN, std=IMNET_STD, only_if_larger=False, device=None,
                 interpolation="bilinear", dims_interpolation="bilinear", pad=None, label_lut=None):
        self.label_lut = label_lut                                  # 256 uint8 codes (host or device): see label()
        self._lut_dev = {}
        self.device = torch.device(device) if device is not None else None      # None: the input's device, else the current one
        self.dims = None if dims is None else (int(dims[0]), int(dims[1]))
        self.resize, self.img_only, self.only_if_larger = resize, bool(img_only), bool(only_if_larger)
        self.mean, self.std = mean, std
        self.interpolation = _filter(interpolation, "EvalIngest(interpolation=)")
        self.dims_interpolation = _filter(dims_interpolation, "EvalIngest(dims_interpolation=)")
        if not (pad is None or pad == "same" or (isinstance(pad, (tuple, list)) and len(pad) == 2)):
            raise ValueError(f"EvalIngest: pad must be None, 'same' or (h, w), got {pad!r}")
        self.pad = pad if pad is None or pad == "same" else (int(pad[0]), int(pad[1]))

    def _steps(self, h, w):
        """the chain of (size, filter, is the Resize) an (h, w) input runs through (identity steps dropped)"""
        chain = []
        for step, filt in ((self.dims, self.dims_interpolation), (self.resize, self.interpolation)):
            if step is None:
                continue
            nh, nw = target_size(h, w, step, self.only_if_larger) if step is self.resize else step
            if (nh, nw) != (h, w):
                chain.append(((nh, nw), filt, step is self.resize))
                h, w = nh, nw
        return chain

    def _sizes(self, h, w):
        """the chain of sizes an (h, w) input runs through (identity steps dropped)"""
        return [size for size, _, _ in self._steps(h, w)]

    def _upload(self, x):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.is_cuda:
            return x
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError("EvalIngest: a HIP device is required (the product path has no CPU fallback)")
        return x.to(dev, non_blocking=True)

    def image(self, image_hwc_u8, pad_to=None):
        x = self._upload(image_hwc_u8)
        _check_image(x, "EvalIngest")
        chain = self._steps(x.shape[0], x.shape[1])
        for size, filt, _ in chain[:-1]:                                # Pillow's uint8 image in between, channels last again
            x = resize_u8(x, size, filt).permute(1, 2, 0).contiguous()
        (h, w), filt = chain[-1][:2] if chain else ((x.shape[0], x.shape[1]), "bilinear")
        return resize_crop_flip_normalize(x, (h, w), 0, 0, h, w, False, None, self.mean, self.std, filt, pad_to).unsqueeze(0)

    def _lut(self, device):
        if self.label_lut is None:
            return None
        if device not in self._lut_dev:
            self._lut_dev[device] = device_lut(self.label_lut, device)
        return self._lut_dev[device]

    def label(self, label_u8):
        """label_lut: the file's codes are encoded (lut[label]) by the first resize's launch, as the reader does in front of its
        load-time resize; with no resize to do it is one launch of its own at the file's size"""
        y = self._upload(label_u8)
        lut = self._lut(y.device)
        steps = (self.dims,) if self.img_only else (self.dims, self.resize)
        for step in steps:
            if step is None:
                continue
            size = target_size(y.shape[0], y.shape[1], step, self.only_if_larger) if step is self.resize else step
            if tuple(size) != tuple(y.shape):
                y, lut = resize_nearest_u8(y, size, lut), None
        if lut is not None:
            y = resize_nearest_u8(y, tuple(y.shape), lut)
        return y.to(torch.int64).unsqueeze(0)

    def points(self, pts, h, w):
        """(n, 2) fp32 (x, y) points of a decoded (h, w) image through that image's resize steps -> a HOST fp32 tensor"""
        pts = torch.as_tensor(pts).detach().cpu().to(torch.float32).clone()
        if pts.dim() != 2 or pts.shape[1] != 2:
            raise ValueError(f"EvalIngest: points must be (n, 2) (x, y), got {tuple(pts.shape)}")
        for (nh, nw), _, is_resize in self._steps(h, w):
            if not (is_resize and self.img_only):
                pts = scale_points(pts, h, w, nh, nw)
            h, w = nh, nw
        return pts

    def final_size(self, h, w):
        chain = self._sizes(h, w)
        return chain[-1] if chain else (int(h), int(w))

    def __call__(self, image, semantic=None, image_ref=None, corr_pts=None, corr_pts_ref=None):
        if corr_pts_ref is not None and image_ref is None:
            raise ValueError("EvalIngest: corr_pts_ref are points of image_ref, which is missing")
        pad_to = self.pad
        if pad_to == "same":
            sizes = [self.final_size(*x.shape[:2]) for x in (image, image_ref) if x is not None]
            pad_to = (max(s[0] for s in sizes), max(s[1] for s in sizes))
        out = {"image": self.image(image, pad_to)}
        if image_ref is not None:
            out["image_ref"] = self.image(image_ref, pad_to)
        if semantic is not None:
            if pad_to is not None:
                raise NotImplementedError("EvalIngest: PadBottomRight of a label map is not built (no config of the reference pads one)")
            out["semantic"] = self.label(semantic)
        for key, pts, img in (("corr_pts", corr_pts, image), ("corr_pts_ref", corr_pts_ref, image_ref)):
            if pts is not None:
                out[key] = [self._upload(self.points(pts, img.shape[0], img.shape[1]))]
        return out

"""The matcher's warp supervision on the device (csrc/flowsynth.hip): data_modules/transforms.py's CompositeFlow -- a random
homography, affine, thin-plate-spline or affine-TPS flow, optionally composed with an elastic perturbation -- the warp of
`image_prime` by that flow, the validity mask and CenterCrop.  In the reference this runs per sample in the data-loader workers
on the CPU: several full-frame grid_sample calls, a TPS over every pixel and two Gaussian blurs of 600 to 1080 taps.

Host side (this file): the DRAWS, where the reference makes them and in its order, and the small linear algebra in the
reference's own order -- the 8 x 8 inverse of the homography, Li of the 3 x 3 control grid, W_X / W_Y / A_X / A_Y, the 2 x 3
affine matrix.  Draw order of one sample (both streams stand afterwards where the reference leaves them):
    random.choice over the transforms
    the transform's torch.rand draws from torch's global CPU generator: hom 8; affine 1 + 1 + 1 (rotation, shear, scale), then
        1 + 1 (tx, ty); tps 18; afftps the affine draws, then 18
    with add_elastic: random.randint (the number of bumps), random.random() twice (sigma, alpha), torch.rand(h, w) twice, and
        per bump random.randint three times (sigma, x, y)
Device side: every flow is analytic per pixel, so the kernels take 9 + 24 + 6 floats, a transform code and the bump list and
store nothing but the flow (one launch for the flow and the border count, one for the warp, the masks and the crop; two for a
blur).  Nothing here waits for the device: the mask fallback is decided there from an integer count.

The elastic field's blur is cv2.GaussianBlur(src, (0, 0), sigma) for a float32 image AS OPENCV DOCUMENTS IT (gaussian_blur_f32).
OpenCV is installed neither where this was written nor where it was tested: parity with cv2 itself is NOT verified."""
import ctypes
import math
import random

import numpy as np
import torch

from . import _lib
from ._tensor import ptr, upload_async, workspace

TRANSFORMS = ("hom", "affine", "tps", "afftps")            # the kernel's transform codes
MAX_BUMPS = 13
# RandomElastic's defaults (CompositeFlow builds it with nothing but apply_keys)
_ELASTIC = {"min_nbr_perturbations": 5, "max_nbr_perturbations": 13, "min_sigma_mask": 10, "max_sigma_mask": 40,
            "min_sigma": 0.1, "max_sigma": 0.08, "min_alpha": 1, "max_alpha": 1}
_HOM_ID = (-1, -1, 1, 1, -1, 1, -1, 1)
_TPS_ID = (-1, -1, -1, 0, 0, 0, 1, 1, 1, -1, 0, 1, -1, 0, 1, -1, 0, 1)


class FlowParams:
    """One sample's parameters.  kind: a name of TRANSFORMS; theta_hom (8,) / theta_aff (2, 3) / theta_tps (18,): fp32 CPU
    tensors or None; theta39: what the kernel takes; elastic: None or a dict -- sigma, alpha, n_perturbations, drawn (the
    (sigma, x, y) triples as drawn), bumps (the kept ones as (x, y, sigma, scale)), noise ((2, h, w) uniform draws, CPU) and / or
    field ((2, h, w), the blurred and scaled perturbation)."""

    def __init__(self, kind, h, w, theta_hom=None, theta_aff=None, theta_tps=None, elastic=None, transform_index=None):
        if kind not in TRANSFORMS:
            raise ValueError(f"flowsynth: unknown transform {kind!r} ({', '.join(TRANSFORMS)})")
        self.kind, self.h, self.w, self.transform_index = kind, int(h), int(w), transform_index
        self.theta_hom, self.theta_aff, self.theta_tps, self.elastic = theta_hom, theta_aff, theta_tps, elastic
        t39 = torch.zeros(39, dtype=torch.float32)
        if theta_hom is not None:
            t39[:9] = homography(theta_hom)
        if theta_tps is not None:
            t39[9:33] = tps_weights(theta_tps)
        if theta_aff is not None:
            t39[33:] = torch.as_tensor(theta_aff, dtype=torch.float32).reshape(6)
        self.theta39 = t39


def homography(theta):
    """h0 .. h8 from the four displaced corners (transforms.py:731-750): h33 = 1, the 8 x 8 system inverted."""
    theta = torch.as_tensor(theta, dtype=torch.float32).reshape(1, 8)
    xp, yp = theta[:, :4].unsqueeze(2), theta[:, 4:].unsqueeze(2)
    x = theta.new_tensor([-1, -1, 1, 1]).view(1, 4, 1)
    y = theta.new_tensor([-1, 1, -1, 1]).view(1, 4, 1)
    z, o = theta.new_zeros(1, 4, 1), theta.new_ones(1, 4, 1)
    A = torch.cat([torch.cat([-x, -y, -o, z, z, z, x * xp, y * xp, xp], 2),
                   torch.cat([z, z, z, -x, -y, -o, x * yp, y * yp, yp], 2)], 1)
    h = torch.bmm(torch.inverse(A[:, :, :8]), -A[:, :, 8].unsqueeze(2))
    return torch.cat([h, theta.new_ones(1, 1, 1)], 1).reshape(9)


_LI = None


def tps_li():
    """Li of the 3 x 3 control grid on [-1, 1]^2, reg_factor 0 (transforms.py:1013-1032); control point k = (axis[k // 3],
    axis[k % 3])."""
    global _LI
    if _LI is None:
        axis = np.linspace(-1, 1, 3)
        P_Y, P_X = np.meshgrid(axis, axis)
        X, Y = torch.FloatTensor(np.reshape(P_X, (-1, 1))), torch.FloatTensor(np.reshape(P_Y, (-1, 1)))
        N = 9
        Xm, Ym = X.expand(N, N), Y.expand(N, N)
        d2 = torch.pow(Xm - Xm.transpose(0, 1), 2) + torch.pow(Ym - Ym.transpose(0, 1), 2)
        d2[d2 == 0] = 1
        K = torch.mul(d2, torch.log(d2))
        P = torch.cat((torch.ones(N, 1), X, Y), 1)
        L = torch.cat((torch.cat((K, P), 1), torch.cat((P.transpose(0, 1), torch.zeros(3, 3)), 1)), 0)
        _LI = torch.inverse(L).unsqueeze(0)
    return _LI


def tps_weights(theta):
    """W_X (9), W_Y (9), A_X (3), A_Y (3) of the displaced control points (transforms.py:903-914)."""
    theta = torch.as_tensor(theta, dtype=torch.float32).reshape(1, 18, 1)
    Li, N = tps_li(), 9
    Q_X, Q_Y = theta[:, :N], theta[:, N:]
    W_X, W_Y = torch.bmm(Li[:, :N, :N], Q_X), torch.bmm(Li[:, :N, :N], Q_Y)
    A_X, A_Y = torch.bmm(Li[:, N:, :N], Q_X), torch.bmm(Li[:, N:, :N], Q_Y)
    return torch.cat([W_X.reshape(9), W_Y.reshape(9), A_X.reshape(3), A_Y.reshape(3)])


def _draw_affine(random_alpha, random_s, random_tx, random_ty):
    """RandomAffine.get_params (transforms.py:617-640), preserve_aspect_ratio=True as CompositeFlow leaves it"""
    rot_angle = (torch.rand(1).item() - 0.5) * 2 * random_alpha
    sh_angle = (torch.rand(1).item() - 0.5) * 2 * random_alpha
    lambda_1 = 1 + (2 * torch.rand(1).item() - 1) * random_s
    tx = (2 * torch.rand(1) - 1) * random_tx
    ty = (2 * torch.rand(1) - 1) * random_ty
    R_sh = torch.tensor([[math.cos(sh_angle), -math.sin(sh_angle)], [math.sin(sh_angle), math.cos(sh_angle)]])
    R_alpha = torch.tensor([[math.cos(rot_angle), -math.sin(rot_angle)], [math.sin(rot_angle), math.cos(rot_angle)]])
    D = torch.diag(torch.tensor([lambda_1, lambda_1]))
    A = R_alpha @ R_sh.T @ D @ R_sh
    return torch.stack([A[0, 0], A[0, 1], tx[0], A[1, 0], A[1, 1], ty[0]]).view(2, 3)


def bump_scale(h, w, x, y, sigma):
    """2 / mask.max() of one Gaussian bump as RandomElastic.get_params forms it (transforms.py:1241-1266), or None where the
    reference skips the bump (max < 1e-6).  The quirk is kept: gkern applies `x` to axis 0 (length h) and `y` to axis 1,
    although x was drawn against the width.  The maximum of the outer product of two positive vectors is the product of their
    maxima, rounded once: the (h, w) mask is not formed."""
    sig2 = 2 * sigma * sigma
    g1 = torch.exp(-(torch.arange(0, h) - x) ** 2 / sig2)
    g2 = torch.exp(-(torch.arange(0, w) - y) ** 2 / sig2)
    m = (g1.max() * g2.max()) / (sigma * math.sqrt(2 * math.pi) ** 2)
    if m < 1e-6:
        return None
    return float(2.0 / m)


def _draw_elastic(h, w):
    """RandomElastic.get_params' draws (transforms.py:1227-1259) with the class defaults"""
    e = _ELASTIC
    n = random.randint(e["min_nbr_perturbations"], e["max_nbr_perturbations"])
    sigma = max(h, w) * (e["min_sigma"] + e["max_sigma"] * random.random())
    alpha = max(h, w) * (e["min_alpha"] + e["max_alpha"] * random.random())
    noise = torch.stack([torch.rand(h, w, dtype=torch.float), torch.rand(h, w, dtype=torch.float)])
    drawn, bumps = [], []
    for _ in range(n):
        s = random.randint(e["min_sigma_mask"], e["max_sigma_mask"])
        x = random.randint(0 + s * 3, w - s * 3)
        y = random.randint(0 + s * 3, h - s * 3)
        drawn.append((s, x, y))
        scale = bump_scale(h, w, x, y, s)
        if scale is not None:
            bumps.append((float(x), float(y), float(s), scale))
    return {"sigma": sigma, "alpha": alpha, "n_perturbations": n, "drawn": drawn, "bumps": bumps, "noise": noise, "field": None}


def draw_composite(h, w, include_transforms=("hom", "affine"), random_alpha=0.065, random_s=0.6, random_tx=0.3, random_ty=0.1,
                   random_t_hom=0.3, random_t_tps=0, random_t_tps_for_afftps=0, add_elastic=False,
                   parameterize_with_gaussian=False):
    """One sample's FlowParams, drawn as CompositeFlow.forward draws them (the order: this module's docstring).  The defaults
    are CompositeFlow's."""
    if parameterize_with_gaussian:
        raise ValueError("flowsynth.draw_composite: parameterize_with_gaussian=True is not carried (no reference config sets it)")
    include_transforms = list(include_transforms)
    for t in include_transforms:
        if t not in TRANSFORMS:
            raise ValueError(f"flowsynth.draw_composite: unknown transform {t!r} ({', '.join(TRANSFORMS)})")
    kind = random.choice(include_transforms)
    hom = aff = tps = None
    if kind == "hom":
        hom = torch.tensor(_HOM_ID, dtype=torch.float) + (torch.rand(8) - 0.5) * 2 * random_t_hom
    elif kind == "affine":
        aff = _draw_affine(random_alpha, random_s, random_tx, random_ty)
    elif kind == "tps":
        tps = torch.tensor(_TPS_ID, dtype=torch.float) + (torch.rand(18) - 0.5) * 2 * random_t_tps
    else:
        aff = _draw_affine(random_alpha, random_s, random_tx, random_ty)
        tps = torch.tensor(_TPS_ID, dtype=torch.float) + (torch.rand(18) - 0.5) * 2 * random_t_tps_for_afftps
    elastic = _draw_elastic(h, w) if add_elastic else None
    return FlowParams(kind, h, w, hom, aff, tps, elastic, transform_index=include_transforms.index(kind))


def params_from(kind, h, w, theta_hom=None, theta_aff=None, theta_tps=None, field=None, bumps=(), theta39=None):
    """FlowParams from explicit values, bypassing the draws: theta_hom (8) the displaced corners, theta_aff the 2 x 3 matrix of
    affine_grid, theta_tps (18) the displaced control points -- or theta39, the kernel's 39 floats as they stand (h0 .. h8, W_X,
    W_Y, A_X, A_Y, the affine matrix); field a ready (2, h, w) perturbation (dx, dy) in pixels with `bumps` [(x, y, sigma,
    scale), ...] (scale: bump_scale), at most MAX_BUMPS."""
    need = {"hom": (theta_hom,), "affine": (theta_aff,), "tps": (theta_tps,), "afftps": (theta_aff, theta_tps)}.get(kind, ())
    if theta39 is None and any(v is None for v in need):
        raise ValueError(f"flowsynth.params_from: {kind!r} needs its theta")
    elastic = None
    if field is not None:
        field = torch.as_tensor(field, dtype=torch.float32)
        if tuple(field.shape) != (2, h, w):
            raise ValueError(f"flowsynth.params_from: field {tuple(field.shape)}, (2, {h}, {w}) expected")
        elastic = {"sigma": None, "alpha": None, "n_perturbations": len(bumps), "drawn": None,
                   "bumps": [tuple(float(v) for v in b) for b in bumps], "noise": None, "field": field}
    cpu = lambda v: None if v is None else torch.as_tensor(v, dtype=torch.float32).cpu()  # noqa: E731
    p = FlowParams(kind, h, w, cpu(theta_hom), cpu(theta_aff), cpu(theta_tps), elastic)
    if theta39 is not None:
        p.theta39 = torch.as_tensor(theta39, dtype=torch.float32).reshape(39).cpu().clone()
    return p


def gaussian_taps(sigma):
    """cv2.getGaussianKernel(ksize, sigma, CV_32F) for the ksize GaussianBlur derives from sigma for a float image, as OpenCV
    documents both: round(sigma * 8 + 1) | 1 taps, exp(-x^2 / 2 sigma^2) in double, normalised to sum 1, stored as float32."""
    n = int(round(float(sigma) * 8 + 1)) | 1
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2
    k = np.exp(-(x * x) / (2.0 * float(sigma) * float(sigma)))
    return (k / k.sum()).astype(np.float32)


def gaussian_blur_f32(field, sigma):
    """cv2.GaussianBlur(src, (0, 0), sigma) of a float32 (h, w) or (planes, h, w) device tensor, as OpenCV documents it:
    gaussian_taps(sigma), separable, BORDER_REFLECT_101 (applied as often as needed when the radius exceeds the side),
    accumulated in fp64 through both passes and rounded once -- a thousand fp32 taps and the factor alpha (up to 2 max(h, w))
    afterwards would leave thousandths of a pixel in the flow.  Parity with cv2 itself is NOT verified: OpenCV is not installed
    where this is built and tested (cv2's own float path accumulates in fp32 with SIMD-dependent order)."""
    if not (torch.is_tensor(field) and field.is_cuda and field.dtype == torch.float32 and field.dim() in (2, 3)):
        raise RuntimeError("gaussian_blur_f32: field must be a (h, w) or (planes, h, w) float32 HIP (cuda:N) tensor: "
                           "refign_amd has no CPU path")
    src = field.contiguous()
    h, w = src.shape[-2:]
    planes = 1 if src.dim() == 2 else src.shape[0]
    taps = gaussian_taps(sigma)
    dev = src.device
    taps_d = upload_async(taps, torch.float32, dev)
    tmp = torch.empty(planes * h * w, dtype=torch.float64, device=dev)
    out = torch.empty_like(src)
    _lib.call("rfn_gaussian_blur_f32", dev, ptr(src), ptr(taps_d), int(taps.size), planes, h, w, ptr(tmp), ptr(out))
    return out


def crop_origin(h, w, ch, cw):
    """torchvision's center_crop: Python's rounding (half to even), so a difference of 45 gives 22"""
    return int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))


def elastic_field(p, device):
    """the sample's perturbation (2, h, w) on `device`: the ready field, or elastic_transform's recipe (transforms.py:93-104)
    from the drawn noise -- 2 u - 1, blurred, times alpha, each in fp32"""
    e = p.elastic
    if e["field"] is not None:
        f = e["field"]
        return f.to(device, non_blocking=True) if f.device != device else f
    noise = upload_async(e["noise"], torch.float32, device)
    return gaussian_blur_f32(noise * 2 - 1, e["sigma"]) * e["alpha"]


def synthesize(image_prime, params, crop=None, min_fraction_valid_corr=0.1, return_count=False):
    """What CompositeFlow.forward followed by CenterCrop leaves in the sample.  image_prime: the normalised fp32 (B, 3, h, w)
    batch on the device, or one (3, h, w) image; params: B FlowParams (or one); crop: (ch, cw) or None (the full frame).
    -> image_prime (B, 3, ch, cw) fp32, image_prime_flow (B, 2, ch, cw) fp32, image_prime_mask (B, ch, cw) bool: the flow, the
    image warped by helpers.matching_utils.warp(padding_mode='zeros'), and the warp mask -- or create_border_mask(flow) where
    that covers less than min_fraction_valid_corr of the FULL frame.  return_count: also the (B,) int32 counts of
    create_border_mask over the full frame, on the device.  No host synchronisation.
    (One departure: a flow that is zero at EVERY pixel makes the reference's warp return the image with an all-true mask; here
    the pixels of the first row and column then fail the strict `> -1`.)"""
    if not (torch.is_tensor(image_prime) and image_prime.is_cuda and image_prime.dtype == torch.float32 and
            image_prime.dim() in (3, 4) and image_prime.shape[-3] == 3):
        raise RuntimeError("flowsynth.synthesize: image_prime must be a (B, 3, h, w) or (3, h, w) float32 HIP (cuda:N) tensor: "
                           "refign_amd has no CPU path")
    img = (image_prime if image_prime.dim() == 4 else image_prime.unsqueeze(0)).contiguous()
    params = [params] if isinstance(params, FlowParams) else list(params)
    B, _, h, w = img.shape
    if len(params) != B or any(p.h != h or p.w != w for p in params):
        raise RuntimeError(f"flowsynth.synthesize: {B} samples of {h} x {w} need as many parameter sets of that frame")
    ch, cw = (h, w) if crop is None else (int(crop[0]), int(crop[1]))
    if ch > h or cw > w or ch < 1 or cw < 1:
        raise RuntimeError(f"flowsynth.synthesize: crop {ch} x {cw} of a {h} x {w} frame")
    top, left = crop_origin(h, w, ch, cw)
    dev = img.device
    out_img = torch.empty((B, 3, ch, cw), dtype=torch.float32, device=dev)
    out_flow = torch.empty((B, 2, ch, cw), dtype=torch.float32, device=dev)
    out_mask = torch.empty((B, ch, cw), dtype=torch.bool, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    flow_ws = workspace(2 * h * w * 4, dev)                 # the full-frame flow of the sample in flight
    for b, p in enumerate(params):
        e = p.elastic
        field, bumps = None, []
        if e is not None:
            bumps = e["bumps"]
            if len(bumps) > MAX_BUMPS:
                raise RuntimeError(f"flowsynth.synthesize: {len(bumps)} bumps, the kernel takes {MAX_BUMPS}")
            field = elastic_field(p, dev).contiguous()
        theta = (ctypes.c_float * 39)(*p.theta39.tolist())
        flat = [v for bump in bumps for v in bump]
        _lib.call("rfn_flowsynth_flow_f32", dev, theta, TRANSFORMS.index(p.kind), (ctypes.c_float * max(len(flat), 1))(*flat),
                  len(bumps), ptr(field), h, w, ptr(flow_ws), ptr(counts[b]))
        _lib.call("rfn_flowsynth_warp_f32", dev, ptr(img[b]), ptr(flow_ws), ptr(counts[b]), h, w, top, left, ch, cw,
                  float(min_fraction_valid_corr), ptr(out_img[b]), ptr(out_flow[b]), ptr(out_mask[b]))
    return (out_img, out_flow, out_mask, counts) if return_count else (out_img, out_flow, out_mask)


def center_crop(x, size):
    """CenterCrop of a (..., h, w) tensor (a view)"""
    top, left = crop_origin(x.shape[-2], x.shape[-1], size[0], size[1])
    return x[..., top:top + size[0], left:left + size[1]]


class WarpSupervision:
    """The geometric half of the reference's MegaDepth training pipeline over a batch on the device: per sample one
    draw_composite, then synthesize with the crop, and the same CenterCrop of `image` and `image_ref`.
    plan: config.warp_supervision_plan(cfg) -- {"composite": draw_composite's keywords, "crop": (ch, cw) or None,
    "min_fraction_valid_corr": f}.  __call__(sample) takes device tensors image, image_ref, image_prime ((B, 3, h, w) each) and
    optionally image_prime_idx, and returns the keys AlignmentModel.training_step reads: image_ref, image_trg, image_prime,
    flow_prime, mask_prime, prime_trg_idx.
    photometric: config.photometric_plan(cfg) or None.  With a plan the pipeline's photometric half runs in front: image_prime
    is then the uint8 (B, 3, h, w) device tensor of the load-time resize, per sample the draws are photometric.draw followed by
    draw_composite (the reference's order: each sample runs its whole pipeline), and the batch goes through photometric.apply
    into synthesize.  With None every launch and every draw is as it was.
    draw(h, w) makes one sample's draws in that order and returns them; __call__(sample, draws=[...]) takes a batch's draws made
    that way instead of drawing -- for a caller that has draws of its own to make between two samples' (the data module's
    exchange coin comes in front of each sample's pipeline, as in the reference's __getitem__)."""

    def __init__(self, plan, photometric=None):
        self.composite = dict(plan["composite"])
        self.crop = None if plan.get("crop") is None else tuple(plan["crop"])
        self.min_fraction_valid_corr = float(plan.get("min_fraction_valid_corr", 0.1))
        self.photometric = None if photometric is None else dict(photometric)

    def draw(self, h, w):
        """one sample's draws for an (h, w) frame -> (PhotoParams or None, FlowParams)"""
        photo = None
        if self.photometric is not None:
            from . import photometric
            photo = photometric.draw(self.photometric)
        return photo, draw_composite(h, w, **self.composite)

    def __call__(self, sample, draws=None):
        prime = sample["image_prime"]
        prime = prime if prime.dim() == 4 else prime.unsqueeze(0)
        B, _, h, w = prime.shape
        if draws is not None and len(draws) != B:
            raise RuntimeError(f"flowsynth.WarpSupervision: {len(draws)} sets of draws for {B} samples")
        if self.photometric is None:
            params = [draw_composite(h, w, **self.composite) for _ in range(B)] if draws is None else [d[1] for d in draws]
        else:
            from . import photometric
            if not (prime.is_cuda and prime.dtype == torch.uint8):
                raise RuntimeError("flowsynth.WarpSupervision: with a photometric plan image_prime must be the uint8 (B, 3, h, w) "
                                   "HIP (cuda:N) tensor the chain starts from")
            draws = [self.draw(h, w) for _ in range(B)] if draws is None else draws
            photo, params = [d[0] for d in draws], [d[1] for d in draws]
            prime = photometric.apply(prime, photo)
        img, flow, mask = synthesize(prime, params, self.crop, self.min_fraction_valid_corr)
        crop = (lambda x: x) if self.crop is None else (lambda x: center_crop(x, self.crop).contiguous())
        both = lambda x: crop(x if x.dim() == 4 else x.unsqueeze(0))  # noqa: E731
        idx = sample.get("image_prime_idx")
        idx = [0] * B if idx is None else [int(v) for v in torch.as_tensor(idx).flatten().tolist()]
        return {"image_ref": both(sample["image_ref"]), "image_trg": both(sample["image"]), "image_prime": img,
                "flow_prime": flow, "mask_prime": mask, "prime_trg_idx": idx}

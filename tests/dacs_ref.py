"""Reference, fp32 model and driver for the DACS data step (refign_amd/csrc/dacs.hip behind refign_amd/dacs.py): class-mix,
colour jitter and Gaussian blur of a mixed batch.

Used by test_dacs_ref_cpu.py (which shows that the bound below has teeth, and holds the torch fallback in refign_amd/uda.py to
the same reference) and test_dacs_gpu.py (which holds the kernels to it).  Everything except run_kernels is numpy on the CPU.

  reference   the data step in fp64 on the float32 parameters the kernel receives (factors, hue matrix, ImageNet mean / std)
  model32     the same in fp32 with the kernel's 33-tap truncation of the blur (and, optionally, one injected fault)
  run_kernels refign_amd.dacs.mix with explicit jitter, blur_sigma and class_bits
  builders    random, saturating, impulses, constant, labels_edge
  ORDERS      all 24 operator orders; CASES the table every test walks; FAULTS the designated (fault, cases)

The operators, as refign_amd/uda.py and the header of dacs.hip state them:
  mix         where(mask, src, trg); mask from a bit set per sample: bit c = class c for 0 <= c <= 30, bit 31 = the label 255;
              any other label value (negative, 31 .. 254, above 255) is never taken from the source
  jitter      de-normalise (x * std + mean), the four operators in the given order, each followed by a clamp to [0, 1],
              re-normalise ((x - mean) / std).  0 brightness: + (f - 1); 1 contrast: (x - m) f + m about the mean m of the whole
              image (3 channels) as it stands in front of the operator; 2 saturation: (x - y) f + y about the luma
              y = 0.299 r + 0.587 g + 0.114 b; 3 hue: a 3x3 matrix on (r, g, b)
  blur        separable, rows then columns, `reflect` border (no edge repeat); window ks = window(extent) per axis (~0.1 x the
              extent, odd), taps exp(-t^2 / 2 sigma^2) normalised over the whole window
  labels      where(mask, gt, pseudo); weights where(mask, 1, pseudo_weight)

The bound of the GPU tests, in the metric rel_err = max|got - want| / max(1, max|want|):  bound(E) = min(M E + 2^-23, 1e-5),
E = rel_err of model32 against reference on the very same input.  M covers what the model does not transcribe (fma
contraction, the summation order of the contrast mean): other draws of the same rounding noise.  profiles/dacs_reference.txt
holds the measured kernel / E ratios.
"""
import dataclasses
import functools
import itertools
import math

import numpy as np

S = 0.2                                          # colour-jitter strength of every case
M = 4.0                                          # profiles/dacs_reference.txt
FLOOR = 2.0 ** -23
CAP = 1e-5                                       # the bound the suite held before: never exceeded
BLUR_R = 16                                      # kBlurR of dacs.hip
MAX_BATCH = 8                                    # kDacsMaxBatch
MEAN32 = np.array((0.485, 0.456, 0.406), np.float32)
STD32 = np.array((0.229, 0.224, 0.225), np.float32)
_YIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]])
ORDERS = tuple(itertools.permutations(range(4)))


@dataclasses.dataclass(frozen=True)
class Case:
    """One batch.  src, trg (B, 3, H, W) float32; gt, pseudo (B, H, W) int64; pweight (B, H, W) float32; bits: B ints;
    jitter: per sample None or (order[4], factor[4] by operator, hue (3, 3) float32); sigma: per sample None or float;
    draws: per sample None or the uniforms behind `jitter` in the order uda._color_jitter draws them."""
    src: np.ndarray
    trg: np.ndarray
    gt: np.ndarray
    pseudo: np.ndarray
    pweight: np.ndarray
    bits: tuple
    jitter: tuple
    sigma: tuple
    draws: tuple

    @property
    def shape(self):
        return self.gt.shape


def window(extent):
    """dacs.mix's rule for the blur window (kornia's, dacs_transforms.py:68-72): ~0.1 x the extent, odd."""
    c = math.ceil(0.1 * extent)
    return int(math.floor(c - 0.5 + c % 2))


def bound(E):
    return min(M * E + FLOOR, CAP)


def rel_err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / max(1.0, float(np.abs(want).max()))


# ---------------------------------------------------------------------------------------------------------------------
# the data step, once for both precisions
# ---------------------------------------------------------------------------------------------------------------------
FAULT_NAMES = ("contrast_mean_unjittered", "factor_by_position", "no_clamp_after_saturation", "hue_transposed",
               "blur_symmetric", "taps_norm_33", "mask_ignores_255", "class30_out_of_range")


def class_mask(gt, bits, fault=None):
    """(B, H, W) bool: the pixels taken from the source."""
    out = np.zeros(gt.shape, bool)
    top = 29 if fault == "class30_out_of_range" else 30
    for n, b in enumerate(bits):
        for c in range(top + 1):
            if (b >> c) & 1:
                out[n] |= gt[n] == c
        if (b >> 31) & 1 and fault != "mask_ignores_255":
            out[n] |= gt[n] == 255
    return out


def _jitter(x, order, factor, hue, dt, fault):
    """x (3, H, W) in [0, 1]-space, of dtype dt."""
    x0 = x
    for k, op in enumerate(order):
        f = dt(factor[k if fault == "factor_by_position" else op])
        if op == 0:
            x = x + (f - dt(1))
        elif op == 1:
            of = x0 if fault == "contrast_mean_unjittered" else x
            mu = dt(of.sum(dtype=np.float64) / of.size)
            x = (x - mu) * f + mu
        elif op == 2:
            gray = dt(0.299) * x[0] + dt(0.587) * x[1] + dt(0.114) * x[2]
            x = (x - gray) * f + gray
        else:
            h = (hue.T if fault == "hue_transposed" else hue).astype(dt)
            x = np.stack([h[i, 0] * x[0] + h[i, 1] * x[1] + h[i, 2] * x[2] for i in range(3)])
        if not (op == 2 and fault == "no_clamp_after_saturation"):
            x = np.clip(x, dt(0), dt(1))
        assert x.dtype == dt
    return x


def taps(ks, sigma, truncate, fault=None):
    """float64 taps of a window of ks.  truncate: the kernel's |t| <= 16.  Fault taps_norm_33: the divisor is the sum over all
    33 taps whatever the window."""
    rad = min(ks // 2, BLUR_R) if truncate else ks // 2
    g = lambda r: np.exp(-np.arange(-r, r + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))   # noqa: E731
    return g(rad) / (g(BLUR_R) if fault == "taps_norm_33" else g(rad)).sum()


def _blur_axis(x, w, axis, dt, mode):
    rad, n = len(w) // 2, x.shape[axis]
    pad = [(0, 0)] * x.ndim
    pad[axis] = (rad, rad)
    xp = np.pad(x, pad, mode=mode)
    acc = np.zeros_like(x)
    for t in range(2 * rad + 1):                                   # t = -rad .. rad in the kernel's order
        sl = [slice(None)] * x.ndim
        sl[axis] = slice(t, t + n)
        if dt is np.float32:                                       # the kernel's fmaf: the product of two floats is exact in fp64
            acc = (acc.astype(np.float64) + np.float64(np.float32(w[t])) * xp[tuple(sl)].astype(np.float64)).astype(np.float32)
        else:
            acc = acc + dt(w[t]) * xp[tuple(sl)]
    assert acc.dtype == dt
    return acc


def _data_step(c, dt, truncate, fault):
    assert fault is None or fault in FAULT_NAMES, fault
    B, H, W = c.shape
    mask = class_mask(c.gt, c.bits, fault)
    img = np.where(mask[:, None], c.src, c.trg).astype(dt)
    mean, std = MEAN32.astype(dt).reshape(3, 1, 1), STD32.astype(dt).reshape(3, 1, 1)
    mode = "symmetric" if fault == "blur_symmetric" else "reflect"
    for n in range(B):
        x = img[n]
        if c.jitter[n] is not None:
            order, factor, hue = c.jitter[n]
            x = (_jitter(x * std + mean, order, factor, hue, dt, fault) - mean) / std
        if c.sigma[n] is not None:
            x = _blur_axis(x, taps(window(H), c.sigma[n], truncate, fault), 1, dt, mode)
            x = _blur_axis(x, taps(window(W), c.sigma[n], truncate, fault), 2, dt, mode)
        img[n] = x
    return img, np.where(mask, c.gt, c.pseudo), np.where(mask, np.float32(1), c.pweight)


def reference(c):
    """(img float64, lbl int64, wgt float32): the data step in fp64, the blur over its whole window."""
    return _data_step(c, np.float64, False, None)


def model32(c, fault=None):
    """The same in fp32 as dacs.hip orders it, with the 33-tap truncation of the blur; `fault`: one of FAULT_NAMES -- what a
    kernel with that defect would compute.  The blur accumulates with the kernel's explicit fmaf.  Not transcribed: the
    compiler's fma contraction in the jitter chain; the contrast mean is the float32 of an fp64 sum (the kernel adds fp32
    partial sums of a workgroup in fp64)."""
    return _data_step(c, np.float32, True, fault)


def plain_mix(c):
    """where(mask, src, trg) in float32: what every sample that is neither jittered nor blurred must equal bit for bit."""
    return np.where(class_mask(c.gt, c.bits)[:, None], c.src, c.trg)


# ---------------------------------------------------------------------------------------------------------------------
# jitter parameters from uniforms, as dacs.draw_jitter / uda._color_jitter make them from torch's generator
# ---------------------------------------------------------------------------------------------------------------------
def make_jitter(order, u_op, u_hue):
    """order: a permutation of (0, 1, 2, 3); u_op[op]: the uniform of operator op; u_hue: the hue angle's uniform.  Returns
    ((order, factor, hue) with float32 values, draws in the order the generator is asked)."""
    lo = max(0.0, 1 - S)
    factor = [float(np.float32(lo + u * (1 + S - lo))) for u in u_op]
    h = (2.0 * u_hue - 1.0) * S * 2 * math.pi
    cs, sn = math.cos(h), math.sin(h)
    hue = (np.linalg.inv(_YIQ) @ np.array([[1, 0, 0], [0, cs, -sn], [0, sn, cs]]) @ _YIQ).astype(np.float32)
    draws = []
    for op in order:
        draws.append(u_op[op])
        if op == 3:
            draws.append(u_hue)
    return (list(order), factor, hue), draws


def order_jitter(i):
    """Order i of ORDERS with factors at 1 - s, 1 + s and an interior value, hue angle at -s 2 pi, +s 2 pi and an interior value,
    rotating with i; no two neighbouring operator codes share a factor (a factor indexed by position shows)."""
    interior = (0.3, 0.45, 0.6, 0.7)
    u_op = [(0.0, 1.0, interior[op])[(i + op) % 3] for op in range(4)]
    return make_jitter(ORDERS[i], u_op, (0.0, 1.0, 0.29)[i % 3])


# ---------------------------------------------------------------------------------------------------------------------
# builders: (src, trg, gt, pseudo, pweight, bits)
# ---------------------------------------------------------------------------------------------------------------------
def _labels(g, B, H, W, values, block):
    v = np.asarray(values, np.int64)
    gt = v[g.integers(0, len(v), (B, -(-H // block), -(-W // block)))].repeat(block, 1).repeat(block, 2)[:, :H, :W].copy()
    noise = g.random((B, H, W)) < 0.05
    gt[noise] = v[g.integers(0, len(v), int(noise.sum()))]
    return gt


def _common(g, B, H, W):
    gt = _labels(g, B, H, W, list(range(19)) + [255], 8)
    bits = []
    for n in range(B):                                              # about half of the 19 classes; 255 for odd samples
        b = sum(1 << int(k) for k in g.choice(19, 10, replace=False))
        bits.append(b | ((n & 1) << 31))
    return gt, g.integers(0, 19, (B, H, W)), g.random((B, H, W), dtype=np.float32), tuple(bits)


def build_random(seed, B, H, W):
    """randn images: after jitter 0-20 % of the values sit on a clamp."""
    g = np.random.default_rng(seed)
    src, trg = (g.standard_normal((B, 3, H, W), dtype=np.float32) for _ in range(2))
    return (src, trg) + _common(g, B, H, W)


def build_saturating(seed, B, H, W):
    """[0, 1]-space values uniform in (-0.4, 1.4): a third is clamped by the first operator, so the mean of the image in front
    of an operator is not the mean behind it."""
    g = np.random.default_rng(seed)
    norm = lambda v: ((v - MEAN32.reshape(3, 1, 1)) / STD32.reshape(3, 1, 1)).astype(np.float32)   # noqa: E731
    src, trg = (norm(g.uniform(-0.4, 1.4, (B, 3, H, W)).astype(np.float32)) for _ in range(2))
    return (src, trg) + _common(g, B, H, W)


def build_impulses(seed, B, H, W):
    """Zero but for deltas at (0, 0), (H - 1, W - 1) and (1, W - 2), of another height per sample, channel and image."""
    g = np.random.default_rng(seed)
    src, trg = np.zeros((B, 3, H, W), np.float32), np.zeros((B, 3, H, W), np.float32)
    amp = np.array([1.0, -2.0, 3.0], np.float32)
    for n in range(B):
        for y, x in ((0, 0), (H - 1, W - 1), (1, W - 2)):
            src[n, :, y, x] = amp * (1 + n)
            trg[n, :, y, x] = -0.5 * amp * (1 + n)
    return (src, trg) + _common(g, B, H, W)


def build_constant(seed, B, H, W):
    """One value per sample and channel, the same in both images: the blur must give it back (the taps sum to 1)."""
    g = np.random.default_rng(seed)
    v = g.uniform(-2.0, 2.0, (B, 3, 1, 1)).astype(np.float32)
    src = np.broadcast_to(v, (B, 3, H, W)).copy()
    return (src, src.copy()) + _common(g, B, H, W)


EDGE_LABELS = (0, 5, 18, 30, 31, 40, 254, 255, -1)


def build_labels_edge(seed, B, H, W):
    """Labels from EDGE_LABELS in 4x4 blocks; bit sets with every combination of bit 30 and bit 31 over a random choice of
    {0, 5, 18}.  (Label 31 is never taken, not even when bit 31 is set: that bit stands for 255.)"""
    g = np.random.default_rng(seed)
    src, trg = (g.standard_normal((B, 3, H, W), dtype=np.float32) for _ in range(2))
    gt = _labels(g, B, H, W, EDGE_LABELS, 4)
    bits = []
    for n in range(B):
        b = sum(1 << k for k in (0, 5, 18) if g.random() < 0.6)
        bits.append(b | ((n & 1) << 30) | (((n >> 1) & 1) << 31))
    return src, trg, gt, g.integers(0, 19, (B, H, W)), g.random((B, H, W), dtype=np.float32), tuple(bits)


BUILDERS = {"random": build_random, "saturating": build_saturating, "impulses": build_impulses, "constant": build_constant,
            "labels_edge": build_labels_edge}


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
JITTER_SHAPES = ((40, 72), (18, 22))             # 720 quads: the third workgroup of 256 is partly idle; W % 4 != 0
BLUR_SHAPES = ((17, 20), (40, 72), (344, 24), (24, 700))     # windows 1x1, 3x7, 35x3 (35 > 33 taps), 3x69 (11 column blocks)
BLUR_SIGMA = (0.15, None, 0.5, 1.15, None)
# contrast (code 1) at each of its four positions, twice; brightness (code 0) first wherever contrast is not
CONTRAST_ORDERS = ((1, 0, 2, 3), (0, 1, 2, 3), (0, 2, 1, 3), (0, 2, 3, 1), (1, 0, 3, 2), (0, 1, 3, 2), (0, 3, 1, 2), (0, 3, 2, 1))


def _mk(built, jit, sigma):
    jitter = tuple(None if j is None else j[0] for j in jit)
    draws = tuple(None if j is None else tuple(j[1]) for j in jit)
    return Case(*built, jitter=jitter, sigma=tuple(sigma), draws=draws)


def _jitter_case(shape, third, even_only):
    def make():
        jit = [order_jitter(8 * third + n) for n in range(8)]
        if even_only:
            jit = [j if n % 2 == 0 else None for n, j in enumerate(jit)]
        return _mk(build_random(100 + 10 * JITTER_SHAPES.index(shape) + third, 8, *shape), jit, [None] * 8)
    return make


def _contrast_case():
    # brightness at 1 + s pushes a third of the values onto the upper clamp; contrast at 1 - s and 1 + s in turn
    jit = [make_jitter(o, [1.0, float(n % 2), 0.8, 0.55], 0.29) for n, o in enumerate(CONTRAST_ORDERS)]
    return _mk(build_saturating(200, 8, 40, 72), jit, [None] * 8)


def _mask_case():
    jit = [order_jitter(3 * n + 2) if n % 2 == 0 else None for n in range(8)]
    return _mk(build_labels_edge(300, 8, 40, 72), jit, [0.5 if n in (2, 3) else None for n in range(8)])


def _blur_case(shape, builder):
    def make():
        B = len(BLUR_SIGMA)
        return _mk(BUILDERS[builder](400 + BLUR_SHAPES.index(shape), B, *shape), [None] * B, BLUR_SIGMA)
    return make


def _both_case():
    # every combination of jitter on / off and blur on / off in one batch of 8, three sigmas
    jit = [order_jitter(3 * n + 1) if n % 2 == 0 else None for n in range(8)]
    return _mk(build_random(500, 8, 40, 72), jit, [(0.15, 1.15, None, None, 0.5, 0.8, None, None)[n] for n in range(8)])


def _table():
    t = {}
    for h, w in JITTER_SHAPES:
        for third in range(3):
            t[f"jitter-{h}x{w}-{third}"] = _jitter_case((h, w), third, False)
            t[f"jitter-{h}x{w}-{third}-even"] = _jitter_case((h, w), third, True)
    t["contrast-40x72"] = _contrast_case
    t["mask-40x72"] = _mask_case
    for h, w in BLUR_SHAPES:
        for builder in ("random", "impulses", "constant"):
            t[f"blur-{h}x{w}-{builder}"] = _blur_case((h, w), builder)
    t["both-40x72"] = _both_case
    return t


CASES = _table()
JITTER_CASES = tuple(n for n in CASES if n.startswith("jitter-") and not n.endswith("-even"))
EVEN_CASES = tuple(n for n in CASES if n.endswith("-even"))
BLUR_CASES = tuple(n for n in CASES if n.startswith("blur-"))

# fault -> cases where a kernel with that defect must be caught
FAULTS = {
    "contrast_mean_unjittered": ("contrast-40x72",),
    "factor_by_position": JITTER_CASES,
    "no_clamp_after_saturation": JITTER_CASES,
    "hue_transposed": JITTER_CASES,
    "blur_symmetric": tuple(n for n in BLUR_CASES if n.endswith("impulses") and "17x20" not in n),   # (a 1x1 window has no border)
    "taps_norm_33": tuple(n for n in BLUR_CASES if n.endswith("constant") and "17x20" not in n),     # (every axis here has a 3-window)
    "mask_ignores_255": ("mask-40x72",),
    "class30_out_of_range": ("mask-40x72",),
}
LABEL_FAULTS = ("mask_ignores_255", "class30_out_of_range")


@functools.lru_cache(maxsize=None)
def case(name):
    """Shared; do not modify."""
    c = CASES[name]()
    for a in (c.src, c.trg, c.gt, c.pseudo, c.pweight):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case_reference(name):
    return reference(case(name))


@functools.lru_cache(maxsize=None)
def case_model(name, fault=None):
    return model32(case(name), fault)


def case_E(name):
    return rel_err(case_model(name)[0], case_reference(name)[0])


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
def run_kernels(c, dev, part="all"):
    """refign_amd.dacs.mix on the case's arrays with its jitter, blur_sigma and class_bits: (img, lbl, wgt) device tensors
    (None for the half that `part` leaves out)."""
    import torch
    from refign_amd import dacs
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    src, trg = (t(c.src), t(c.trg)) if part != "labels" else (None, None)
    pseudo, pweight = (t(c.pseudo), t(c.pweight)) if part != "image" else (None, None)
    bits = torch.tensor(list(c.bits), dtype=torch.int64, device=dev)
    return dacs.mix(src, trg, t(c.gt), pseudo, pweight, bits, list(c.jitter), list(c.sigma), part=part)

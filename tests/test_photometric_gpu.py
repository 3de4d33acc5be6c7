"""GPU: the photometric chain on image_prime (csrc/photometric.hip through refign_amd/photometric.py) against a restatement of
torchvision's tensor path for uint8 images in torch operations on the CPU, so that every intermediate dtype is torch's:

    gray(img)         (0.2989 r + 0.587 g + 0.114 b).to(uint8)
    blend(a, b, f)    (f a + (1.0 - f) b).clamp(0, 255).to(uint8)
    brightness / contrast / saturation: blend with 0 / the fp32 mean of gray(img) / gray(img), in the order drawn
    out[c] = in[perm[c]];  the 7 x 7 blur under reflect padding, torch.round, uint8;  (u8 / 255 - mean) / std

torchvision itself is not installed: parity with it is NOT verified here, the kernel is pinned to this restatement.

Without blur the fp32 output is held BIT-EQUAL.  The shapes of those cases satisfy 255 H W < 2^24, where every summation order
of the contrast mean is exact (torch.mean and the exact integer sum divided once agree: asserted).  With blur the oracle
accumulates the 49 taps in fp64 from the same fp32 weights: a pixel whose fp64 value lies further than 1e-3 from a half-integer
must be bit-equal (fp32 and fp64 accumulation differ by at most 7.3e-5 grey levels at these shapes, a wrong tap by up to
255 times its weight), the remaining pixels may differ by one grey level, and their share is capped at 3 % per sample -- a
condition on the seeded images (the oracle alone decides it), not a measurement.  The kernel's tile is 64 x 16: (37, 150)
spans three tiles each way with ragged edges."""
import itertools
import os
import random

import pytest
import torch
import torch.nn.functional as F

from guardband import FILLS, GuardArena

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SHAPES = [(4, 5), (37, 53), (37, 150)]
ORDERS = list(itertools.permutations(range(4)))
PERMS = list(itertools.permutations(range(3)))
HALF_MARGIN, EXEMPT_CAP = 1e-3, 0.03


# ---- the oracle: torch operations on the CPU ---------------------------------------------------------------------------------
def gray(img):
    r, g, b = img.unbind(0)
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(torch.uint8)


def blend(a, b, f):
    return (f * a + (1.0 - f) * b).clamp(0, 255).to(torch.uint8)


def jitter(img, p, mean="exact"):
    """-> the jittered, shuffled uint8 image and the int64 sum of gray() in front of the contrast step (0 without one).
    mean: "exact" -- (float)sum / (float)n, one division -- or "torch" -- torch.mean of the fp32 gray image"""
    x, gsum = img, 0
    for s in p.order:
        f = p.factors[s] if s < 3 else None
        if f is None:
            continue
        if s == 0:
            x = blend(x, torch.zeros_like(x), f)
        elif s == 1:
            g = gray(x)
            gsum = int(g.to(torch.int64).sum())
            if mean == "exact":
                m = torch.tensor(gsum, dtype=torch.int64).to(torch.float32) / torch.tensor(g.numel(), dtype=torch.float32)
            else:
                m = torch.mean(g.to(torch.float32))
            x = blend(x, m, f)
        else:
            x = blend(x, gray(x).unsqueeze(0), f)
    return x[list(p.perm)], gsum


def normalise(u8, p):
    mean, std = torch.tensor(p.mean, dtype=torch.float32), torch.tensor(p.std, dtype=torch.float32)
    return (u8.to(torch.float32) / 255 - mean[:, None, None]) / std[:, None, None]


def blur64(u8, kernel):
    """the 49-tap sum of the reflect-padded image in fp64 from the fp32 weights, before rounding"""
    _, h, w = u8.shape
    x = F.pad(u8.to(torch.float32)[None], (3, 3, 3, 3), mode="reflect")[0].double()
    acc = torch.zeros(3, h, w, dtype=torch.float64)
    for dy in range(7):
        for dx in range(7):
            acc += kernel[dy, dx].double() * x[:, dy:dy + h, dx:dx + w]
    return acc


def oracle(img, p, mean="exact"):
    """-> (fp32 output, gray sum, exempt mask or None): the chain of one sample"""
    x, gsum = jitter(img, p, mean)
    if p.sigma is None:
        return normalise(x, p), gsum, None
    acc = blur64(x, p.kernel)
    exempt = ((acc - torch.floor(acc)) - 0.5).abs() <= HALF_MARGIN
    return normalise(torch.round(acc).to(torch.uint8), p), gsum, exempt


def levels(out, p):
    """the grey level of every output value: each must be the normalised form of one of the 256 levels, bit for bit"""
    table = normalise(torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(3, 256, 1).contiguous(), p)[:, :, 0]
    idx = (out.unsqueeze(-1) - table.view(3, 1, 1, 256)).abs().argmin(-1)
    assert torch.equal(torch.gather(table, 1, idx.view(3, -1)).view_as(out), out), "an output value that no grey level gives"
    return idx


def check_sample(got, img, p, ctx):
    want, _, exempt = oracle(img, p)
    if exempt is None:
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
            (ctx, int((got != want).sum()), float((got - want).abs().max()))
        return 0.0
    share = float(exempt.float().mean())
    print(f"{ctx}: sigma {p.sigma}: {int(exempt.sum())} of {exempt.numel()} values within {HALF_MARGIN} of a half ({share:.4f})")
    assert share <= EXEMPT_CAP, (ctx, share)
    strict = ~exempt
    assert torch.equal(got.view(torch.int32)[strict], want.view(torch.int32)[strict]), (ctx, int((got != want)[strict].sum()))
    d = (levels(got, p) - levels(want, p)).abs()
    assert int(d[exempt].max() if exempt.any() else 0) <= 1, (ctx, int(d.max()))
    return share


def run(dev, imgs, params):
    from refign_amd import photometric
    return photometric.apply(imgs.to(dev), params).cpu()


def images(seed, B, h, w):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 3, h, w), dtype=torch.uint8, generator=g)


def param_set(orders, sigma=None):
    """one parameter set per order: factors at both ends of [0.4, 1.6] in every pairing, contrast absent in every third, the six
    channel permutations in turn"""
    from refign_amd import photometric
    out = []
    for i, order in enumerate(orders):
        sig = sigma[i % len(sigma)] if isinstance(sigma, (list, tuple)) else sigma
        out.append(photometric.params_from(order, (0.4, 1.6)[i % 2], (1.6, 0.4, None)[i % 3], (0.4, 1.6)[(i // 2) % 2],
                                           PERMS[i % 6], sig, mean=MEAN, std=STD))
    return out


# ---- without blur: bit-equal ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_no_blur_is_bit_equal(dev, shape):
    """all 24 step orders at (37, 53), six elsewhere; both ends of the factor range, contrast absent, all six permutations"""
    h, w = shape
    assert 255 * h * w < 2 ** 24
    orders = ORDERS if shape == (37, 53) else ORDERS[::4]
    params = param_set(orders)
    assert {tuple(p.perm) for p in params} == set(PERMS) and any(p.contrast is None for p in params)
    imgs = images(0, len(params), h, w)
    got = run(dev, imgs, params)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(params), 3, h, w)
    for b, p in enumerate(params):
        check_sample(got[b], imgs[b], p, f"{shape} order {p.order}")
        if p.contrast is not None:                               # at these sizes torch's own mean is the same number
            assert torch.equal(oracle(imgs[b], p, "torch")[0], oracle(imgs[b], p, "exact")[0])


def test_constant_images_and_the_grey_ramp(dev):
    """all 0, all 255, and r = g = b = 0 .. 255, where gray() truncates 0.9999 v below v"""
    ramp = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).expand(3, 16, 16)
    assert int((gray(ramp.contiguous()).view(-1).int() < torch.arange(256)).sum()) > 100
    imgs = torch.stack([torch.zeros(3, 16, 16, dtype=torch.uint8), torch.full((3, 16, 16), 255, dtype=torch.uint8), ramp])
    for params in (param_set(ORDERS[0:3]), param_set(ORDERS[9:12]), param_set(ORDERS[14:17]), param_set(ORDERS[21:24])):
        got = run(dev, imgs, params)
        for b, p in enumerate(params):
            check_sample(got[b], imgs[b], p, f"image {b} order {p.order}")


def test_identity_parameters_only_convert(dev):
    from refign_amd import photometric
    imgs = images(1, 1, 19, 70)
    p = photometric.params_from([0, 1, 2, 3], None, None, None, [0, 1, 2], None, mean=MEAN, std=STD)
    got = run(dev, imgs, [p])
    assert torch.equal(got[0].view(torch.int32), normalise(imgs[0], p).view(torch.int32))


# ---- with blur -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(7, 7)])
def test_blur(dev, shape):
    """sigma 0.2, 0.7 and 2.0 behind a jitter and a shuffle; at (4, 5) every tap but the centre's is reflected"""
    h, w = shape
    params = param_set([ORDERS[5], ORDERS[10], ORDERS[19], ORDERS[0], ORDERS[14], ORDERS[23]], sigma=[0.2, 0.7, 2.0])
    assert sorted({p.sigma for p in params}) == [0.2, 0.7, 2.0]
    torch.manual_seed(0)
    imgs = torch.randint(0, 256, (len(params), 3, h, w), dtype=torch.uint8)
    got = run(dev, imgs, params)
    for b, p in enumerate(params):
        check_sample(got[b], imgs[b], p, f"{shape} order {p.order}")


def test_blur_alone_and_a_smaller_kernel(dev):
    from refign_amd import photometric
    imgs = images(3, 2, 21, 67)
    params = [photometric.params_from([0, 1, 2, 3], None, None, None, [0, 1, 2], 1.1, mean=MEAN, std=STD),
              photometric.params_from([0, 1, 2, 3], None, None, None, [0, 1, 2], 0.9, kernel_size=3, mean=MEAN, std=STD)]
    got = run(dev, imgs, params)
    for b, p in enumerate(params):
        check_sample(got[b], imgs[b], p, f"kernel {p.kernel_size}")
    # the 3 x 3 kernel against its own 1-pixel reflect padding: the zero taps of the 7 x 7 form add nothing
    k3 = params[1].kernel[2:5, 2:5].double()
    x = F.pad(imgs[1].float()[None], (1, 1, 1, 1), mode="reflect")[0].double()
    acc = sum(k3[dy, dx] * x[:, dy:dy + 21, dx:dx + 67] for dy in range(3) for dx in range(3))
    assert torch.equal(acc, blur64(imgs[1], params[1].kernel))


# ---- batches -------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_equals_the_samples_alone(dev):
    from refign_amd import photometric
    imgs = images(4, 3, 37, 150).to(dev)
    params = [photometric.params_from([1, 0, 2, 3], 0.7, 1.3, 0.5, [1, 2, 0], None, mean=MEAN, std=STD),
              photometric.params_from([2, 3, 1, 0], 1.4, 0.6, 1.2, [2, 1, 0], 1.3, mean=MEAN, std=STD),
              photometric.params_from([3, 0, 2, 1], 1.1, None, 0.9, [0, 2, 1], None, mean=MEAN, std=STD)]
    batch = photometric.apply(imgs, params)
    for b, p in enumerate(params):
        alone = photometric.apply(imgs[b], p)
        assert tuple(alone.shape) == (1, 3, 37, 150)
        assert torch.equal(batch[b].view(torch.int32), alone[0].view(torch.int32)), b
    sums = photometric.gray_sums(imgs, params).cpu().tolist()
    want = [jitter(imgs[b].cpu(), p)[1] for b, p in enumerate(params)]
    assert sums == want and sums[2] == 0 and sums[0] > 0
    out = torch.empty_like(batch)
    assert photometric.apply(imgs, params, out=out) is out and torch.equal(out, batch)


def test_full_size_sample(dev):
    """750 x 750: the sum of gray() exceeds 2^24, torch's fp32 mean is no longer exact; the kernel's is (float)sum / (float)n"""
    from refign_amd import photometric
    img = images(5, 1, 750, 750)
    p = photometric.params_from([0, 1, 2, 3], 1.3, 0.7, 1.4, [2, 0, 1], None, mean=MEAN, std=STD)
    want, gsum, _ = oracle(img[0], p, "exact")
    assert gsum > 2 ** 24
    d = img.to(dev)
    assert photometric.gray_sums(d, [p]).cpu().tolist() == [gsum]
    got = photometric.apply(d, [p]).cpu()[0]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), int((got != want).sum())
    # against torch.mean: counted, not asserted (README: the first of the two deviations)
    other = oracle(img[0], p, "torch")[0]
    n = int((got != other).sum())
    line = (f"750 x 750, seed 5, order {p.order}, contrast {p.contrast}: {n} of {got.numel()} output values differ from the "
            f"restatement that takes torch.mean of the fp32 gray image (sum of gray {gsum}, exact mean "
            f"{gsum / 562500:.7f}, torch.mean {float(torch.mean(gray(blend(img[0], torch.zeros_like(img[0]), 1.3)).float())):.7f}); "
            f"0 differ from the restatement that divides the exact sum once")
    print(line)
    path = os.environ.get("RFN_PHOTOMETRIC_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


# ---- how it runs ---------------------------------------------------------------------------------------------------------------
def test_no_host_synchronisation_and_repeatability(dev):
    from refign_amd import determinism, photometric
    imgs = images(6, 2, 37, 150).to(dev)
    params = param_set([ORDERS[7], ORDERS[16]], sigma=[None, 1.7])
    first = photometric.apply(imgs, params)
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = photometric.apply(imgs, params)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    with determinism.deterministic():                            # no refused kernel: integer atomics only
        third = photometric.apply(imgs, params)
    assert torch.equal(first.view(torch.int32), third.view(torch.int32))


def test_arguments(dev):
    from refign_amd import photometric
    p = photometric.params_from([0, 1, 2, 3], 1.0, 1.0, 1.0, [0, 1, 2], None)
    blurred = photometric.params_from([0, 1, 2, 3], 1.0, 1.0, 1.0, [0, 1, 2], 1.0)
    img = images(7, 2, 8, 8).to(dev)
    with pytest.raises(RuntimeError, match="no CPU path"):
        photometric.apply(img.cpu(), [p, p])
    with pytest.raises(RuntimeError, match="no CPU path"):
        photometric.apply(img.float(), [p, p])
    with pytest.raises(RuntimeError, match="as many"):
        photometric.apply(img, [p])
    for shape in ((3, 3, 9), (3, 9, 3)):
        with pytest.raises(RuntimeError, match="cannot be blurred"):
            photometric.apply(torch.zeros(shape, dtype=torch.uint8, device=dev), blurred)
        assert tuple(photometric.apply(torch.zeros(shape, dtype=torch.uint8, device=dev), p).shape) == (1, *shape)
    with pytest.raises(RuntimeError, match="out must"):
        photometric.apply(img, [p, p], out=torch.empty(2, 3, 8, 9, device=dev))


def test_guard_band(dev):
    """inside the poisoned arena: untouched guards, equal bits across the fills, and the oracle's bits"""
    from refign_amd import photometric
    imgs = images(8, 2, 21, 70)
    params = param_set([ORDERS[3], ORDERS[20]], sigma=[None, 0.7])
    bits = []
    for fill in FILLS:
        arena = GuardArena(dev, fill, 4 << 20, skew=1)
        placed = arena.place(imgs.to(dev))
        with arena.allocations():
            got = photometric.apply(placed, params)
            sums = photometric.gray_sums(placed, params)
        arena.check()
        assert torch.equal(placed.cpu(), imgs), "the image is read only"
        bits.append((got.cpu(), sums.cpu()))
    for got, sums in bits[1:]:
        assert torch.equal(got.view(torch.int32), bits[0][0].view(torch.int32)) and torch.equal(sums, bits[0][1])
    for b, p in enumerate(params):
        check_sample(bits[0][0][b], imgs[b], p, f"guard band sample {b}")


# ---- WarpSupervision -----------------------------------------------------------------------------------------------------------
def test_warp_supervision_with_the_photometric_plan(dev):
    from refign_amd import flowsynth, photometric
    h, w, crop = 72, 88, (48, 64)
    plan = {"composite": {"include_transforms": ["hom", "tps", "afftps"], "random_t_hom": 0.3, "random_t_tps": 0.3,
                          "random_t_tps_for_afftps": 0.2, "add_elastic": False}, "crop": crop, "min_fraction_valid_corr": 0.1}
    photo = {"brightness": (0.4, 1.6), "contrast": (0.4, 1.6), "saturation": (0.4, 1.6), "shuffle": True,
             "blur": {"p": 0.5, "kernel_size": 7, "sigma": (0.2, 2.0)}, "mean": MEAN, "std": STD}
    B = 3
    prime = images(9, B, h, w).to(dev)
    fp = normalise(images(10, 1, h, w)[0], photometric.params_from([0, 1, 2, 3], None, None, None, [0, 1, 2], None)).to(dev)
    sample = {"image": fp.unsqueeze(0).repeat(B, 1, 1, 1), "image_ref": fp.unsqueeze(0).repeat(B, 1, 1, 1) * 0.5, "image_prime": prime}
    random.seed(21)
    torch.manual_seed(21)
    batch = flowsynth.WarpSupervision(plan, photometric=photo)(sample)
    tails = (random.random(), torch.rand(1).item())
    # by hand: per sample photometric.draw, then draw_composite; apply; synthesize
    random.seed(21)
    torch.manual_seed(21)
    pp, fpars = [], []
    for _ in range(B):
        pp.append(photometric.draw(photo))
        fpars.append(flowsynth.draw_composite(h, w, **plan["composite"]))
    assert tails == (random.random(), torch.rand(1).item())
    img, flow, mask = flowsynth.synthesize(photometric.apply(prime, pp), fpars, crop, 0.1)
    assert torch.equal(batch["image_prime"].view(torch.int32), img.view(torch.int32))
    assert torch.equal(batch["flow_prime"].view(torch.int32), flow.view(torch.int32)) and torch.equal(batch["mask_prime"], mask)
    assert tuple(batch["image_trg"].shape) == (B, 3, *crop)
    # photometric=None: the call as it was
    fsample = dict(sample, image_prime=photometric.apply(prime, pp))
    outs = []
    for ws in (flowsynth.WarpSupervision(plan), flowsynth.WarpSupervision(plan, photometric=None)):
        random.seed(22)
        torch.manual_seed(22)
        outs.append((ws(fsample), random.random(), torch.rand(1).item()))
    for k in ("image_prime", "flow_prime", "mask_prime", "image_ref", "image_trg"):
        assert torch.equal(outs[0][0][k], outs[1][0][k]), k
    assert outs[0][1:] == outs[1][1:]
    with pytest.raises(RuntimeError, match="uint8"):
        flowsynth.WarpSupervision(plan, photometric=photo)(fsample)

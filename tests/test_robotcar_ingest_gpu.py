"""GPU: the labelled RobotCar section on the device -- Pillow's NEAREST rotation (csrc/rotate.hip), ColorJitter's hue step
(csrc/photometric.hip), the fused rotation + crop + jitter + mirror + normalisation pass (photometric.apply(geometry=)) and
datastep.RotatedLabelledSampler.

Operands.  The rotation: tests/golden/rotate_pillow.npz (Pillow's own pixels) at 5 x 7, 37 x 53 and 64 x 16, and
test_rotate_cpu.rotate_reference (held bit-equal to Pillow there) at 720 x 720.  The hue step: `hue_step` below, torchvision's
tensor path for a uint8 image (functional_tensor.py: adjust_hue, _rgb2hsv, _hsv2rgb) restated in torch operations on the CPU,
every intermediate an fp32 tensor; the einsum of _hsv2rgb over the six one-hot masks adds five zeros to the selected value
and is written as that selection.  torchvision itself is not installed: parity with it is NOT verified here, the kernel is
pinned to this restatement.  The rest of the chain: the restatement of tests/test_photometric_gpu.py, repeated here.

Everything is held BIT-EQUAL: each operation is a single IEEE fp32 operation on both sides (shapes with 255 h w < 2^24 where a
contrast mean is compared with the oracle's, so that every summation order of it is exact), and the fused pass is compared with
the composition of the pieces tested before it, which computes the same numbers in the same order."""
import itertools
import random

import numpy as np
import pytest
import torch
from conftest import golden

from guardband import FILLS, GuardArena
from test_rotate_cpu import rotate_reference

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ORDERS = list(itertools.permutations(range(4)))
SMALL = [(5, 7), (37, 53), (64, 16)]


# ---- the oracle: torch operations on the CPU ---------------------------------------------------------------------------------
def rgb2hsv(img_u8):
    x = img_u8.to(torch.float32) / 255.0
    r, g, b = x.unbind(0)
    maxc, minc = torch.max(x, dim=0).values, torch.min(x, dim=0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    return torch.fmod(h / 6.0 + 1.0, 1.0), s, maxc


def hsv2rgb_u8(h, s, v):
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32)
    p = torch.clamp(v * (1.0 - s), 0.0, 1.0)
    q = torch.clamp(v * (1.0 - s * f), 0.0, 1.0)
    t = torch.clamp(v * (1.0 - (s * (1.0 - f))), 0.0, 1.0)
    i = i % 6

    def pick(six):
        out = six[5]
        for k in (4, 3, 2, 1, 0):
            out = torch.where(i == k, six[k], out)
        return out
    rgb = torch.stack([pick((v, q, p, p, t, v)), pick((t, v, v, q, p, p)), pick((p, p, t, v, v, q))])
    return (rgb * 255.0).to(torch.uint8)


def hue_step(img_u8, factor, hsv=None):
    h, s, v = rgb2hsv(img_u8) if hsv is None else hsv
    return hsv2rgb_u8((h + factor) % 1.0, s, v)


def gray(img):
    r, g, b = img.unbind(0)
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(torch.uint8)


def blend(a, b, f):
    return (f * a + (1.0 - f) * b).clamp(0, 255).to(torch.uint8)


def jitter(img, p):
    """-> the jittered uint8 image and the int64 sum of gray() in front of the contrast step (0 without one)"""
    x, gsum = img, 0
    for s in p.order:
        if s == 3:
            if p.hue is not None:
                x = hue_step(x, p.hue)
            continue
        f = p.factors[s]
        if f is None:
            continue
        if s == 0:
            x = blend(x, torch.zeros_like(x), f)
        elif s == 1:
            g = gray(x)
            gsum = int(g.to(torch.int64).sum())
            x = blend(x, torch.tensor(gsum, dtype=torch.int64).to(torch.float32) / torch.tensor(g.numel(), dtype=torch.float32), f)
        else:
            x = blend(x, gray(x).unsqueeze(0), f)
    return x, gsum


def normalise(u8, p):
    mean, std = torch.tensor(p.mean, dtype=torch.float32), torch.tensor(p.std, dtype=torch.float32)
    return (u8.to(torch.float32) / 255 - mean[:, None, None]) / std[:, None, None]


def bits(t):
    return t.contiguous().view(torch.int32)


def images(seed, B, h, w):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, 3, h, w), dtype=torch.uint8, generator=g)
    img[:, :, 0, :] = img[:, :1, 0, :]                           # a row of greys (maxc == minc) ...
    img[:, 1, 1, :] = img[:, 0, 1, :]                            # ... and one of ties between two channels
    return img


# ---- rotate_nearest_u8 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL)
def test_rotate_equals_pillow(dev, shape):
    """ragged tiles (the kernel's is 64 x 4), W < 64, both fills, the mask"""
    from refign_amd import resample
    h, w = shape
    z = golden("rotate_pillow")
    img = torch.from_numpy(z[f"image_{h}x{w}"]).permute(2, 0, 1).contiguous().to(dev)
    lbl = torch.from_numpy(z[f"label_{h}x{w}"]).to(dev)
    touched = 0
    for k, a in enumerate(z["angles"].tolist()):
        got, outside = resample.rotate_nearest_u8(img, a, 0)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (3, h, w) and outside.dtype == torch.bool
        assert np.array_equal(got.permute(1, 2, 0).cpu().numpy(), z[f"rot_image_{h}x{w}"][k]), (shape, a)
        assert np.array_equal(outside.cpu().numpy(), z[f"rot_mask_{h}x{w}"][k]), (shape, a)
        got, outside = resample.rotate_nearest_u8(lbl, a, 255)
        assert tuple(got.shape) == (h, w) and np.array_equal(got.cpu().numpy(), z[f"rot_label_{h}x{w}"][k]), (shape, a)
        assert np.array_equal(outside.cpu().numpy(), z[f"rot_mask_{h}x{w}"][k]), (shape, a)
        touched += int(outside.any())
    assert touched > 0


@pytest.mark.parametrize("angle", [10.0, -10.0, 0.001])
def test_rotate_at_full_size(dev, angle):
    from refign_amd import resample
    rng = np.random.default_rng(3)
    img, lbl = rng.integers(0, 256, (720, 720, 3), dtype=np.uint8), rng.integers(0, 19, (720, 720), dtype=np.uint8)
    got, outside = resample.rotate_nearest_u8(torch.from_numpy(img).permute(2, 0, 1).contiguous().to(dev), angle, 0)
    want, mask = rotate_reference(img, angle, 0)
    assert np.array_equal(got.permute(1, 2, 0).cpu().numpy(), want) and np.array_equal(outside.cpu().numpy(), mask)
    got, outside = resample.rotate_nearest_u8(torch.from_numpy(lbl).to(dev), angle, 255)
    want, mask = rotate_reference(lbl, angle, 255)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(outside.cpu().numpy(), mask)
    assert mask.any() == (abs(angle) > 1)


def test_rotate_by_zero_and_the_refusals(dev):
    from refign_amd import resample
    img = images(0, 1, 19, 70)[0].to(dev)
    for a in (0.0, 360.0, -720.0):
        got, outside = resample.rotate_nearest_u8(img, a, 7)
        assert torch.equal(got, img) and got.data_ptr() != img.data_ptr() and not bool(outside.any())
    for a in (90, 180.0, 270, -90.0):
        with pytest.raises(ValueError, match="transpose"):
            resample.rotate_nearest_u8(img, a, 0)
    with pytest.raises(RuntimeError, match="device tensors"):
        resample.rotate_nearest_u8(img.cpu(), 3.0, 0)
    for bad in (img.float(), img[:2], img.unsqueeze(0), img[:, :, ::2]):
        with pytest.raises(RuntimeError, match="uint8"):
            resample.rotate_nearest_u8(bad, 3.0, 0)
    with pytest.raises(ValueError, match="fill"):
        resample.rotate_nearest_u8(img, 3.0, 256)
    with pytest.raises(ValueError, match="3 x 40000"):
        resample.rotate_nearest_u8(torch.zeros(3, 40000, dtype=torch.uint8, device=dev), 3.0, 0)


# ---- the hue step alone ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def every_colour():
    """one 4096 x 4096 image holding every RGB triple, and its (h, s, v), which does not depend on the factor"""
    idx = torch.arange(1 << 24, dtype=torch.int32)
    img = torch.stack([idx >> 16, (idx >> 8) & 255, idx & 255]).to(torch.uint8).view(3, 4096, 4096)
    return img, rgb2hsv(img)


@pytest.mark.parametrize("factor", [-0.1, 0.1, 0.5])
def test_hue_of_every_colour(dev, every_colour, factor):
    """mean 0 and std 1 leave u8 / 255, which names its uint8 value: bit-equal fp32 is the bit-equal uint8 result, no pixel left out"""
    from refign_amd import photometric
    img, hsv = every_colour
    p = photometric.params_from([3, 0, 1, 2], None, None, None, [0, 1, 2], None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), hue=factor)
    got = photometric.apply(img.to(dev), p).cpu()[0]
    want = hue_step(img, p.hue, hsv)
    assert not torch.equal(want, img)
    back = torch.round(got * 255.0).to(torch.uint8)
    assert torch.equal(bits(got), bits(back.to(torch.float32) / 255)), "an output value that no grey level gives"
    diff = (back != want).any(0)
    assert not bool(diff.any()), (factor, int(diff.sum()), img[:, diff][:, :4].tolist(), back[:, diff][:, :4].tolist(),
                                  want[:, diff][:, :4].tolist())


# ---- hue inside the chain ----------------------------------------------------------------------------------------------------
def chain_params(hue=True):
    """one parameter set per order: both ends of the section's ranges in every pairing, contrast absent in every third"""
    from refign_amd import photometric
    out = []
    for i, order in enumerate(ORDERS):
        kw = dict(hue=(-0.1, 0.1)[(i // 3) % 2]) if hue else {}
        out.append(photometric.params_from(order, (0.75, 1.25)[i % 2], (1.25, 0.75, None)[i % 3], (0.75, 1.25)[(i // 2) % 2],
                                           [0, 1, 2], None, mean=MEAN, std=STD, **kw))
    return out


def test_hue_in_every_order(dev):
    from refign_amd import photometric
    h, w = 16, 20
    assert 255 * h * w < 2 ** 24
    params = chain_params()
    seen = {(p.order.index(3) < p.order.index(1), p.hue) for p in params if p.contrast is not None}
    assert seen == {(True, -0.1), (True, 0.1), (False, -0.1), (False, 0.1)}, "hue in front of and behind contrast, both ends"
    assert {(p.brightness, p.saturation) for p in params} == set(itertools.product((0.75, 1.25), repeat=2))
    imgs = images(0, len(params), h, w)
    d = imgs.to(dev)
    got, sums = photometric.apply(d, params).cpu(), photometric.gray_sums(d, params).cpu().tolist()
    for b, p in enumerate(params):
        x, gsum = jitter(imgs[b], p)
        assert sums[b] == gsum, (p.order, sums[b], gsum)
        assert torch.equal(bits(got[b]), bits(normalise(x, p))), (p.order, p.hue, int((got[b] != normalise(x, p)).sum()))
    # the mean pass applied the hue step where the order puts it in front of contrast: there it changes the sum
    moved = [b for b, p in enumerate(params) if p.contrast is not None and p.order.index(3) < p.order.index(1) and
             jitter(imgs[b], photometric.params_from(p.order, p.brightness, p.contrast, p.saturation, [0, 1, 2], None))[1] != sums[b]]
    assert moved


def test_without_hue_nothing_changes(dev):
    """hue=None: the chain as it was -- the oracle without the step, and params_from called as before the keyword existed"""
    from refign_amd import photometric
    params = chain_params(hue=False)
    assert all(p.hue is None and p.record()[7] == 0 and p.record()[73] == 0 for p in params)
    imgs = images(1, len(params), 16, 20)
    got = photometric.apply(imgs.to(dev), params).cpu()
    same = photometric.apply(imgs.to(dev), [photometric.params_from(p.order, *p.factors, [0, 1, 2], None, mean=MEAN, std=STD)
                                            for p in params]).cpu()
    assert torch.equal(bits(got), bits(same))
    for b, p in enumerate(params):
        assert torch.equal(bits(got[b]), bits(normalise(jitter(imgs[b], p)[0], p))), p.order


# ---- the fused pass ----------------------------------------------------------------------------------------------------------
def composed(d, params, geometry):
    """rotate_nearest_u8 -> slice -> apply -> mirror -> zero under the mask, per sample, from the pieces tested above"""
    from refign_amd import photometric, resample
    outs, sums = [], []
    for b, (p, g) in enumerate(zip(params, geometry)):
        rot, outside = resample.rotate_nearest_u8(d[b], g.angle, 0)
        box = (slice(g.top, g.top + g.h), slice(g.left, g.left + g.w))
        crop = rot[:, box[0], box[1]].contiguous()
        out, mask = photometric.apply(crop, p)[0], outside[box]
        if g.flip:
            out, mask = out.flip(-1), mask.flip(-1)
        outs.append(torch.where(mask, torch.zeros((), device=d.device), out))
        sums.append(photometric.gray_sums(crop, p)[0])
    return torch.stack(outs), torch.stack(sums), None


@pytest.mark.parametrize("shape,crop", [((37, 53), (24, 32)), ((720, 720), (512, 512))])
def test_fused_pass_equals_the_composition(dev, shape, crop):
    from refign_amd import photometric
    (H, W), (h, w) = shape, crop
    boxes = [(0, 0), (H - h, W - w), (0, W - w), ((H - h) // 2, (W - w) // 2)]
    geometry = [photometric.RotateCrop(a, *boxes[k], h, w, flip) for k, (a, flip) in
                enumerate(itertools.product((10.0, -10.0), (False, True)))]
    orders = [ORDERS[k] for k in (0, 9, 14, 23)]                  # hue behind and in front of contrast
    params = [photometric.params_from(o, (0.75, 1.25)[k % 2], (1.25, 0.75, 1.25, None)[k], 1.25, [0, 1, 2], None, mean=MEAN, std=STD,
                                      hue=(-0.1, 0.1)[k % 2]) for k, o in enumerate(orders)]
    d = images(2, 4, H, W).to(dev)
    got = photometric.apply(d, params, geometry=geometry)
    want, want_sums, _ = composed(d, params, geometry)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 3, h, w)
    assert torch.equal(bits(got), bits(want)), [int((got[b] != want[b]).sum()) for b in range(4)]
    assert torch.equal(photometric.gray_sums(d, params, geometry=geometry), want_sums) and int(want_sums[3]) == 0
    # exact 0.0 outside, in all three channels; the corner boxes do reach outside
    from refign_amd import resample
    n_outside = 0
    for b, g in enumerate(geometry):
        mask = resample.rotate_nearest_u8(d[b], g.angle, 0)[1][g.top:g.top + g.h, g.left:g.left + g.w]
        mask = mask.flip(-1) if g.flip else mask
        assert bool((bits(got[b])[:, mask] == 0).all()), b
        n_outside += int(mask.sum())
    assert n_outside > 0
    out = torch.empty_like(got)
    assert photometric.apply(d, params, out=out, geometry=geometry) is out and torch.equal(bits(out), bits(got))
    # one sample, one RotateCrop; angle 0 and the whole image: the plain call
    alone = photometric.apply(d[1], params[1], geometry=geometry[1])
    assert torch.equal(bits(alone[0]), bits(got[1]))
    whole = photometric.apply(d[0], params[0], geometry=photometric.RotateCrop(0.0, 0, 0, H, W, False))
    assert torch.equal(bits(whole), bits(photometric.apply(d[0], params[0])))


def test_fused_pass_refusals(dev):
    from refign_amd import photometric
    d = images(3, 2, 21, 30).to(dev)
    g = photometric.RotateCrop(5.0, 2, 3, 16, 20, False)
    plain = photometric.params_from([0, 1, 2, 3], 1.1, 0.9, 1.2, [0, 1, 2], None, hue=0.05)
    blurred = photometric.params_from([0, 1, 2, 3], 1.1, 0.9, 1.2, [0, 1, 2], 1.0)
    shuffled = photometric.params_from([0, 1, 2, 3], 1.1, 0.9, 1.2, [1, 0, 2], None)
    for bad in (blurred, shuffled):
        with pytest.raises(RuntimeError, match="blur"):
            photometric.apply(d, [plain, bad], geometry=[g, g])
        with pytest.raises(RuntimeError, match="blur"):
            photometric.gray_sums(d, [plain, bad], geometry=[g, g])
    with pytest.raises(RuntimeError, match="as many RotateCrop"):
        photometric.apply(d, [plain, plain], geometry=[g])
    with pytest.raises(RuntimeError, match="one crop size"):
        photometric.apply(d, [plain, plain], geometry=[g, photometric.RotateCrop(5.0, 2, 3, 16, 18, False)])
    with pytest.raises(RuntimeError, match="does not lie"):
        photometric.apply(d, [plain, plain], geometry=[g, photometric.RotateCrop(5.0, 6, 3, 16, 20, False)])
    with pytest.raises(ValueError, match="transpose"):
        photometric.apply(d, [plain, plain], geometry=[g, photometric.RotateCrop(90.0, 2, 3, 16, 20, False)])
    with pytest.raises(RuntimeError, match="out must"):
        photometric.apply(d, [plain, plain], out=torch.empty(2, 3, 21, 30, device=dev), geometry=[g, g])
    assert tuple(photometric.apply(d, [plain, plain], geometry=[g, g]).shape) == (2, 3, 16, 20)


# ---- RotatedLabelledSampler --------------------------------------------------------------------------------------------------
PLAN = {"dims": (72, 72), "crop_size": (48, 48), "cat_max_ratio": 0.75, "flip": 0.5, "mean": MEAN, "std": STD,
        "load_keys": ["image", "semantic"], "rotation": {"degrees": (-10.0, 10.0)},
        "jitter": {"brightness": (0.75, 1.25), "contrast": (0.75, 1.25), "saturation": (0.75, 1.25), "hue": (-0.1, 0.1),
                   "shuffle": False, "blur": None}}


def decoded_sample():
    rng = np.random.default_rng(11)
    coarse = rng.integers(0, 5, (8, 8), dtype=np.uint8)
    coarse[rng.random((8, 8)) < 0.6] = 2                         # a dominant class: RandomCrop re-draws
    lbl = np.repeat(np.repeat(coarse, 12, 0), 12, 1)
    lbl[rng.random((96, 96)) < 0.03] = 255
    return rng.integers(0, 256, (96, 96, 3), dtype=np.uint8), lbl


@pytest.mark.parametrize("seed", [3, 5])                         # (angles -9.9 and 6.6 degrees)
def test_sampler_equals_the_host_composition(dev, seed):
    from refign_amd import datastep, photometric, resample
    img, lbl = decoded_sample()
    lbl72 = resample.resize_nearest_reference(lbl, PLAN["dims"])
    # the recorded draw sequence, by hand, with the pixels of the label map on the host
    random.seed(seed)
    torch.manual_seed(seed)
    angle = float(torch.empty(1).uniform_(-10.0, 10.0).item())
    rot_lbl, _ = rotate_reference(lbl72, angle, 255)

    def host_hists(boxes):
        return np.stack([np.bincount(rot_lbl[t:t + h, l:l + w].reshape(-1), minlength=256) for t, l, h, w in boxes])
    (top, left, h, w), _ = datastep.draw_crop(72, 72, PLAN["crop_size"], 0.75, 255, host_hists)
    pp = photometric.draw(dict(PLAN["jitter"], mean=MEAN, std=STD))
    flip = random.random() < 0.5
    states = (random.getstate(), torch.get_rng_state())
    assert pp.hue is not None and abs(angle) > 5
    # the expected tensors from the pieces
    d72 = resample.resize_u8(torch.from_numpy(img).to(dev), PLAN["dims"])
    want_img, _, _ = composed(d72.unsqueeze(0), [pp], [photometric.RotateCrop(angle, top, left, h, w, flip)])
    want_lbl = rot_lbl[top:top + h, left:left + w]
    want_lbl = torch.from_numpy(np.ascontiguousarray(want_lbl[:, ::-1] if flip else want_lbl)).to(torch.int64)
    for hists in (host_hists, None):                             # an injected host counter, then the device counter
        sampler = datastep.RotatedLabelledSampler(lambda index: (img, lbl), PLAN, dev, hists=hists)
        random.seed(seed)
        torch.manual_seed(seed)
        out_img, out_lbl = sampler.sample(0)
        assert random.getstate() == states[0] and torch.equal(torch.get_rng_state(), states[1])
        assert out_img.dtype == torch.float32 and tuple(out_img.shape) == (3, 48, 48)
        assert out_lbl.dtype == torch.int64 and torch.equal(out_lbl.cpu(), want_lbl)
        assert torch.equal(bits(out_img), bits(want_img[0]))
    # into the slots of a batch
    slot_i, slot_l = torch.empty(2, 3, 48, 48, device=dev), torch.empty(2, 48, 48, dtype=torch.int64, device=dev)
    random.seed(seed)
    torch.manual_seed(seed)
    a, b = sampler.sample(0, slot_i[1], slot_l[1])
    assert a.data_ptr() == slot_i[1].data_ptr() and torch.equal(bits(slot_i[1]), bits(want_img[0])) and torch.equal(slot_l[1].cpu(), want_lbl)


# ---- guard band --------------------------------------------------------------------------------------------------------------
def test_guard_band(dev):
    """the new passes inside the poisoned arena: untouched guards, equal bits across the fills"""
    from refign_amd import photometric, resample
    imgs = images(8, 2, 37, 70)
    lbl = torch.randint(0, 19, (37, 70), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    params = [photometric.params_from(ORDERS[k], 1.25, 0.75, 1.25, [0, 1, 2], None, mean=MEAN, std=STD, hue=f)
              for k, f in ((3, 0.1), (20, -0.1))]
    geometry = [photometric.RotateCrop(10.0, 0, 0, 21, 66, False), photometric.RotateCrop(-10.0, 16, 4, 21, 66, True)]
    results = []
    for fill in FILLS:
        arena = GuardArena(dev, fill, 4 << 20, skew=1)
        placed, placed_lbl = arena.place(imgs.to(dev)), arena.place(lbl.to(dev))
        with arena.allocations():
            fused = photometric.apply(placed, params, geometry=geometry)
            sums = photometric.gray_sums(placed, params, geometry=geometry)
            hue = photometric.apply(placed, params)
            rot, outside = resample.rotate_nearest_u8(placed[0], 10.0, 0)
            rot_lbl, _ = resample.rotate_nearest_u8(placed_lbl, -10.0, 255)
        arena.check()
        assert torch.equal(placed.cpu(), imgs) and torch.equal(placed_lbl.cpu(), lbl), "the inputs are read only"
        results.append([t.cpu() for t in (fused, sums, hue, rot, outside, rot_lbl)])
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a, b) if a.dtype != torch.float32 else torch.equal(bits(a), bits(b))
    fused, sums, hue, rot, outside, rot_lbl = results[0]
    for b, p in enumerate(params):
        assert torch.equal(bits(hue[b]), bits(normalise(jitter(imgs[b], p)[0], p)))
    want, mask = rotate_reference(imgs[0].permute(1, 2, 0).numpy(), 10.0, 0)
    assert np.array_equal(rot.permute(1, 2, 0).numpy(), want) and np.array_equal(outside.numpy(), mask)
    assert np.array_equal(rot_lbl.numpy(), rotate_reference(lbl.numpy(), -10.0, 255)[0])
    want_fused, want_sums, _ = composed(imgs.to(dev), params, geometry)
    assert torch.equal(bits(fused), bits(want_fused.cpu())) and torch.equal(sums, want_sums.cpu())

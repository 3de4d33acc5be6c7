"""tests/golden/make_golden_flowsynth.py -- goldens of the matcher's warp supervision: the reference's own CompositeFlow and
Random* classes (data_modules/transforms.py:573-1395) and helpers.matching_utils run on a 248 x 272 frame, followed by the
centre crop to 203 x 224 (torchvision's center_crop origin, int(round((H - h) / 2.0)): (22, 24)).  The reference's modules are
imported as make_golden_data.py imports them (_ref_import + its stubs()).

cv2 is not installed.  The one cv2 call on this path, cv2.GaussianBlur(src, (0, 0), sigma, dst=src) in elastic_transform, is
replaced by a STAND-IN for third-party arithmetic: the formula OpenCV documents (round(sigma * 8 + 1) | 1 taps of
exp(-x^2 / 2 sigma^2) computed in double, normalised, stored as float32; separable; BORDER_REFLECT_101) through
scipy.ndimage.correlate1d(mode="mirror") in float64, rounded once.  The elastic cases store the field elastic_transform
RETURNED (blurred and scaled), and the device test feeds that field in: a case's result does not depend on whose blur made it.

What the reference drew is recorded at the calls it makes (random.choice / randint / random, torch.bmm's results -- the
homography's h and the spline's W_X, W_Y, A_X, A_Y --, affine_grid's theta, elastic_transform's arguments and result).
`ref_err`: the same mapping evaluated in float64 from the same parameters with the reference's formulas (`flow64`), against the
reference's float32 flow, over the crop's pixels that are sentinel on neither side; the device test derives its tolerance from it.
    python tests/golden/make_golden_flowsynth.py      ->  flowsynth_<case>.npz"""
import math
import os
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from fill import hashed_uniform  # noqa: E402

H, W, CROP = 248, 272, (203, 224)
SEED = 3
AMPLITUDES = dict(random_alpha=0.26, random_s=0.45, random_tx=0.25, random_ty=0.25, random_t_hom=0.4, random_t_tps=0.4,
                  random_t_tps_for_afftps=0.26)
KINDS = ("hom", "affine", "tps", "afftps")
# name -> (include_transforms, add_elastic)
CASES = {"hom": (["hom"], False), "hom_elastic": (["hom"], True), "tps": (["tps"], False), "tps_elastic": (["tps"], True),
         "afftps": (["afftps"], False), "afftps_elastic": (["afftps"], True), "affine": (["affine"], False)}
BATCH_INCLUDE = ["hom", "afftps"]
FALLBACK_THETA = [[1.0, 0.0, 1.4], [0.0, 1.0, 1.4]]       # a shift of 0.7 of the frame both ways: 0.3 x 0.3 < 10 % stays valid
ALL_CASES = tuple(CASES) + ("fallback", "batch")


def image_in(tag="img"):
    """the normalised input image (3, H, W), not stored"""
    return (hashed_uniform((3, H, W), "flowsynth/" + tag) * 2.0 - 1.0).astype(np.float32)


def crop_origin():
    return int(round((H - CROP[0]) / 2.0)), int(round((W - CROP[1]) / 2.0))


def crop(a):
    top, left = crop_origin()
    return a[..., top:top + CROP[0], left:left + CROP[1]]


def opencv_taps(sigma):
    n = int(round(sigma * 8 + 1)) | 1
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2
    k = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (k / k.sum()).astype(np.float32)


def gaussian_blur_standin(src, ksize, sigma, dst=None):
    from scipy.ndimage import correlate1d
    assert tuple(ksize) == (0, 0) and src.dtype == np.float32
    k = opencv_taps(float(sigma)).astype(np.float64)
    out = correlate1d(correlate1d(src.astype(np.float64), k, axis=1, mode="mirror"), k, axis=0, mode="mirror").astype(np.float32)
    if dst is not None:
        dst[...] = out
        return dst
    return out


class Recorder:
    """wraps the calls at which the reference's draws and small results become visible; restores them on exit"""

    def __init__(self, tr):
        self.tr, self.log = tr, {"choice": [], "randint": [], "random": [], "bmm": [], "affine": [], "elastic": []}

    def __enter__(self):
        tr, log = self.tr, self.log
        self.saved = (random.choice, random.randint, random.random, torch.bmm, F.affine_grid, tr.elastic_transform)

        def choice(seq, _f=random.choice):
            v = _f(seq)
            log["choice"].append([i for i, m in enumerate(seq) if m is v][0])
            return v

        def randint(a, b, _f=random.randint):
            v = _f(a, b)
            log["randint"].append(v)
            return v

        def rnd(_f=random.random):
            v = _f()
            log["random"].append(v)
            return v

        def bmm(a, b, _f=torch.bmm):
            v = _f(a, b)
            log["bmm"].append(v.detach().clone().reshape(-1))
            return v

        def affine_grid(theta, size, align_corners=None, _f=F.affine_grid):
            log["affine"].append(theta.detach().clone().reshape(6))
            return _f(theta, size, align_corners=align_corners)

        def elastic(shape, sigma, alpha, **kw):
            dx, dy = self.saved[5](shape, sigma, alpha, **kw)
            log["elastic"].append((float(sigma), float(alpha), torch.stack([dx, dy]).clone()))
            return dx, dy

        random.choice, random.randint, random.random, torch.bmm = choice, randint, rnd, bmm
        F.affine_grid = torch.nn.functional.affine_grid = affine_grid
        tr.elastic_transform = elastic
        return self

    def __exit__(self, *exc):
        random.choice, random.randint, random.random, torch.bmm, F.affine_grid, self.tr.elastic_transform = self.saved
        torch.nn.functional.affine_grid = self.saved[4]
        return False


def theta39_of(kind, log, start_bmm=0, start_aff=0):
    t = np.zeros(39, np.float32)
    if kind == "hom":
        t[:8], t[8] = log["bmm"][start_bmm].numpy(), 1.0
    if kind in ("tps", "afftps"):
        t[9:33] = np.concatenate([v.numpy() for v in log["bmm"][start_bmm:start_bmm + 4]])
    if kind in ("affine", "afftps"):
        t[33:] = log["affine"][start_aff].numpy()
    return t


def bumps_of(drawn):
    """the bump list the kernel takes, (x, y, sigma, 2 / mask.max()), from the FULL 2-D mask as get_params forms it"""
    out = []
    for s, x, y in drawn:
        sig2 = 2 * s * s
        g1 = torch.exp(-(torch.arange(0, H) - x) ** 2 / sig2)
        g2 = torch.exp(-(torch.arange(0, W) - y) ** 2 / sig2)
        m = (torch.outer(g1, g2) / (s * math.sqrt(2 * math.pi) ** 2)).max()
        if m < 1e-6:
            continue
        out.append((float(x), float(y), float(s), float(2.0 / m)))
    return np.array(out, np.float32).reshape(-1, 4)


def flow64(tr, kind, theta39, field=None, bumps=None):
    """the case's flow (2, H, W) in float64 from the float32 parameters, with the reference's formulas"""
    t = torch.from_numpy(theta39.astype(np.float64))
    gx = torch.linspace(-1, 1, W, dtype=torch.float64).view(1, W).expand(H, W)
    gy = torch.linspace(-1, 1, H, dtype=torch.float64).view(H, 1).expand(H, W)

    def tps():
        X, Y = t[27] + t[28] * gx + t[29] * gy, t[30] + t[31] * gx + t[32] * gy
        for k in range(9):
            d = (gx - (k // 3 - 1)) ** 2 + (gy - (k % 3 - 1)) ** 2
            d = torch.where(d == 0, torch.ones_like(d), d)
            u = d * torch.log(d)
            X, Y = X + t[9 + k] * u, Y + t[18 + k] * u
        return torch.stack([X, Y], -1).unsqueeze(0)

    def aff():
        return F.affine_grid(t[33:].view(1, 2, 3), [1, 3, H, W], align_corners=False)

    if kind == "hom":
        k = gx * t[6] + gy * t[7] + t[8]
        grid = torch.stack([(gx * t[0] + gy * t[1] + t[2]) / k, (gx * t[3] + gy * t[4] + t[5]) / k], -1).unsqueeze(0)
    elif kind == "tps":
        grid = tps()
    elif kind == "affine":
        grid = aff()
    else:
        grid = tr.RandomAffineTPS.get_params(aff(), tps())       # dtype-generic: runs in float64 as given
    mp = grid.permute(0, 3, 1, 2)
    xx = torch.arange(W, dtype=torch.float64).view(1, W).expand(H, W)
    yy = torch.arange(H, dtype=torch.float64).view(H, 1).expand(H, W)
    mapping = torch.stack([(mp[0, 0] + 1) * (W - 1) / 2.0, (mp[0, 1] + 1) * (H - 1) / 2.0])
    if field is not None:
        mask = torch.zeros(H, W, dtype=torch.float64)
        for x, y, s, scale in bumps.astype(np.float64):
            g1 = torch.exp(-(torch.arange(H, dtype=torch.float64) - x) ** 2 / (2 * s * s))
            g2 = torch.exp(-(torch.arange(W, dtype=torch.float64) - y) ** 2 / (2 * s * s))
            mask = mask + torch.clamp(scale * torch.outer(g1, g2) / (s * 2 * math.pi), 0.0, 1.0)
        pert = torch.from_numpy(field.astype(np.float64)) * torch.clamp(mask, 0.0, 1.0)
        vx, vy = 2.0 * (xx + pert[0]) / (W - 1) - 1.0, 2.0 * (yy + pert[1]) / (H - 1) - 1.0
        mapping = F.grid_sample(mapping.unsqueeze(0), torch.stack([vx, vy], -1).unsqueeze(0), align_corners=True)[0]
    return torch.stack([mapping[0] - xx, mapping[1] - yy]).numpy()


def sample_arrays(tr, mu, kind, theta39, out, field=None, drawn=None, with_image=True):
    """what one sample stores: the parameters and the reference's cropped outputs; `out` = (image, flow, mask) of the full frame"""
    image, flow, mask = (v.detach() for v in out)
    flow = flow.reshape(2, H, W)
    border = mu.create_border_mask(flow)
    warp_mask = tr.warp(torch.from_numpy(image_in()).unsqueeze(0), flow.unsqueeze(0), padding_mode="zeros", return_mask=True)[1][0]
    bumps = bumps_of(drawn) if drawn is not None else np.zeros((0, 4), np.float32)
    f64 = flow64(tr, kind, theta39, None if field is None else field.numpy(), bumps)
    f32 = flow.numpy()
    ok = (np.abs(f32) <= 1e4).all(0) & (np.abs(f64) <= 1e4).all(0)
    ref_err = float(np.abs(crop(f32).astype(np.float64) - crop(f64))[:, crop(ok)].max())
    arrays = dict(kind=np.int64(KINDS.index(kind)), theta39=theta39, flow=crop(f32).copy(), mask=crop(mask.reshape(H, W).numpy()).copy(),
                  border_mask=crop(border.numpy()).copy(), warp_mask=crop(warp_mask.numpy()).copy(),
                  border_count=np.int64(int(border.sum())), ref_err=np.float64(ref_err), bumps=bumps)
    if field is not None:
        arrays["field"] = field.numpy().copy()
        arrays["drawn"] = np.array(drawn, np.int64).reshape(-1, 3)
    if with_image:
        arrays["image"] = crop(image.reshape(3, H, W).numpy()).copy()
    frac = float(mask.float().mean())
    sent = float((np.abs(f32) > 1e4).any(0).mean())
    print(f"    {kind:7s} valid {frac:.3f}  border {int(border.sum()) / (H * W):.3f}  sentinel {sent:.4f}  ref_err {ref_err:.3e} px")
    return arrays


def save(name, **arrays):
    path = os.path.join(HERE, "flowsynth_" + name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrays.items()})
    size = os.path.getsize(path)
    print(f"  wrote flowsynth_{name}.npz  ({size / 1000:.1f} kB)")
    return size


def tails():
    return dict(random_tail=np.array([random.random() for _ in range(4)]), torch_tail=torch.rand(4).numpy())


def run_case(tr, mu, name, include, add_elastic, seed=SEED, n=1):
    cf = tr.CompositeFlow(apply_keys=["image_prime"], include_transforms=include, add_elastic=add_elastic, **AMPLITUDES)
    random.seed(seed)
    torch.manual_seed(seed)
    samples = []
    with Recorder(tr) as rec:
        for i in range(n):
            nb, na, ne, nr, nq = (len(rec.log[k]) for k in ("bmm", "affine", "elastic", "randint", "random"))
            s = cf({"image_prime": torch.from_numpy(image_in("img" if n == 1 else f"img{i}"))})
            kind = include[rec.log["choice"][i]]
            field = drawn = None
            scal = {}
            if add_elastic:
                sigma, alpha, field = rec.log["elastic"][ne]
                ints = rec.log["randint"][nr:]
                drawn = [tuple(ints[1 + 3 * j:4 + 3 * j]) for j in range(ints[0])]
                scal = dict(n_perturbations=np.int64(ints[0]), sigma=np.float64(sigma), alpha=np.float64(alpha))
            a = sample_arrays(tr, mu, kind, theta39_of(kind, rec.log, nb, na), (s["image_prime"], s["image_prime_flow"],
                              s["image_prime_mask"]), field, drawn, with_image=False)
            a.update(scal, transform=np.int64(rec.log["choice"][i]))
            samples.append((a, s["image_prime"]))
        tail = tails()
    return samples, tail


def main():
    import _ref_import as R
    from make_golden_data import stubs
    R.setup()
    stubs()
    sys.modules["cv2"].GaussianBlur = gaussian_blur_standin
    tr = R.ref_module("data_modules.transforms")
    mu = R.ref_module("helpers.matching_utils")
    top, left = crop_origin()
    common = dict(size=np.array([H, W, *CROP]), origin=np.array([top, left]), seed=np.int64(SEED),
                  **{k: np.float64(v) for k, v in AMPLITUDES.items()})
    for name, (include, add_elastic) in CASES.items():
        samples, tail = run_case(tr, mu, name, include, add_elastic)
        a, image = samples[0]
        arrays = dict(common, include=np.array(include), add_elastic=np.bool_(add_elastic), **a, **tail)
        if not add_elastic:                                  # an elastic case's field alone is 540 kB: no room for the image
            arrays["image"] = crop(image.reshape(3, H, W).numpy()).copy()
        assert save(name, **arrays) < 1000000
    # fallback: an explicit shift that leaves < 10 % valid, through the reference's own apply_transform
    ra = tr.RandomAffine(apply_keys=["image_prime"], **{k: AMPLITUDES[k] for k in ("random_alpha", "random_s", "random_tx", "random_ty")})
    theta = torch.tensor(FALLBACK_THETA, dtype=torch.float32)
    grid = F.affine_grid(theta.view(1, 2, 3), [1, 3, H, W], align_corners=False)
    flow = mu.unnormalise_and_convert_mapping_to_flow(grid, output_channel_first=True)
    out = ra.apply_transform(torch.from_numpy(image_in()), flow)
    t39 = np.zeros(39, np.float32)
    t39[33:] = theta.reshape(6).numpy()
    a = sample_arrays(tr, mu, "affine", t39, out)
    # (the two masks describe the same region and differ on exact border hits only -- `>= 0` against `> -1`: here nowhere)
    assert a["border_count"] < 0.1 * H * W and (a["mask"] == a["border_mask"]).all()
    assert save("fallback", **dict(common, **a)) < 1000000
    # B = 2 mixing hom and afftps: the first seed from SEED on whose two choices differ
    seed = SEED
    while True:
        samples, tail = run_case(tr, mu, "batch", BATCH_INCLUDE, False, seed=seed, n=2)
        if {int(a["transform"]) for a, _ in samples} == {0, 1}:
            break
        seed += 1
    arrays = dict(common, include=np.array(BATCH_INCLUDE), add_elastic=np.bool_(False), **tail)
    arrays["seed"] = np.int64(seed)
    for i, (a, _) in enumerate(samples):
        arrays.update({f"s{i}_{k}": v for k, v in a.items()})
    assert save("batch", **arrays) < 1000000


if __name__ == "__main__":
    main()

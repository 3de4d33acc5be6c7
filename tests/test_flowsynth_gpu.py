"""GPU: the matcher's warp supervision (refign_amd/flowsynth.py, csrc/flowsynth.hip) against the reference's CompositeFlow +
CenterCrop on a 248 x 272 frame cropped to 203 x 224 (tests/golden/flowsynth_*.npz, tests/golden/make_golden_flowsynth.py).

Bounds.  tol_flow = max(4 * ref_err, 1e-4) px per case: ref_err is the reference's own float32 error against a float64
evaluation of the same mapping (stored by the generator); the factor 4 covers a different operation order and the device's log.
Sentinel pixels: the reference's |flow| > 1e4 (the -1e10 out-of-bounds marker of the affine-TPS composition, whole or blended);
there the device's component must exceed 1e3 in magnitude with the reference's sign.  Mismatches -- a pixel that is sentinel on
one side only, or a mask that differs -- are capped at 0.1 % of the crop; a mask mismatch must lie where the reference's
sampling position is within tol_flow of the decision boundary (0 or n - 1).  The full-frame count is held to the same number of
pixels.  Image: tol_flow * G + 1e-5 on non-sentinel pixels, G the largest finite difference of the zero-padded input.
Blur: 2^-22 * max |oracle| against a float64 numpy restatement (one rounding to fp32, a factor 2 for the float32 taps).
Every figure is printed before it is asserted (pytest -s): profiles/flowsynth_parity.txt."""
import random

import numpy as np
import pytest
import torch
from conftest import golden
from make_golden_flowsynth import AMPLITUDES, CASES, CROP, H, KINDS, W, image_in

pytestmark = pytest.mark.gpu

TOP, LEFT = 22, 24
CAP = int(0.001 * CROP[0] * CROP[1])                       # mismatching pixels allowed in a crop: 45
SINGLES = list(CASES) + ["fallback"]


def params_of(z, prefix=""):
    from refign_amd import flowsynth
    g = lambda k: z[prefix + k]  # noqa: E731
    field = torch.from_numpy(g("field")) if prefix + "field" in z else None
    return flowsynth.params_from(KINDS[int(g("kind"))], H, W, theta39=g("theta39"), field=field,
                                 bumps=[tuple(b) for b in g("bumps").tolist()] if field is not None else ())


def reference_warp(image, flow_crop):
    """helpers.matching_utils.warp(image, flow, 'zeros') on the crop's pixels, restated with torch's CPU grid_sample: the grid
    is the FULL frame's, so the crop's pixel (i, j) samples at (j + LEFT + fx, i + TOP + fy)"""
    ch, cw = flow_crop.shape[-2:]
    xx = torch.arange(LEFT, LEFT + cw, dtype=torch.float32).view(1, -1).repeat(ch, 1)
    yy = torch.arange(TOP, TOP + ch, dtype=torch.float32).view(-1, 1).repeat(1, cw)
    f = torch.from_numpy(flow_crop)
    vx = 2.0 * (xx + f[0]) / float(W - 1) - 1.0
    vy = 2.0 * (yy + f[1]) / float(H - 1) - 1.0
    grid = torch.stack([vx, vy], -1).unsqueeze(0)
    return torch.nn.functional.grid_sample(torch.from_numpy(image).unsqueeze(0), grid, align_corners=True,
                                           padding_mode="zeros")[0].numpy()


def gradient_bound(image):
    p = np.pad(image.astype(np.float64), ((0, 0), (1, 1), (1, 1)))
    return float(max(np.abs(np.diff(p, axis=1)).max(), np.abs(np.diff(p, axis=2)).max()))


_RUNS = {}


def run_single(dev, name, prefix=""):
    """(z, device outputs as numpy) of one fixture sample, synthesized alone; computed once and shared"""
    from refign_amd import flowsynth
    key = name + prefix
    if key not in _RUNS:
        z = golden("flowsynth_" + name)
        tag = "img" if not prefix else "img" + prefix[1]
        image = image_in(tag)
        p = params_of(z, prefix)
        x = torch.from_numpy(image).to(dev)
        img, flow, mask, count = flowsynth.synthesize(x, p, crop=CROP, return_count=True)
        border = flowsynth.synthesize(x, p, crop=CROP, min_fraction_valid_corr=2.0)[2]       # fraction 2: always the fallback
        warpm = flowsynth.synthesize(x, p, crop=CROP, min_fraction_valid_corr=-1.0)[2]       # never
        _RUNS[key] = (z, image, (img, flow, mask), dict(img=img[0].cpu().numpy(), flow=flow[0].cpu().numpy(),
                      mask=mask[0].cpu().numpy(), border=border[0].cpu().numpy(), warp=warpm[0].cpu().numpy(),
                      count=int(count[0])))
    return _RUNS[key]


def check_sample(z, image, got, label, prefix=""):
    g = lambda k: z[prefix + k]  # noqa: E731
    R, D = g("flow").astype(np.float64), got["flow"].astype(np.float64)
    tol = max(4.0 * float(g("ref_err")), 1e-4)
    sent_ref, sent_dev = (np.abs(R) > 1e4).any(0), (np.abs(D) > 1e3).any(0)
    one_sided = sent_ref != sent_dev
    plain = ~sent_ref & ~sent_dev
    err = float(np.abs(D - R)[:, plain].max())
    big = (np.abs(R) > 1e4) & (sent_ref & sent_dev)[None]
    sent_ok = bool(((np.abs(D) > 1e3) & (np.sign(D) == np.sign(R)))[big].all())
    # the reference's sampling position in pixels, and its distance to the nearer decision boundary of either axis
    mx = R[0] + np.arange(LEFT, LEFT + CROP[1])[None, :]
    my = R[1] + np.arange(TOP, TOP + CROP[0])[:, None]
    dist = np.minimum(np.minimum(np.abs(mx), np.abs(mx - (W - 1))), np.minimum(np.abs(my), np.abs(my - (H - 1))))
    mism = {"border": got["border"] != g("border_mask"), "warp": got["warp"] != g("warp_mask"), "mask": got["mask"] != g("mask")}
    total = one_sided.copy()
    far = 0
    for m in mism.values():
        total |= m
        far += int((m & ~(dist <= tol)).sum())
    dcount = abs(got["count"] - int(g("border_count")))
    expected = g("image") if prefix + "image" in z else reference_warp(image, g("flow"))
    G = gradient_bound(image)
    img_err = float(np.abs(got["img"].astype(np.float64) - expected)[:, plain].max())
    img_tol = tol * G + 1e-5
    print(f"\nflowsynth parity {label:16s} flow err {err:.3e} px (tol {tol:.3e}, ref_err {float(g('ref_err')):.3e})  sentinel px "
          f"{int(sent_ref.sum())} one-sided {int(one_sided.sum())}  mask mismatches border/warp/final "
          f"{int(mism['border'].sum())}/{int(mism['warp'].sum())}/{int(mism['mask'].sum())} (cap {CAP}, away from a boundary {far})  "
          f"count diff {dcount}  image err {img_err:.3e} (tol {img_tol:.3e}, G {G:.3f})")
    assert err <= tol
    assert sent_ok
    assert int(total.sum()) <= CAP and far == 0
    assert dcount <= CAP
    assert img_err <= img_tol
    assert got["mask"].dtype == np.bool_ and got["flow"].dtype == np.float32 and got["img"].dtype == np.float32


@pytest.mark.parametrize("case", SINGLES)
def test_case_matches_the_reference(dev, case):
    z, image, _, got = run_single(dev, case)
    check_sample(z, image, got, case)
    if case == "fallback":                                  # < 10 % of the frame valid: the returned mask is the border mask
        assert got["count"] < 0.1 * H * W
        np.testing.assert_array_equal(got["mask"], got["border"])
    else:
        np.testing.assert_array_equal(got["mask"], got["warp"])


def test_batch_equals_its_samples_alone(dev):
    from refign_amd import flowsynth
    singles = [run_single(dev, "batch", f"s{i}_") for i in range(2)]
    z = singles[0][0]
    assert {KINDS[int(z[f"s{i}_kind"])] for i in range(2)} == {"hom", "afftps"}
    for i, (_, image, _, got) in enumerate(singles):
        check_sample(z, image, got, f"batch[{i}]", f"s{i}_")
    x = torch.from_numpy(np.stack([image_in("img0"), image_in("img1")])).to(dev)
    out = flowsynth.synthesize(x, [params_of(z, "s0_"), params_of(z, "s1_")], crop=CROP)
    assert tuple(out[0].shape) == (2, 3, *CROP) and tuple(out[1].shape) == (2, 2, *CROP) and tuple(out[2].shape) == (2, *CROP)
    for i, (_, _, alone, _) in enumerate(singles):
        for a, b in zip(out, alone):
            assert a.dtype == b.dtype and torch.equal(a[i], b[0])        # (no NaN in these flows: equal is bit-equal)


def test_rectangular_crop_origin(dev):
    """(248 - 203) / 2 = 22.5 rounds to 22 (half to even), (272 - 224) / 2 = 24: the crop is the full-frame result at (22, 24)"""
    from refign_amd import flowsynth
    z, image, cropped, _ = run_single(dev, "tps_elastic")
    assert tuple(int(v) for v in z["origin"]) == (TOP, LEFT) == flowsynth.crop_origin(H, W, *CROP)
    full = flowsynth.synthesize(torch.from_numpy(image).to(dev), params_of(z))
    assert tuple(full[1].shape) == (1, 2, H, W)
    for a, b in zip(full, cropped):
        assert torch.equal(a[..., TOP:TOP + CROP[0], LEFT:LEFT + CROP[1]], b)


def blur_oracle(src, sigma):
    """cv2.GaussianBlur(src, (0, 0), sigma) as OpenCV documents it, in float64: the float32 taps, BORDER_REFLECT_101 by
    folding the index with period 2(n - 1)"""
    n = int(round(sigma * 8 + 1)) | 1
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2
    k = np.exp(-(x * x) / (2.0 * sigma * sigma))
    k = (k / k.sum()).astype(np.float32).astype(np.float64)

    def fold(i, m):
        r = np.mod(i, 2 * (m - 1))
        return np.where(r < m, r, 2 * (m - 1) - r)

    def along(a, axis):
        m = a.shape[axis]
        idx = fold(np.arange(m)[:, None] + np.arange(n)[None, :] - n // 2, m)         # (m, n)
        return np.tensordot(np.take(a, idx, axis=axis), k, axes=([axis + 1], [0]))
    return along(along(src.astype(np.float64), 1), 0)


@pytest.mark.parametrize("h,w,sigma", [(64, 80, 9.0), (40, 100, 18.0)])
def test_blur_matches_the_float64_oracle(dev, h, w, sigma):
    from fill import hashed_uniform
    from refign_amd import flowsynth
    assert (h, sigma) != (40, 18.0) or (int(round(sigma * 8 + 1)) | 1) // 2 == 72 > h   # repeated reflection happens
    src = (hashed_uniform((2, h, w), f"flowsynth/blur{h}") * 2.0 - 1.0).astype(np.float32)
    got = flowsynth.gaussian_blur_f32(torch.from_numpy(src).to(dev), sigma).cpu().numpy()
    one = flowsynth.gaussian_blur_f32(torch.from_numpy(src[1]).to(dev), sigma).cpu().numpy()
    want = np.stack([blur_oracle(src[0], sigma), blur_oracle(src[1], sigma)])
    err, bound = float(np.abs(got.astype(np.float64) - want).max()), 2.0 ** -22 * float(np.abs(want).max())
    print(f"\nflowsynth parity blur {h} x {w} sigma {sigma}: err {err:.3e} (bound {bound:.3e})")
    assert got.dtype == np.float32 and err <= bound
    np.testing.assert_array_equal(one, got[1])


def test_warp_supervision_end_to_end(dev):
    """the stage-2 recipe from the draws to the batch: under the hom_elastic fixture's seeds the drawn noise, blurred on the
    device and scaled, is the fixture's field (made by the generator's float64 stand-in: one rounding each side plus the fp32
    product, 2^-21 max |field|), and the batch's flow is the fixture's within tol_flow plus that field error carried through a
    mapping whose slope stays below 4 at these amplitudes"""
    from refign_amd import flowsynth
    z = golden("flowsynth_hom_elastic")
    plan = {"composite": dict(AMPLITUDES, include_transforms=["hom"], add_elastic=True), "crop": CROP,
            "min_fraction_valid_corr": 0.1}
    image = torch.from_numpy(image_in()).to(dev)
    sample = {"image": image.unsqueeze(0) * 0.5, "image_ref": image.unsqueeze(0) * 0.25, "image_prime": image.unsqueeze(0)}
    random.seed(int(z["seed"]))
    torch.manual_seed(int(z["seed"]))
    batch = flowsynth.WarpSupervision(plan)(sample)
    np.testing.assert_array_equal(np.array([random.random() for _ in range(4)]), z["random_tail"])
    assert set(batch) == {"image_ref", "image_trg", "image_prime", "flow_prime", "mask_prime", "prime_trg_idx"}
    assert tuple(batch["flow_prime"].shape) == (1, 2, *CROP) and batch["mask_prime"].dtype == torch.bool
    assert torch.equal(batch["image_trg"], sample["image"][..., TOP:TOP + CROP[0], LEFT:LEFT + CROP[1]])
    assert torch.equal(batch["image_ref"], sample["image_ref"][..., TOP:TOP + CROP[0], LEFT:LEFT + CROP[1]])
    random.seed(int(z["seed"]))
    torch.manual_seed(int(z["seed"]))
    p = flowsynth.draw_composite(H, W, **plan["composite"])
    field = flowsynth.elastic_field(p, dev).cpu().numpy()
    ferr, fbound = float(np.abs(field.astype(np.float64) - z["field"]).max()), 2.0 ** -21 * float(np.abs(z["field"]).max())
    tol = max(4.0 * float(z["ref_err"]), 1e-4) + 4.0 * fbound
    err = float(np.abs(batch["flow_prime"][0].cpu().numpy().astype(np.float64) - z["flow"]).max())
    print(f"\nflowsynth parity end to end: field err {ferr:.3e} (bound {fbound:.3e})  flow err {err:.3e} px (tol {tol:.3e})")
    assert ferr <= fbound and err <= tol


def test_entry_points_refuse_bad_arguments(dev):
    from refign_amd import _lib, flowsynth
    from refign_amd._tensor import ptr
    import ctypes
    x = torch.zeros(3, 8, 8, device=dev)
    flow, count = torch.zeros(2, 8, 8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    theta, bumps = (ctypes.c_float * 39)(), (ctypes.c_float * 56)()
    with pytest.raises(RuntimeError, match="null"):
        _lib.call("rfn_flowsynth_flow_f32", dev, theta, 0, bumps, 0, None, 8, 8, None, ptr(count))
    with pytest.raises(RuntimeError, match="bumps"):
        _lib.call("rfn_flowsynth_flow_f32", dev, theta, 0, bumps, 14, ptr(flow), 8, 8, ptr(flow), ptr(count))
    with pytest.raises(RuntimeError, match=">= 2"):
        _lib.call("rfn_flowsynth_flow_f32", dev, theta, 0, bumps, 0, None, 1, 8, ptr(flow), ptr(count))
    out_i, out_m = torch.zeros(3, 8, 8, device=dev), torch.zeros(8, 8, dtype=torch.bool, device=dev)
    with pytest.raises(RuntimeError, match="crop"):
        _lib.call("rfn_flowsynth_warp_f32", dev, ptr(x), ptr(flow), ptr(count), 8, 8, 0, 0, 9, 8, 0.1, ptr(out_i), ptr(flow), ptr(out_m))
    with pytest.raises(RuntimeError, match="null"):
        _lib.call("rfn_gaussian_blur_f32", dev, ptr(x), None, 3, 3, 8, 8, ptr(flow), ptr(out_i))
    with pytest.raises(RuntimeError, match="crop"):
        flowsynth.synthesize(x, flowsynth.params_from("affine", 8, 8, theta_aff=[[1, 0, 0], [0, 1, 0]]), crop=(9, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        flowsynth.synthesize(x.cpu(), flowsynth.params_from("affine", 8, 8, theta_aff=[[1, 0, 0], [0, 1, 0]]))
    assert int(count[0]) == 0                               # nothing was launched

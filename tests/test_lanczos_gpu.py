"""Pillow's LANCZOS resize on the device (csrc/resample.hip through refign_amd/resample.py) against Pillow's own pixels
(tests/golden/lanczos_pillow.npz, made with Pillow alone) and against the reference's transforms around them
(tests/golden/matcher_ingest.npz): every comparison is equality of bytes, and of fp32 BITS after the normalisation; the padding of
transforms.PadBottomRight is exactly 0.0 and written by the same launch."""
import numpy as np
import pytest
import torch
from conftest import golden
from make_golden_lanczos import BINARY, CASES, CHAIN, binary_in, case_name, image_in
from make_golden_matcher_ingest import IMAGE, IMAGE_REF, SIZE, points_in
from make_golden_matcher_ingest import image_in as decoded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return golden("lanczos_pillow")


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


def chw(a):
    return torch.from_numpy(a).permute(2, 0, 1)


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_lanczos_resize_equals_pillow(dev, fixture, case):
    from refign_amd.resample import resize_u8
    H, W, h, w = case
    img = resize_u8(up(image_in(H, W), dev), (h, w), filter="lanczos")
    assert img.dtype == torch.uint8 and tuple(img.shape) == (3, h, w)
    assert torch.equal(img.cpu(), chw(fixture["img_" + case_name(case)]))


def test_overshoot_is_clipped_between_the_passes(dev, fixture):
    from refign_amd.resample import resize_u8
    H, W, h, w = BINARY
    got = resize_u8(up(binary_in(H, W), dev), (h, w), filter="lanczos")
    assert torch.equal(got.cpu(), chw(fixture["bin_" + case_name(BINARY)]))


def test_two_resizes_keep_the_byte_image_in_between(dev, fixture):
    from refign_amd.resample import resize_u8
    mid = resize_u8(up(image_in(*CHAIN[0]), dev), CHAIN[1], filter="lanczos").permute(1, 2, 0).contiguous()
    assert torch.equal(resize_u8(mid, CHAIN[2], filter="lanczos").cpu(), chw(fixture["chain"]))


@pytest.mark.parametrize("pad_to", [(20, 70), (41, 25), (16, 25)], ids=lambda p: "pad%dx%d" % p)
def test_fused_normalise_and_pad(dev, fixture, pad_to):
    """27 x 43 -> 16 x 25 padded to 20 x 70 (rows below the image inside its tile, a second column tile of padding alone), to
    41 x 25 (tiles of padding alone below) and not at all.  The output starts as NaN: a pixel nobody wrote would show."""
    from refign_amd.datastep import crop_flip_normalize
    from refign_amd.resample import resize_crop_flip_normalize
    case = (27, 43, 16, 25)
    H, W, h, w = case
    want, _ = crop_flip_normalize(up(fixture["img_" + case_name(case)].transpose(2, 0, 1), dev), None, 0, 0, h, w, False)
    out = torch.full((3,) + pad_to, float("nan"), dtype=torch.float32, device=dev)
    got = resize_crop_flip_normalize(up(image_in(H, W), dev), (h, w), 0, 0, h, w, False, out, filter="lanczos", pad_to=pad_to)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(bits(out[:, :h, :w]), bits(want))
    outside = torch.ones(pad_to, dtype=torch.bool, device=dev)
    outside[:h, :w] = False
    assert int(outside.sum()) == pad_to[0] * pad_to[1] - h * w
    assert bool((bits(out[:, outside]) == 0).all())                    # +0.0 exactly: not NaN, not -0.0
    fresh = resize_crop_flip_normalize(up(image_in(H, W), dev), (h, w), 0, 0, h, w, False, filter="lanczos", pad_to=pad_to)
    assert tuple(fresh.shape) == (3,) + pad_to and torch.equal(bits(fresh), bits(out))


def test_pad_with_the_bilinear_filter_and_defaults(dev):
    """the filter and the padding are independent; the defaults are the calls of before"""
    from refign_amd.resample import resize_crop_flip_normalize, resize_u8
    img = up(image_in(27, 43), dev)
    plain = resize_crop_flip_normalize(img, (16, 25), 2, 3, 11, 17, True)
    assert torch.equal(bits(plain), bits(resize_crop_flip_normalize(img, (16, 25), 2, 3, 11, 17, True, filter="bilinear")))
    padded = resize_crop_flip_normalize(img, (16, 25), 2, 3, 11, 17, True, pad_to=(13, 66))
    assert torch.equal(bits(padded[:, :11, :17]), bits(plain)) and int((bits(padded) != 0).sum()) == int((bits(plain) != 0).sum())
    assert torch.equal(resize_u8(img, (16, 25)), resize_u8(img, (16, 25), filter="bilinear"))
    assert not torch.equal(resize_u8(img, (16, 25)), resize_u8(img, (16, 25), filter="lanczos"))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("box", [(1, 2, 65, 117), (30, 50, 5, 9)], ids=lambda b: "crop%d.%d.%d.%d" % b)
def test_fused_crop_is_bit_equal_to_crop_of_pillows_image(dev, fixture, box, flip):
    from refign_amd.datastep import crop_flip_normalize
    from refign_amd.resample import resize_crop_flip_normalize
    case = (135, 240, 67, 120)
    H, W, h, w = case
    top, left, ch, cw = box
    want, _ = crop_flip_normalize(up(fixture["img_" + case_name(case)].transpose(2, 0, 1), dev), None, top, left, ch, cw, flip)
    got = resize_crop_flip_normalize(up(image_in(H, W), dev), (h, w), top, left, ch, cw, flip, filter="lanczos")
    assert tuple(got.shape) == (3, ch, cw) and torch.equal(bits(got), bits(want))
    padded = resize_crop_flip_normalize(up(image_in(H, W), dev), (h, w), top, left, ch, cw, flip, filter="lanczos", pad_to=(ch + 3, cw + 70))
    assert torch.equal(bits(padded[:, :ch, :cw]), bits(want)) and not padded[:, ch:].any() and not padded[:, :, cw:].any()


def test_scale_limit_of_the_lanczos_filter(dev):
    """129 taps per pixel are ceil(3 * scale) <= 64 for Lanczos: down-scaling by 22 is refused with a message that names the
    filter and the cap, and nothing is launched (the output keeps what it held); by 21 it runs"""
    from refign_amd import _lib, resample
    from refign_amd._tensor import ptr
    img = up(image_in(9, 220), dev)                                    # 220 -> 10: 22 x, ceil(66) * 2 + 1 = 133 taps
    out = torch.full((3, 9, 10), 7.0, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="lanczos filter needs 7 x 133 taps per pixel, the kernel is built for 129 .lanczos: down-scaling"):
        resample.resize_crop_flip_normalize(img, (9, 10), 0, 0, 9, 10, False, out, filter="lanczos")
    assert bool((out == 7.0).all())
    with pytest.raises(RuntimeError, match="lanczos.*129"):
        resample.resize_u8(img, (9, 10), filter="lanczos")
    assert tuple(resample.resize_u8(img, (9, 10)).shape) == (3, 9, 10)           # bilinear takes the same sizes: 45 taps
    img = up(image_in(9, 210), dev)                                    # 21 x: 127 taps
    got = resample.resize_u8(img, (9, 10), filter="lanczos")
    assert torch.equal(got.cpu(), chw(resample.lanczos_reference(image_in(9, 210), (9, 10))))
    # the tables must be the filter's: bilinear tables handed in as Lanczos ones are refused, and so is an output smaller than the crop
    bx, cx, kx = resample._device_tables("bilinear", 210, 10, dev)
    by, cy, ky = resample._device_tables("bilinear", 9, 9, dev)
    u8 = torch.zeros((3, 9, 10), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="tables of 3 x 43 taps.*take 7 x 127 .lanczos"):
        _lib.call("rfn_resize_filter_u8", dev, ptr(img), 9, 210, 9, 10, 1, ptr(bx), ptr(cx), kx, ptr(by), ptr(cy), ky, ptr(u8))
    with pytest.raises(RuntimeError, match="filter 2"):
        _lib.call("rfn_resize_filter_u8", dev, ptr(img), 9, 210, 9, 10, 2, ptr(bx), ptr(cx), kx, ptr(by), ptr(cy), ky, ptr(u8))
    with pytest.raises(RuntimeError, match="out_image must be"):
        resample.resize_crop_flip_normalize(img, (9, 10), 0, 0, 9, 10, False, out, filter="lanczos", pad_to=(9, 12))
    with pytest.raises(RuntimeError, match="smaller than the 9 x 10 crop"):
        resample.resize_crop_flip_normalize(img, (9, 10), 0, 0, 9, 10, False, filter="lanczos", pad_to=(9, 8))
    assert not u8.any()


def test_eval_ingest_of_the_matcher_pipeline(dev):
    """decoded uint8 arrays and points -> the batch of the matcher's `test:` section, against the reference's own transforms"""
    from refign_amd.resample import EvalIngest
    z = golden("matcher_ingest")
    img, ref = decoded(*IMAGE, "image"), decoded(*IMAGE_REF, "image_ref")
    pts, pts_ref = points_in(*IMAGE, "image"), points_in(*IMAGE_REF, "image_ref")
    out = EvalIngest(resize=SIZE, interpolation="lanczos", pad="same")(img, image_ref=ref, corr_pts=pts, corr_pts_ref=pts_ref)
    assert set(out) == {"image", "image_ref", "corr_pts", "corr_pts_ref"}
    for key in ("image", "image_ref"):
        assert tuple(out[key].shape) == (1, 3, 128, 160) and out[key].dtype == torch.float32 and out[key].device == dev
        assert torch.equal(bits(out[key][0]), torch.from_numpy(z[key].view(np.int32))), key
    for key in ("corr_pts", "corr_pts_ref"):
        assert isinstance(out[key], list) and len(out[key]) == 1 and out[key][0].device == dev
        assert torch.equal(bits(out[key][0]), torch.from_numpy(z[key].view(np.int32))), key
    # a fixed pad size, device inputs, load-time dims in front: two Lanczos resizes with a byte image in between
    two = EvalIngest(dims=CHAIN[1], resize=CHAIN[2], dims_interpolation="lanczos", interpolation="lanczos", pad=(48, 80))
    got = two(up(image_in(*CHAIN[0]), dev))["image"]
    from refign_amd.datastep import crop_flip_normalize
    want, _ = crop_flip_normalize(up(golden("lanczos_pillow")["chain"].transpose(2, 0, 1), dev), None, 0, 0, *CHAIN[2], False)
    assert tuple(got.shape) == (1, 3, 48, 80) and torch.equal(bits(got[0, :, :40, :72]), bits(want))
    assert not got[0, :, 40:].any() and not got[0, :, :, 72:].any()

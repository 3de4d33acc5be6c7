"""The load-time resize on the device (csrc/resample.hip through refign_amd/resample.py) against Pillow's own pixels
(tests/golden/resample_pillow.npz, made with Pillow alone): every comparison is equality of bytes, and of fp32 BITS after the
normalisation -- the arithmetic is integer up to the byte, then u8 / 255, (x - mean) / std with true divisions exactly as
datastep.crop_flip_normalize computes it."""
import random

import numpy as np
import pytest
import torch
from conftest import golden
from make_golden_resample import (EVAL, EVAL_DIMS, EVAL_RESIZE, SET_DIMS, SET_N, case_name, image_in, label_in, sampler_set)

pytestmark = pytest.mark.gpu
SIZES = [(24, 40, 12, 20), (27, 43, 16, 25), (9, 13, 16, 25), (37, 64, 37, 21), (100, 333, 31, 7)]
# (case, crop (top, left, h, w) of the resized image): the places where the fused kernel can go wrong
CROPS = [((24, 40, 12, 20), (0, 0, 12, 20)),          # the whole image
         ((54, 96, 27, 48), (9, 21, 18, 27)),         # touches the right and the bottom edge: the tables are clipped there
         ((27, 43, 16, 25), (3, 5, 11, 17)),          # left and w odd
         ((135, 240, 67, 120), (30, 50, 5, 9)),       # smaller than one 16 x 64 tile
         ((135, 240, 67, 120), (1, 2, 65, 117)),      # more than one tile in both directions, ragged last tiles
         ((9, 13, 16, 25), (2, 1, 13, 23)),           # up-sampling
         ((37, 64, 37, 21), (0, 0, 37, 21)),          # one axis keeps its size (Pillow skips that pass)
         ((100, 333, 31, 7), (1, 0, 30, 7))]          # 47.6 x along x (97 taps), 3.2 x along y


@pytest.fixture(scope="module")
def fixture():
    return golden("resample_pillow")


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("case", SIZES, ids=case_name)
def test_resize_equals_pillow(dev, fixture, case):
    from refign_amd.resample import resize_nearest_u8, resize_u8
    H, W, h, w = case
    lbl = resize_nearest_u8(up(label_in(H, W), dev), (h, w))
    assert lbl.dtype == torch.uint8 and torch.equal(lbl.cpu(), torch.from_numpy(fixture["lbl_" + case_name(case)]))
    img = resize_u8(up(image_in(H, W), dev), (h, w))
    assert img.dtype == torch.uint8 and tuple(img.shape) == (3, h, w)
    assert torch.equal(img.cpu(), torch.from_numpy(fixture["img_" + case_name(case)]).permute(2, 0, 1))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("case,box", CROPS, ids=[case_name(c) + "_crop%d.%d.%d.%d" % b for c, b in CROPS])
def test_fused_crop_is_bit_equal_to_crop_of_pillows_image(dev, fixture, case, box, flip):
    from refign_amd.datastep import crop_flip_normalize
    from refign_amd.resample import resize_crop_flip_normalize
    H, W, h, w = case
    top, left, ch, cw = box
    resized = up(fixture["img_" + case_name(case)].transpose(2, 0, 1), dev)
    want, _ = crop_flip_normalize(resized, None, top, left, ch, cw, flip)
    got = resize_crop_flip_normalize(up(image_in(H, W), dev), (h, w), top, left, ch, cw, flip)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, ch, cw)
    assert torch.equal(bits(got), bits(want))
    slot = torch.zeros((2, 3, ch, cw), dtype=torch.float32, device=dev)      # into a slot of a batch tensor
    assert resize_crop_flip_normalize(up(image_in(H, W), dev), (h, w), top, left, ch, cw, flip, slot[1]).data_ptr() == slot[1].data_ptr()
    assert torch.equal(bits(slot[1]), bits(want)) and not slot[0].any()


def _set(fixture, resized):
    """the samplers' data set: decoded samples (channels last), or what Pillow's load-time resize leaves of them (ToTensor's
    layout)"""
    if not resized:
        return sampler_set()
    return ([fixture[f"set_img{i}"].transpose(2, 0, 1) for i in range(SET_N)], [fixture[f"set_ref{i}"].transpose(2, 0, 1) for i in range(SET_N)],
            [fixture[f"set_lbl{i}"] for i in range(SET_N)])


def _host(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_rare_class_sampler_from_decoded_files(dev, fixture):
    from refign_amd.datastep import RareClassSourceSampler
    classes, prob = [11, 12, 13], [0.5, 0.3, 0.2]
    small = _set(fixture, True)[2]
    with_class = {c: [i for i in range(SET_N) if (small[i] == c).sum() > 0] for c in classes}
    assert all(with_class.values())
    runs = []
    for dims in (None, SET_DIMS):
        imgs, _, lbls = _set(fixture, dims is None)
        redraws = [0]

        def load(i, imgs=imgs, lbls=lbls):
            return _host(imgs[i]), _host(lbls[i])

        s = RareClassSourceSampler(load, classes, prob, with_class, (32, 32), dev, cat_max_ratio=0.75, rcs_min_pixels=60,
                                   rcs_min_crop_ratio=0.5, dims=dims)
        inner = s._augment_params
        s._augment_params = lambda *a, inner=inner, redraws=redraws: (redraws.__setitem__(0, redraws[0] + 1), inner(*a))[1]
        random.seed(7)
        out = [s.sample() for _ in range(6)]
        runs.append(([bits(a) for a, _ in out], [b.cpu() for _, b in out], random.getstate(), redraws[0]))
    (ia, la, sa, ra), (ib, lb, sb, rb) = runs
    assert ra == rb and ra > 6                                        # the re-draw chain of rare-class sampling ran
    assert sa == sb                                                   # python's `random` stream stands where it stood
    for k in range(6):
        assert torch.equal(ia[k], ib[k]) and torch.equal(la[k], lb[k]), k
        assert lb[k].dtype == torch.int64 and tuple(lb[k].shape) == (32, 32)


def test_pair_sampler_from_decoded_files(dev, fixture):
    from refign_amd.datastep import PairSampler
    runs = []
    for dims in (None, SET_DIMS):
        imgs, refs, _ = _set(fixture, dims is None)
        s = PairSampler(lambda i, imgs=imgs, refs=refs: (_host(imgs[i]), _host(refs[i])), (32, 48), dev, dims=dims)
        random.seed(11)
        out = [s.sample(i % SET_N) for i in range(5)]
        runs.append(([bits(a) for a, _ in out], [bits(b) for _, b in out], random.getstate()))
    (ia, ra, sa), (ib, rb, sb) = runs
    assert sa == sb
    for k in range(5):
        assert tuple(ia[k].shape) == (3, 32, 48) and torch.equal(ia[k], ib[k]) and torch.equal(ra[k], rb[k]), k


def test_eval_ingest(dev, fixture):
    from refign_amd.datastep import crop_flip_normalize
    from refign_amd.resample import EvalIngest
    img, lbl = image_in(*EVAL), label_in(*EVAL)
    h, w = EVAL_RESIZE

    def normalized(hwc):
        return crop_flip_normalize(up(hwc.transpose(2, 0, 1), dev), None, 0, 0, h, w, False)[0]

    # load-time dims, then transforms.Resize: two Pillow resizes with a uint8 image in between
    out = EvalIngest(dims=EVAL_DIMS, resize=EVAL_RESIZE)(img, semantic=lbl, image_ref=img)
    assert tuple(out["image"].shape) == (1, 3, h, w) and out["image"].dtype == torch.float32 and out["image"].device == dev
    assert torch.equal(bits(out["image"][0]), bits(normalized(fixture["eval_img2"])))
    assert torch.equal(bits(out["image_ref"]), bits(out["image"]))
    assert out["semantic"].dtype == torch.int64 and torch.equal(out["semantic"][0].cpu(), torch.from_numpy(fixture["eval_lbl2"]).long())
    assert not np.array_equal(fixture["eval_img2"], fixture["eval_img1"])     # (merging the two resizes would show)
    # a `test:` section: Resize alone with img_only -- the label keeps its size
    out = EvalIngest(resize=EVAL_RESIZE, img_only=True)(up(img, dev), semantic=up(lbl, dev))
    assert torch.equal(bits(out["image"][0]), bits(normalized(fixture["eval_img1"])))
    assert torch.equal(out["semantic"][0].cpu(), torch.from_numpy(lbl).long())
    # nothing to resize: conversion and normalisation alone
    out = EvalIngest()(fixture["eval_img1"])
    assert torch.equal(bits(out["image"][0]), bits(normalized(fixture["eval_img1"]))) and "semantic" not in out


def test_cpu_tensors_are_refused(dev):
    from refign_amd import resample
    img, lbl = torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((8, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resample.resize_u8(img, (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resample.resize_nearest_u8(lbl, (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resample.resize_crop_flip_normalize(img, (4, 4), 0, 0, 4, 4, False)
    with pytest.raises(RuntimeError, match="channels last"):
        resample.resize_u8(torch.zeros((3, 8, 8), dtype=torch.uint8, device=dev), (4, 4))


def test_scale_limit(dev):
    """down-scaling by more than 64 needs more than the 129 taps per pixel the kernel is built for: the library says so and
    launches nothing (the output keeps what it held)"""
    from refign_amd import resample
    img = up(image_in(9, 650), dev)                                    # 650 -> 10: 65 x, 131 taps
    out = torch.full((3, 9, 10), 7.0, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="131 taps per pixel, the kernel is built for 129"):
        resample.resize_crop_flip_normalize(img, (9, 10), 0, 0, 9, 10, False, out)
    assert bool((out == 7.0).all())
    with pytest.raises(RuntimeError, match="taps per pixel"):
        resample.resize_u8(img, (9, 10))
    with pytest.raises(RuntimeError, match="outside the 9 x 20 resized image"):
        resample.resize_crop_flip_normalize(img, (9, 20), 0, 5, 9, 16, False)
    got = resample.resize_u8(img, (9, 20))                             # 32.5 x: inside the limit
    assert torch.equal(got.cpu(), torch.from_numpy(resample.resize_reference(image_in(9, 650), (9, 20))).permute(2, 0, 1))

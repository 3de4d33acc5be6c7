"""CPU: the host half of the matcher's ingest (refign_amd/resample.py, refign_amd/config.py): the numpy restatement of Pillow's
LANCZOS resize equals tests/golden/lanczos_pillow.npz (made by tests/golden/make_golden_lanczos.py with Pillow alone) byte for
byte, and live Pillow where it is installed; the tables (filter_tables == bilinear_tables for "bilinear", the accumulator bound);
config.ingest_plan on the reference's matcher configs; EvalIngest's point scaling against the reference's own transforms
(tests/golden/matcher_ingest.npz); the library's new entry points.  No tolerance anywhere."""
import os

import numpy as np
import pytest
import torch
from conftest import golden
from make_golden_lanczos import BINARY, CASES, CHAIN, binary_in, case_name, image_in
from make_golden_matcher_ingest import IMAGE, IMAGE_REF, SIZE, points_in

REF_CONFIGS = "/root/reference/configs"
needs_reference = pytest.mark.skipif(not os.path.isdir(REF_CONFIGS), reason="the reference checkout is absent")


@pytest.fixture(scope="module")
def fixture():
    return golden("lanczos_pillow")


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_restatement_equals_the_fixture(fixture, case):
    from refign_amd.resample import lanczos_reference
    H, W, h, w = case
    np.testing.assert_array_equal(lanczos_reference(image_in(H, W), (h, w)), fixture["img_" + case_name(case)])


def test_restatement_clips_the_overshoot(fixture):
    """an image of 0 and 255 only: the negative lobes push sums below 0 and above 255 in both passes"""
    from refign_amd.resample import PRECISION_BITS, filter_tables, lanczos_reference
    H, W, h, w = BINARY
    img = binary_in(H, W)
    assert set(np.unique(img)) == {0, 255}
    np.testing.assert_array_equal(lanczos_reference(img, (h, w)), fixture["bin_" + case_name(BINARY)])
    xmin, n, coef = filter_tables(W, w, "lanczos")                    # the horizontal pass does leave [0, 255] before the clip
    raw = np.stack([(img[:, xmin[x]:xmin[x] + n[x], 0].astype(np.int64) * coef[x, :n[x]]).sum(1) for x in range(w)], 1)
    raw = (raw + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS
    assert (raw < 0).sum() > 50 and (raw > 255).sum() > 50


def test_chained_resizes_keep_the_byte_image_in_between(fixture):
    from refign_amd.resample import lanczos_reference
    img = image_in(*CHAIN[0])
    np.testing.assert_array_equal(lanczos_reference(lanczos_reference(img, CHAIN[1]), CHAIN[2]), fixture["chain"])
    assert not np.array_equal(lanczos_reference(img, CHAIN[2]), fixture["chain"])       # (merging the two would show)


@pytest.mark.parametrize("case", CASES + [BINARY], ids=case_name)
def test_restatement_and_fixture_equal_live_pillow(fixture, case):
    Image = pytest.importorskip("PIL.Image")
    from refign_amd.resample import lanczos_reference
    H, W, h, w = case
    img, name = (binary_in(H, W), "bin_") if case == BINARY else (image_in(H, W), "img_")
    live = np.asarray(Image.fromarray(img).resize((w, h), Image.LANCZOS))
    np.testing.assert_array_equal(fixture[name + case_name(case)], live)
    np.testing.assert_array_equal(lanczos_reference(img, (h, w)), live)


def test_filter_tables():
    from refign_amd.resample import bilinear_tables, filter_tables
    for a, b in [(40, 20), (13, 25), (13, 13), (333, 7), (170, 10), (97, 60)]:
        for got, want in zip(filter_tables(a, b, "bilinear"), bilinear_tables(a, b)):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        assert all(np.array_equal(g, w) for g, w in zip(filter_tables(a, b), bilinear_tables(a, b)))     # the default filter
    xmin, n, coef = filter_tables(40, 20, "lanczos")                  # scale 2: support 6, 13 taps
    assert coef.shape == (20, 13) and xmin.dtype == n.dtype == coef.dtype == np.int32
    assert xmin[0] == 0 and xmin[-1] + n[-1] == 40 and int(n.max()) == 12
    assert (coef < 0).any() and all(abs(int(coef[i, :n[i]].sum()) - (1 << 22)) <= 6 for i in range(20))
    assert filter_tables(13, 25, "lanczos")[2].shape[1] == 7          # up-scaling: support 3
    assert filter_tables(260, 13, "lanczos")[2].shape[1] == 121       # scale 20
    xmin, n, coef = filter_tables(13, 13, "lanczos")                  # an axis that keeps its size: the identity
    assert all(list(coef[i, :n[i]]).count(1 << 22) == 1 and int(np.abs(coef[i]).sum()) == 1 << 22 for i in range(13))
    assert all(xmin[i] + list(coef[i]).index(1 << 22) == i for i in range(13))
    with pytest.raises(ValueError, match="bicubic"):
        filter_tables(10, 5, "bicubic")


def test_accumulator_bound():
    """255 * sum |coef| + 2^21 < 2^31 is a checked condition once taps can be negative: every Lanczos table of the golden's size
    pairs holds it with room, a hand-made row that violates it is refused"""
    from refign_amd.resample import check_accumulator, filter_tables
    for H, W, h, w in CASES + [BINARY]:
        for a, b in ((H, h), (W, w)):
            coef = filter_tables(a, b, "lanczos")[2].astype(np.int64)
            assert 255 * int(np.abs(coef).sum(1).max()) + (1 << 21) <= 0.78 * 2 ** 31
    ok = np.array([[1 << 22, 0, 0]], np.int32)
    check_accumulator(ok)
    limit = ((1 << 31) - (1 << 21)) // 255                            # the largest sum |coef| with 255 * sum + 2^21 < 2^31 ...
    assert 255 * limit + (1 << 21) < 1 << 31 <= 255 * (limit + 1) + (1 << 21)
    check_accumulator(np.array([[limit // 2, -(limit - limit // 2)]], np.int32))
    with pytest.raises(ValueError, match="overflows the int32 accumulator"):
        check_accumulator(np.array([[(limit + 1) // 2 + 1, -((limit + 1) // 2)]], np.int32))     # ... and one more
    with pytest.raises(ValueError, match="overflows the int32 accumulator"):
        check_accumulator(np.stack([ok[0], np.array([6 << 22, -(5 << 22), 0], np.int32)]))       # sums to one, yet overflows


@needs_reference
def test_ingest_plan_of_the_matcher_configs():
    from refign_amd import config
    cfg = config.load_config(os.path.join(REF_CONFIGS, "megadepth", "uawarpc_evalonly.yaml"))
    for ds in ("MegaDepth", "RobotCarMatching"):
        plan = config.ingest_plan(cfg, "test", ds)
        assert plan["resize"] == 480 and plan["interpolation"] == "lanczos" and plan["pad"] == "same"
        assert plan["dims"] is None and plan["dims_interpolation"] == "lanczos" and not plan["img_only"]
        assert plan["load_keys"] == ["image", "image_ref"]
    # (uawarpc_evalonly.yaml has no `val:` section; the matcher's validation set is configured in the two training configs)
    for name in ("uawarpc_stage1.yaml", "uawarpc_stage2.yaml"):
        cfg = config.load_config(os.path.join(REF_CONFIGS, "megadepth", name))
        val = config.ingest_plan(cfg, "val", "MegaDepth")
        assert val["dims"] == (480, 720) and val["dims_interpolation"] == "lanczos"
        assert val["resize"] is None and val["interpolation"] == "bilinear" and val["pad"] is None
        assert config.ingest_plan(cfg, "test", "MegaDepth")["pad"] == "same"
        with pytest.raises(config.OutOfScopeError, match="ColorJitter"):
            config.ingest_plan(cfg, "train", "MegaDepth")
    seg = config.load_config(os.path.join(REF_CONFIGS, "cityscapes_acdc", "refign_daformer.yaml"))
    for split in ("val", "test", "predict"):                          # the segmentation data sets: bilinear, no padding
        plan = config.ingest_plan(seg, split, "ACDC")
        assert plan["interpolation"] == plan["dims_interpolation"] == "bilinear" and plan["pad"] is None


def _cfg(transforms, dataset="MegaDepth", **sec):
    return {"data": {"init_args": {"load_config": {"test": {dataset: {"load_keys": ["image", "image_ref"],
                                                                       "transforms": transforms, **sec}}}}}}


def _t(name, **args):
    return {"class_path": "data_modules.transforms." + name, "init_args": args}


def test_ingest_plan_interpolation_and_pad():
    from refign_amd import config
    plan = config.ingest_plan(_cfg([_t("Resize", size=[96, 128], img_interpolation="bilinear"), _t("ToTensor"),
                                    _t("ConvertImageDtype"), _t("Normalize"), _t("PadBottomRight", size=[128, 160])]),
                              "test", "MegaDepth")
    assert plan["resize"] == (96, 128) and plan["interpolation"] == "bilinear" and plan["pad"] == (128, 160)
    with pytest.raises(config.OutOfScopeError, match="bicubic"):
        config.ingest_plan(_cfg([_t("Resize", size=480, img_interpolation="bicubic")]), "test", "MegaDepth")
    with pytest.raises(config.OutOfScopeError, match="PadBottomRight"):   # before Normalize the fill would not be 0
        config.ingest_plan(_cfg([_t("ToTensor"), _t("PadBottomRight", size=[8, 8]), _t("Normalize")]), "test", "MegaDepth")
    with pytest.raises(config.OutOfScopeError, match="same_shape_keys"):
        config.ingest_plan(_cfg([_t("PadBottomRight")]), "test", "MegaDepth")
    with pytest.raises(config.OutOfScopeError, match="same_shape_keys"):
        config.ingest_plan(_cfg([_t("PadBottomRight", same_shape_keys=["image"])]), "test", "MegaDepth")
    with pytest.raises(config.OutOfScopeError, match="ignore_index"):
        config.ingest_plan(_cfg([_t("PadBottomRight", size=[8, 8], ignore_index=0)]), "test", "MegaDepth")
    rc = config.ingest_plan(_cfg([_t("ToTensor")], "RobotCarMatching", resize_filter="bilinear"), "test", "RobotCarMatching")
    assert rc["dims_interpolation"] == "bilinear"
    assert config.ingest_plan(_cfg([_t("ToTensor")], "RobotCarMatching"), "test", "RobotCarMatching")["dims_interpolation"] == "lanczos"
    with pytest.raises(config.OutOfScopeError, match="hamming"):
        config.ingest_plan(_cfg([_t("ToTensor")], "RobotCarMatching", resize_filter="hamming"), "test", "RobotCarMatching")
    assert config.ingest_plan(_cfg([_t("ToTensor")], "ACDC"), "test", "ACDC")["dims_interpolation"] == "bilinear"


def test_point_scaling_equals_the_reference():
    """EvalIngest's host-side point arithmetic against the points the reference's own Resize left (bit for bit): each set by its
    own image's size change, 160 x 200 -> 128 x 160 (x 0.8) and 192 x 210 -> 128 x 140 (x 2 / 3)"""
    from refign_amd.resample import EvalIngest, scale_points
    z = golden("matcher_ingest")
    ing = EvalIngest(resize=SIZE, interpolation="lanczos", pad="same")
    assert ing.final_size(*IMAGE) == tuple(z["size"]) == (128, 160) and ing.final_size(*IMAGE_REF) == tuple(z["size_ref"]) == (128, 140)
    for key, (H, W), tag in (("corr_pts", IMAGE, "image"), ("corr_pts_ref", IMAGE_REF, "image_ref")):
        src = points_in(H, W, tag)
        assert ((src < 0).any(1) | (src[:, 0] >= W) | (src[:, 1] >= H)).sum() >= 3      # a few points outside the image
        got = ing.points(src, H, W)
        assert got.dtype == torch.float32 and not got.is_cuda
        assert np.array_equal(got.numpy().view(np.int32), z[key].view(np.int32)), key
        assert np.array_equal(src, points_in(H, W, tag))              # the input is left alone
    # the short side already matches: the reference skips the points (and the image) of that sample
    same = points_in(128, 300, "same")
    assert np.array_equal(ing.points(same, 128, 300).numpy(), same)
    # load-time dims, then Resize: two scalings, each rounded to fp32 (not one merged factor)
    two = EvalIngest(dims=(96, 150), resize=64, dims_interpolation="lanczos", interpolation="lanczos")
    want = scale_points(scale_points(same, 128, 300, 96, 150), 96, 150, 64, 100)
    assert np.array_equal(two.points(same, 128, 300).numpy(), want.numpy())
    f32 = np.float32
    assert np.array_equal(want.numpy()[:, 0], f32(100 / 150.0) * (f32(150 / 300.0) * same[:, 0]))
    # img_only: the Resize leaves the points alone, the reader's dims do not
    only = EvalIngest(dims=(96, 150), resize=64, img_only=True)
    assert np.array_equal(only.points(same, 128, 300).numpy(), scale_points(same, 128, 300, 96, 150).numpy())


def test_golden_images_are_the_padded_restatement():
    """matcher_ingest.npz (the reference's transforms around Pillow) against the numpy restatement: Lanczos, / 255, (x - mean) /
    std, zeros right of and below the image"""
    from refign_amd.datastep import IMNET_MEAN, IMNET_STD
    from refign_amd.resample import lanczos_reference, pad_bottom_right_reference
    from make_golden_matcher_ingest import image_in as decoded
    z = golden("matcher_ingest")
    m, s = np.asarray(IMNET_MEAN, np.float32).reshape(3, 1, 1), np.asarray(IMNET_STD, np.float32).reshape(3, 1, 1)
    for key, (H, W), size in (("image", IMAGE, z["size"]), ("image_ref", IMAGE_REF, z["size_ref"])):
        u8 = lanczos_reference(decoded(H, W, key), size).transpose(2, 0, 1)
        want = pad_bottom_right_reference((u8.astype(np.float32) / np.float32(255) - m) / s, (128, 160))
        assert np.array_equal(want.view(np.int32), z[key].view(np.int32)), key
    assert not z["image_ref"][:, :, 140:].any() and z["image_ref"][:, :, :140].all()


def test_library_exports_the_new_entry_points():
    from refign_amd import _lib
    for name in ("rfn_resize_filter_u8", "rfn_resize_filter_crop_flip_norm_pad_u8", "rfn_sparse_epe_f32"):
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][1][-1] is _lib.c_void_p, name     # the stream comes last
        assert getattr(_lib.load_library(), name) is not None
    assert _lib.ABI_VERSION == 5 and _lib.abi_version() == 5
    for name in ("rfn_resize_crop_flip_norm_u8", "rfn_resize_u8", "rfn_resize_nearest_u8"):     # the old ones keep their shape
        assert len(_lib.SIGNATURES[name][1]) == {"rfn_resize_crop_flip_norm_u8": 20, "rfn_resize_u8": 13, "rfn_resize_nearest_u8": 9}[name]

"""CPU: the host half of the load-time resize (refign_amd/resample.py): the numpy restatements of Pillow's 8-bit resize equal
tests/golden/resample_pillow.npz (made by tests/golden/make_golden_resample.py with Pillow alone) byte for byte, and live Pillow
where it is installed; the size arithmetic of transforms.Resize; config.ingest_plan on the reference's configs.  No tolerance:
every comparison is equality of bytes."""
import os

import numpy as np
import pytest
from conftest import golden
from make_golden_resample import CASES, case_name, image_in, label_in

CPU_CASES = [(24, 40, 12, 20), (27, 43, 16, 25), (9, 13, 16, 25), (37, 64, 37, 21), (100, 333, 31, 7)]
REF_CONFIGS = "/root/reference/configs"


@pytest.fixture(scope="module")
def fixture():
    return golden("resample_pillow")


@pytest.mark.parametrize("case", CPU_CASES, ids=case_name)
def test_restatements_equal_the_fixture(fixture, case):
    from refign_amd.resample import resize_nearest_reference, resize_reference
    assert case in CASES
    H, W, h, w = case
    np.testing.assert_array_equal(resize_reference(image_in(H, W), (h, w)), fixture["img_" + case_name(case)])
    np.testing.assert_array_equal(resize_nearest_reference(label_in(H, W), (h, w)), fixture["lbl_" + case_name(case)])


@pytest.mark.parametrize("case", CPU_CASES, ids=case_name)
def test_restatements_and_fixture_equal_live_pillow(fixture, case):
    Image = pytest.importorskip("PIL.Image")
    from refign_amd.resample import resize_nearest_reference, resize_reference
    H, W, h, w = case
    img, lbl = image_in(H, W), label_in(H, W)
    live = np.asarray(Image.fromarray(img).resize((w, h), Image.BILINEAR))
    live_lbl = np.asarray(Image.fromarray(lbl).resize((w, h), Image.NEAREST))
    np.testing.assert_array_equal(fixture["img_" + case_name(case)], live)
    np.testing.assert_array_equal(fixture["lbl_" + case_name(case)], live_lbl)
    np.testing.assert_array_equal(resize_reference(img, (h, w)), live)
    np.testing.assert_array_equal(resize_nearest_reference(lbl, (h, w)), live_lbl)


def test_tables():
    from refign_amd.resample import bilinear_tables, nearest_table
    xmin, n, coef = bilinear_tables(40, 20)                           # scale 2: support 2, 5 taps at the most
    assert coef.shape == (20, 5) and xmin.dtype == n.dtype == coef.dtype == np.int32
    assert xmin[0] == 0 and n[0] == 3 and xmin[-1] + n[-1] == 40      # clipped at both edges
    assert list(xmin[1:4]) == [1, 3, 5] and list(n[1:4]) == [4, 4, 4]
    assert list(coef[1]) == [524288, 1572864, 1572864, 524288, 0]     # (1, 3, 3, 1) / 8 in 22-bit fixed point
    assert all(abs(int(coef[i, :n[i]].sum()) - (1 << 22)) <= 2 for i in range(20))
    xmin, n, coef = bilinear_tables(13, 13)                           # an axis that keeps its size: the identity
    assert list(xmin) == list(range(13)) and (coef[:, 0] == 1 << 22).all() and (coef[:, 1:] == 0).all()
    assert bilinear_tables(170, 10)[2].shape[1] == 35                 # scale 17
    assert list(nearest_table(40, 20)) == list(range(1, 40, 2))
    assert list(nearest_table(13, 25)) == [int((x + 0.5) * 13 / 25) for x in range(25)]
    tab = nearest_table(333, 7)
    assert tab.dtype == np.int32 and tab[0] == 23 and 0 <= tab.min() and tab.max() < 333


def test_target_size():
    from refign_amd.resample import target_size
    assert target_size(1080, 1920, (540, 960)) == (540, 960)          # a pair is (h, w) as it stands
    assert target_size(1080, 1920, 540) == (540, 960)                 # int: the shorter side; int(540 * 1920 / 1080)
    assert target_size(1920, 1080, 540) == (960, 540)                 # portrait: the width is the shorter side
    assert target_size(100, 333, 31) == (31, 103)                     # int(31 * 333 / 100) = int(103.23)
    assert target_size(540, 960, 540) == (540, 960)                   # already there
    assert target_size(480, 640, [512]) == (512, 682)                 # a one-element sequence is the int; int(682.67)
    assert target_size(100, 50, (40, 40), only_if_larger=True) == (40, 20)    # ratio min(0.4, 0.8) < 1: both sides * 0.4
    assert target_size(333, 100, (100, 90), only_if_larger=True) == (100, 30)  # min(0.3003, 0.9): round(30.03)
    assert target_size(10, 20, (40, 40), only_if_larger=True) == (10, 20)     # ratio 2 >= 1: unchanged
    assert target_size(40, 80, (40, 100), only_if_larger=True) == (40, 80)    # ratio exactly 1: unchanged


needs_reference = pytest.mark.skipif(not os.path.isdir(REF_CONFIGS), reason="the reference checkout is absent")


@needs_reference
def test_ingest_plan_train():
    from refign_amd import config
    cfg = config.load_config(os.path.join(REF_CONFIGS, "cityscapes_acdc", "refign_daformer.yaml"))
    src = config.ingest_plan(cfg, "train", "Cityscapes")
    assert src["dims"] == (512, 1024) and src["crop_size"] == (512, 512) and src["cat_max_ratio"] == 0.75
    assert src["resize"] is None and src["flip"] == 0.5 and src["load_keys"] == ["image", "semantic"]
    assert src["mean"] == (0.485, 0.456, 0.406) and src["std"] == (0.229, 0.224, 0.225)
    trg = config.ingest_plan(cfg, "train", "ACDC")
    assert trg["dims"] == (540, 960) and trg["crop_size"] == (512, 512) and trg["cat_max_ratio"] == 1.0
    assert trg["load_keys"] == ["image", "image_ref"]
    assert set(src) >= {"dims", "resize", "img_only", "crop_size", "cat_max_ratio", "flip", "mean", "std", "load_keys"}


@needs_reference
def test_ingest_plan_eval_sections():
    from refign_amd import config
    cfg = config.load_config(os.path.join(REF_CONFIGS, "cityscapes_acdc", "refign_daformer.yaml"))
    val = config.ingest_plan(cfg, "val", "ACDC")
    assert val["dims"] == (540, 960) and val["resize"] is None and val["crop_size"] is None and val["flip"] == 0.0
    test = config.ingest_plan(cfg, "test", "ACDC")
    assert test["dims"] is None and test["resize"] == (540, 960) and test["img_only"] is True and test["crop_size"] is None
    pred = config.ingest_plan(cfg, "predict", "ACDC")
    assert pred["resize"] == (540, 960) and pred["img_only"] is False and pred["load_keys"] == ["image"]
    assert config.build(cfg["data"]) is cfg["data"]                   # data_modules.* specs still come back as specs


@needs_reference
def test_ingest_plan_refuses_what_it_does_not_cover():
    from refign_amd import config
    cfg = config.load_config(os.path.join(REF_CONFIGS, "megadepth", "uawarpc_stage1.yaml"))
    with pytest.raises(config.OutOfScopeError, match="ColorJitter"):
        config.ingest_plan(cfg, "train", "MegaDepth")


def test_library_exports_the_resize_entry_points():
    import ctypes

    import refign_amd
    from refign_amd import _lib
    lib = ctypes.CDLL(refign_amd.library_path())
    for s in ("rfn_resize_crop_flip_norm_u8", "rfn_resize_u8", "rfn_resize_nearest_u8"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert refign_amd.abi_version() == 5


def test_no_cpu_fallback():
    import torch
    from refign_amd import resample
    img, lbl = torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((8, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        resample.resize_u8(img, (4, 4))
    with pytest.raises(RuntimeError):
        resample.resize_nearest_u8(lbl, (4, 4))
    with pytest.raises(RuntimeError):
        resample.resize_crop_flip_normalize(img, (4, 4), 0, 0, 4, 4, False)

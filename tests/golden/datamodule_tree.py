"""tests/golden/datamodule_tree.py -- a tiny Cityscapes / ACDC / DarkZurich tree of PNG files, built from a recipe (names, sizes,
seeds), and the configurations the data module tests run over it.  make_golden_datamodule.py builds it to run the reference's
readers over it and stores the recipe next to what they found; the tests build the same tree again from that recipe."""
import os

import numpy as np

RECIPE = {
    "seed": 20240,
    "Cityscapes": {"size": [128, 256],
                   "train": {"aachen": ["aachen_000000_000019", "aachen_000001_000019", "aachen_000002_000019"],
                             "bochum": ["bochum_000000_000313", "bochum_000000_000600", "bochum_000000_000885"]},
                   "val": {"frankfurt": ["frankfurt_000000_000294", "frankfurt_000000_000576"]},
                   "test": {"berlin": ["berlin_000000_000019"]}},
    "ACDC": {"size": [108, 192],
             "train": {"fog": {"GOPR0475": ["GOPR0475_frame_000041", "GOPR0475_frame_000247", "GOPR0475_frame_000252"]},
                       "night": {"GOPR0351": ["GOPR0351_frame_000159", "GOPR0351_frame_000161"], "GP010376": ["GP010376_frame_000001"]},
                       "rain": {"GOPR0400": ["GOPR0400_frame_000216"]}, "snow": {"GOPR0122": ["GOPR0122_frame_000001"]}},
             "val": {"fog": {"GOPR0476": ["GOPR0476_frame_000115", "GOPR0476_frame_000301"]},
                     "night": {"GOPR0356": ["GOPR0356_frame_000321"]}, "rain": {"GOPR0402": ["GOPR0402_frame_000250"]},
                     "snow": {"GOPR0607": ["GOPR0607_frame_000112"]}},
             "test": {"fog": {"GOPR0477": ["GOPR0477_frame_000060"]}, "night": {"GOPR0364": ["GOPR0364_frame_000001"]},
                      "rain": {"GOPR0403": ["GOPR0403_frame_000021"]}, "snow": {"GOPR0606": ["GOPR0606_frame_000003"]}}},
    "DarkZurich": {"size": [108, 192],
                   # `night,day` lines: a made-up list in the format of the one the reference ships
                   "pairs": [["train/night/GOPR0351/GOPR0351_frame_000001", "train/day/GOPR0350/GOPR0350_frame_000011"],
                             ["train/night/GOPR0351/GOPR0351_frame_000002", "train/day/GOPR0350/GOPR0350_frame_000017"],
                             ["train/night/GP010376/GP010376_frame_000003", "train/day/GOPR0350/GOPR0350_frame_000011"]],
                   "val": {"GOPR0356": ["GOPR0356_frame_000321", "GOPR0356_frame_000339"]},
                   # test: the reference frame's name carries a suffix the night frame's does not: paired by prefix
                   "test": {"GOPR0364": [["GOPR0364_frame_000001", "GOPR0364_frame_000001_match_000093"],
                                         ["GOPR0364_frame_000002", "GOPR0364_frame_000002_match_000107"]]}},
}


def _image(rng, h, w):
    """smooth colour ramps plus noise, so that a resize has something to interpolate"""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 255 // max(h + w - 2, 1))], -1)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


def _label(rng, h, w):
    """16 x 16 blocks of classes 0..5 under one dominant class, a patch of a rarer class 11..13, some ignore pixels"""
    coarse = rng.integers(0, 6, (-(-h // 16), -(-w // 16)))
    coarse[rng.random(coarse.shape) < 0.4] = int(rng.integers(0, 3))
    lbl = np.repeat(np.repeat(coarse, 16, 0), 16, 1)[:h, :w].astype(np.uint8)
    for c in (11, 12, 13):
        if rng.random() < 0.7:
            y, x = int(rng.integers(0, h - 20)), int(rng.integers(0, w - 28))
            lbl[y:y + 10 + 2 * (c - 11), x:x + 24] = c
    lbl[rng.random((h, w)) < 0.03] = 255
    return lbl


def _save(arr, *path):
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.join(*path)), exist_ok=True)
    Image.fromarray(arr).save(os.path.join(*path))


def build_tree(data_dir, recipe=RECIPE):
    """writes <data_dir>/Cityscapes, /ACDC, /DarkZurich as the recipe says.  Files are written in sorted order from one seeded
    generator, so the same recipe gives the same bytes."""
    rng = np.random.default_rng(int(recipe["seed"]))
    cs, root = recipe["Cityscapes"], os.path.join(data_dir, "Cityscapes")
    for split in ("train", "val", "test"):
        for city, names in sorted(cs[split].items()):
            for n in names:
                _save(_image(rng, *cs["size"]), root, "leftImg8bit", split, city, n + "_leftImg8bit.png")
                _save(_label(rng, *cs["size"]), root, "gtFine", split, city, n + "_gtFine_labelTrainIds.png")
    ac, root = recipe["ACDC"], os.path.join(data_dir, "ACDC")
    for split in ("train", "val", "test"):
        for cond, recs in sorted(ac[split].items()):
            for rec, names in sorted(recs.items()):
                for n in names:
                    _save(_image(rng, *ac["size"]), root, "rgb_anon", cond, split, rec, n + "_rgb_anon.png")
                    _save(_image(rng, *ac["size"]), root, "rgb_anon", cond, split + "_ref", rec, n + "_rgb_ref_anon.png")
                    if split != "test":
                        _save(_label(rng, *ac["size"]), root, "gt", cond, split, rec, n + "_gt_labelTrainIds.png")
    dz, root = recipe["DarkZurich"], os.path.join(data_dir, "DarkZurich")
    os.makedirs(os.path.join(root, "gt"), exist_ok=True)
    for name in sorted({n for pair in dz["pairs"] for n in pair}):
        _save(_image(rng, *dz["size"]), root, "rgb_anon", name + "_rgb_anon.png")
    os.makedirs(os.path.join(root, "lists"), exist_ok=True)
    with open(os.path.join(root, "lists", "zurich_dn_pair_train.csv"), "w") as f:
        f.writelines(f"{night},{day}\n" for night, day in dz["pairs"])
    for rec, names in sorted(dz["val"].items()):
        for n in names:
            _save(_image(rng, *dz["size"]), root, "rgb_anon", "val", "night", rec, n + "_rgb_anon.png")
            _save(_image(rng, *dz["size"]), root, "rgb_anon", "val_ref", "day", rec + "_ref", n + "_ref_rgb_anon.png")
            _save(_label(rng, *dz["size"]), root, "gt", "val", "night", rec, n + "_gt_labelTrainIds.png")
    for rec, pairs in sorted(dz["test"].items()):
        for night, day in pairs:
            _save(_image(rng, *dz["size"]), root, "rgb_anon", "test", "night", rec, night + "_rgb_anon.png")
            _save(_image(rng, *dz["size"]), root, "rgb_anon", "test_ref", "day", rec + "_ref", day + "_rgb_anon.png")
    return data_dir


_PIPE = "data_modules.transforms."


def _transforms(crop=None, cat_max_ratio=None, resize=None, img_only=False):
    out = []
    if resize is not None:
        out.append({"class_path": _PIPE + "Resize", "init_args": {"size": list(resize), **({"img_only": True} if img_only else {})}})
    out.append({"class_path": _PIPE + "ToTensor"})
    if crop is not None:
        args = {"size": list(crop), **({"cat_max_ratio": cat_max_ratio} if cat_max_ratio is not None else {})}
        out += [{"class_path": _PIPE + "RandomCrop", "init_args": args}, {"class_path": _PIPE + "RandomHorizontalFlip"}]
    return out + [{"class_path": _PIPE + "ConvertImageDtype"}, {"class_path": _PIPE + "Normalize"}]


def data_section(target="ACDC", crop=(48, 48), cs_dims=(64, 128), trg_dims=(54, 96), batch_size=4, num_workers=0,
                 rcs_min_pixels=40):
    """a `data:` section in the layout of the reference's refign_daformer.yaml, at the tree's scale: load-time dims on every
    section but `test` (which reads at full size and halves the image alone) and a whole-sample Resize in `predict`"""
    half = [trg_dims[0], trg_dims[1]]
    return {"class_path": "data_modules.CombinedDataModule", "init_args": {
        "batch_size": batch_size, "num_workers": num_workers, "load_config": {
            "train": {"Cityscapes": {"rcs_enabled": True, "rcs_min_crop_ratio": 2.0, "rcs_min_pixels": rcs_min_pixels,
                                     "dims": list(cs_dims), "load_keys": ["image", "semantic"],
                                     "transforms": _transforms(crop, 0.75)},
                      target: {"dims": list(trg_dims), "load_keys": ["image", "image_ref"], "transforms": _transforms(crop)}},
            "val": {target: {"dims": list(trg_dims), "load_keys": ["image", "semantic"], "transforms": _transforms()}},
            "test": {target: {"dims": list(RECIPE[target]["size"]), "load_keys": ["image", "semantic"],
                              "transforms": _transforms(resize=half, img_only=True)}},
            "predict": {target: {"predict_on": "test", "dims": list(RECIPE[target]["size"]), "load_keys": ["image"],
                                 "transforms": _transforms(resize=half)}}}}}

"""tests/golden/robotcar_tree.py -- a tiny Cityscapes / RobotCar / DarkZurich / NighttimeDriving / BDD100kNight tree built from a
recipe (names, sizes, seeds), the `data:` sections the RobotCar and night-test data module tests run over it, and a stand-in for
`h5py` that reads the tree's stand-in correspondence files.  make_golden_robotcar.py builds the tree to run the reference's
readers over it and stores the recipe next to what they found; the tests build the same tree again from that recipe.

RobotCar's label files hold RAW ids (0 ... 33 and a few codes above 33), the other sets' train ids.  A correspondence file
<name>.mat of the tree is a JSON text {"im_i_path": ..., "im_j_path": ...}: real ones are MATLAB v7.3 (HDF5) files, which
nothing here can write or read; `standin_h5py()` gives the module whose File(path, 'r').items() yields the two names as the
(n, 1) arrays of character codes that h5py yields for a real file."""
import json
import os
import types

import numpy as np
from datamodule_tree import _image, _label, _save, _transforms

RECIPE = {
    "seed": 20241,
    "Cityscapes": {"size": [64, 128],
                   "train": {"aachen": ["aachen_000000_000019", "aachen_000001_000019", "aachen_000002_000019"],
                             "bochum": ["bochum_000000_000313", "bochum_000000_000600", "bochum_000000_000885"]}},
    "RobotCar": {"size": [64, 64],
                 "training": ["1417176458999821", "1417176462874112", "1417176499431672", "1417176510180327", "1417176522678315"],
                 "validation": ["1418133739491424", "1418133745990498", "1418133760113642"],
                 "testing": ["1418235225938102", "1418235290304728"],
                 "codes_above_33": [34, 40, 200, 255],
                 # im_i_path (image_ref), im_j_path (image), relative to RobotCar/images: made-up names in the real layout
                 "pairs": {"corr_000001.mat": ["overcast-reference/rear/1417176458999821.png", "night/rear/1418235225938102.png"],
                           "corr_000002.mat": ["overcast-reference/rear/1417176462874112.png", "dusk/rear/1424450252186877.png"],
                           "corr_000003.mat": ["overcast-reference/rear/1417176458999821.png", "rain/rear/1416908195781243.png"],
                           "corr_000004.mat": ["overcast-reference/rear/1417176499431672.png", "night/rear/1418235290304728.png"],
                           "corr_000005.mat": ["overcast-reference/rear/1417176510180327.png", "snow/rear/1423575002498862.png"]},
                 "other_files": ["readme.txt"]},
    "DarkZurich": {"size": [54, 96], "val": {"GOPR0356": ["GOPR0356_frame_000321", "GOPR0356_frame_000339"]}},
    "NighttimeDriving": {"size": [54, 96], "test": ["0_frame_0001", "0_frame_0047", "8_frame_0120"]},
    "BDD100kNight": {"size": [48, 80],
                     "list": ["images/10k/train/0a0c3694-4cc8b0e3.jpg", "images/10k/train/3d581db5-2564fb7e.jpg",
                              "images/10k/val/7d2f7975-e0c1c5a7.jpg"]},
}


def _raw_label(rng, h, w, above):
    """16 x 16 blocks of raw ids 0 ... 33, a stripe of codes outside the map"""
    coarse = rng.integers(0, 34, (-(-h // 16), -(-w // 16)))
    coarse[rng.random(coarse.shape) < 0.4] = 7                       # road: train id 0 dominates, as in a street scene
    lbl = np.repeat(np.repeat(coarse, 16, 0), 16, 1)[:h, :w].astype(np.uint8)
    for n, code in enumerate(above):
        lbl[2 + 3 * n:4 + 3 * n, 5:5 + 9] = code
    return lbl


def build_tree(data_dir, recipe=RECIPE):
    """writes the five data sets under <data_dir> as the recipe says, from one seeded generator, in a fixed order"""
    rng = np.random.default_rng(int(recipe["seed"]))
    cs, root = recipe["Cityscapes"], os.path.join(data_dir, "Cityscapes")
    for city, names in sorted(cs["train"].items()):
        for n in names:
            _save(_image(rng, *cs["size"]), root, "leftImg8bit", "train", city, n + "_leftImg8bit.png")
            _save(_label(rng, *cs["size"]), root, "gtFine", "train", city, n + "_gtFine_labelTrainIds.png")
    rc, root = recipe["RobotCar"], os.path.join(data_dir, "RobotCar")
    for folder in ("training", "validation", "testing"):
        for n in rc[folder]:
            _save(_image(rng, *rc["size"]), root, "segmented_images", folder, "imgs", n + ".png")
            _save(_raw_label(rng, *rc["size"], rc["codes_above_33"]), root, "segmented_images", folder, "annos", n + ".png")
    for rel in sorted({p for pair in rc["pairs"].values() for p in pair}):
        _save(_image(rng, *rc["size"]), root, "images", rel)
    os.makedirs(os.path.join(root, "correspondence_data"), exist_ok=True)
    for name, (ref, img) in sorted(rc["pairs"].items()):
        with open(os.path.join(root, "correspondence_data", name), "w") as f:
            json.dump({"im_i_path": ref, "im_j_path": img}, f)
    for name in rc["other_files"]:
        with open(os.path.join(root, "correspondence_data", name), "w") as f:
            f.write("not a correspondence file\n")
    dz, root = recipe["DarkZurich"], os.path.join(data_dir, "DarkZurich")
    for rec, names in sorted(dz["val"].items()):
        for n in names:
            _save(_image(rng, *dz["size"]), root, "rgb_anon", "val", "night", rec, n + "_rgb_anon.png")
            _save(_image(rng, *dz["size"]), root, "rgb_anon", "val_ref", "day", rec + "_ref", n + "_ref_rgb_anon.png")
            _save(_label(rng, *dz["size"]), root, "gt", "val", "night", rec, n + "_gt_labelTrainIds.png")
    nd, root = recipe["NighttimeDriving"], os.path.join(data_dir, "NighttimeDriving")
    for n in nd["test"]:
        _save(_image(rng, *nd["size"]), root, "leftImg8bit", "test", "night", n + "_leftImg8bit.png")
        _save(_label(rng, *nd["size"]), root, "gtCoarse_daytime_trainvaltest", "test", "night", n + "_gtCoarse_labelTrainIds.png")
    bd, root = recipe["BDD100kNight"], os.path.join(data_dir, "BDD100kNight")
    for line in bd["list"]:
        _, _, split, name = line.split("/")
        _save(_image(rng, *bd["size"]), root, "images", "10k", split, name)
        _save(_label(rng, *bd["size"]), root, "labels", "sem_seg", "masks", split, name.replace(".jpg", ".png"))
    return data_dir


def write_bdd_list(data_dir, recipe=RECIPE):
    """the tree's file list where the BDD100kNight reader looks for it (the user's copy of the list the reference ships)"""
    path = os.path.join(data_dir, "BDD100kNight", "lists", "images_trainval_night_correct_filenames.txt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.writelines(line + "\n" for line in recipe["BDD100kNight"]["list"])
    return path


def standin_h5py():
    """a module to put into sys.modules['h5py']: File(path, 'r').items() -> the (n, 1) arrays of character codes"""
    class File:
        def __init__(self, path, mode="r"):
            assert mode == "r"
            with open(path) as f:
                self._content = json.load(f)

        def items(self):
            return [(k, np.array([[ord(c)] for c in v], dtype=np.uint16)) for k, v in self._content.items()]

        def close(self):
            pass

    mod = types.ModuleType("h5py")
    mod.File = File
    return mod


_PIPE = "data_modules.transforms."


def _labelled_robotcar(crop, dims):
    """the labelled RobotCar section of refign_daformer.yaml at the tree's scale (cat_max_ratio next to init_args, as there)"""
    return {"load_keys": ["image", "semantic"], "dims": list(dims), "transforms": [
        {"class_path": _PIPE + "RandomRotation", "init_args": {"degrees": 10}}, {"class_path": _PIPE + "ToTensor"},
        {"class_path": _PIPE + "RandomCrop", "init_args": {"size": list(crop)}, "cat_max_ratio": 0.75},
        {"class_path": _PIPE + "ColorJitter", "init_args": {"brightness": 0.25, "contrast": 0.25, "saturation": 0.25, "hue": 0.1}},
        {"class_path": _PIPE + "RandomHorizontalFlip"}, {"class_path": _PIPE + "ConvertImageDtype"},
        {"class_path": _PIPE + "Normalize"}]}


def robotcar_section(crop=(48, 48), dims=(56, 56), cs_dims=(56, 112), batch_size=6, num_workers=0, ignore=True, rcs_min_pixels=40,
                     eval_dims=None):
    """a `data:` section in the layout of cityscapes_robotcar/refign_daformer.yaml: three training loaders (rare-class Cityscapes,
    labelled RobotCar, RobotCar pairs); val and test sections without a load-time `dims`, as there (the reader's own 1024 x 1024
    then applies), unless eval_dims names one"""
    plain = {"load_keys": ["image", "semantic"], "transforms": _transforms()}
    if eval_dims is not None:
        plain = dict(plain, dims=list(eval_dims))
    return {"class_path": "data_modules.CombinedDataModule", "init_args": {
        "batch_size": batch_size, "num_workers": num_workers, "ignore_every_second_semantic_training_batch": ignore,
        "load_config": {
            "train": {"Cityscapes": {"rcs_enabled": True, "rcs_min_crop_ratio": 2.0, "rcs_min_pixels": rcs_min_pixels,
                                     "dims": list(cs_dims), "load_keys": ["image", "semantic"], "transforms": _transforms(crop, 0.75)},
                      "RobotCar": [_labelled_robotcar(crop, dims),
                                   {"load_keys": ["image", "image_ref"], "dims": list(dims), "transforms": _transforms(crop)}]},
            "val": {"RobotCar": dict(plain)}, "test": {"RobotCar": dict(plain)}}}}


def night_test_section(dims=None):
    """the `test:` section of cityscapes_darkzurich/refign_hrda_star.yaml: three data sets, no Resize, no `dims` (the readers' own
    then apply) unless dims = {data set: (h, w)} names them"""
    def plain(name):
        sec = {"load_keys": ["image", "semantic"], "transforms": _transforms()}
        return sec if dims is None else dict(sec, dims=list(dims[name]))
    return {"class_path": "data_modules.CombinedDataModule", "init_args": {
        "batch_size": 2, "num_workers": 0,
        "load_config": {"test": {n: plain(n) for n in ("DarkZurich", "NighttimeDriving", "BDD100kNight")}}}}

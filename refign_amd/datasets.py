"""refign_amd/datasets.py -- the readers of the data sets behind the Cityscapes -> ACDC, Cityscapes -> Dark Zurich and
Cityscapes -> RobotCar configurations and of the night test sets (NighttimeDriving, BDD100kNight): which files a stage reads,
how an image is paired with its reference and its label map, and how a file becomes an array.  The semantics are the reference
readers' (data_modules/datasets/{cityscapes,acdc,darkzurich,robotcar,nighttimedriving,bdd100knight}.py), restated:

  * stage -> split: train -> train, val -> val, test -> val, predict -> test (ACDC / Dark Zurich: or `predict_on`); RobotCar has a
    test split of its own, the two night sets have nothing else;
  * the walk is `os.listdir` as it comes (the file system's order: `paths` are parallel lists, their order carries no meaning);
  * a missing folder is a RuntimeError;
  * `decode(index)` stops at the DECODED file: the load-time resize to `dims` is the device's job (`dims=` of the samplers in
    refign_amd/datastep.py, resample.EvalIngest), and so is everything after it.  `transforms` is accepted and ignored.

No reader opens a file before `decode` is called, none starts a process or a thread.
The matcher's two data sets (MegaDepth, RobotCarMatching) follow at the end, in a registry of their own (MATCHING_READERS)."""
import json
import os

import numpy as np

_MISSING = ('Dataset not found or incomplete: {} must hold the folders {} of the split asked for')
_STAGES = ("train", "val", "test", "predict")


def _listed(x):
    return [x] if isinstance(x, str) else list(x)


class _Reader:
    """what the readers share: parallel path lists, `len`, `filename`, `decode`"""
    orig_dims = None
    keys = ("image", "image_ref", "semantic")

    def _stage(self, stage, predict_on=None):
        if stage not in _STAGES:
            raise AssertionError(f"{type(self).__name__}: stage must be one of {_STAGES}, got {stage!r}")
        self.stage = stage
        # test runs on the val split; predict on the test split unless the section names another
        self.split = {"train": "train", "val": "val", "test": "val", "predict": predict_on or "test"}[stage]

    def _need(self, *dirs):
        if not all(os.path.isdir(d) for d in dirs):
            raise RuntimeError(_MISSING.format(self.root, " and ".join(os.path.relpath(d, self.root) for d in dirs)))

    def __len__(self):
        return len(next(iter(self.paths.values())))

    def _check_label(self, a, path):
        """a reader's own demands on a decoded label map, checked before it is copied anywhere"""

    def filename(self, index):
        return self.paths["image"][index].split("/")[-1]

    def decode(self, index, out=None):
        """{key: uint8 array} of the section's load_keys: images (H, W, 3) through `convert('RGB')`, label maps (H, W) as
        stored -- not resized.  out = {key: array of the decoded shape}: the pixels are written there (a pinned buffer)."""
        from PIL import Image
        sample = {}
        for k in self.load_keys:
            if k not in ("image", "image_ref", "semantic"):
                raise ValueError(f"{type(self).__name__}: invalid load_key {k!r}")
            with Image.open(self.paths[k][index]) as im:
                a = np.array(im.convert("RGB") if k != "semantic" else im)         # a copy: writable, as torch wants it
            if k == "semantic":
                self._check_label(a, self.paths[k][index])
            if a.dtype != np.uint8:
                raise ValueError(f"{self.paths[k][index]}: a uint8 file is required, got {a.dtype}")
            if out is not None and k in out:
                np.copyto(out[k], a)
                a = out[k]
            sample[k] = a
        return sample

    def size(self, index, key="image"):
        """(H, W) of a file from its header"""
        from PIL import Image
        with Image.open(self.paths[key][index]) as im:
            return im.size[1], im.size[0]


class Cityscapes(_Reader):
    """<root>/leftImg8bit/<split>/<city>/*_leftImg8bit.png with <root>/gtFine/<split>/<city>/*_gtFine_labelTrainIds.png.
    rcs_enabled: `rcs_classes`, `rcs_classprob` (fp32 numpy) and `indices_with_class` of rare-class sampling from
    <root>/sample_class_stats.json and <root>/samples_with_class.json (write_class_stats makes them)."""
    orig_dims = (1024, 2048)

    def __init__(self, root, stage="train", load_keys=("image", "semantic"), dims=(1024, 2048), transforms=None,
                 rcs_enabled=False, rcs_class_temp=0.01, rcs_min_crop_ratio=0.5, rcs_min_pixels=3000, **kwargs):
        self.root, self.dims = root, dims
        self._stage(stage)
        self.load_keys = _listed(load_keys)
        self.paths = {k: [] for k in self.load_keys}
        images, labels = os.path.join(root, "leftImg8bit", self.split), os.path.join(root, "gtFine", self.split)
        self._need(images, labels)
        for city in os.listdir(images):
            for name in os.listdir(os.path.join(images, city)):
                for k in self.load_keys:
                    if k == "image":
                        self.paths[k].append(os.path.join(images, city, name))
                    elif k == "semantic":
                        self.paths[k].append(os.path.join(labels, city,
                                                          name.replace("leftImg8bit.png", "gtFine_labelTrainIds.png")))
        self.rcs_enabled, self.rcs_class_temp = rcs_enabled, rcs_class_temp
        self.rcs_min_crop_ratio, self.rcs_min_pixels = rcs_min_crop_ratio, rcs_min_pixels
        if rcs_enabled:
            self.rcs_classes, self.rcs_classprob = rcs_class_probs(root, rcs_class_temp)
            with open(os.path.join(root, "samples_with_class.json")) as f:
                with_class = {int(c): v for c, v in json.load(f).items()}
            self.indices_with_class = {}
            for c in self.rcs_classes:
                self.indices_with_class[c] = [self.paths["semantic"].index(os.path.expandvars(file))
                                              for file, pixels in with_class[c] if pixels > rcs_min_pixels]
                assert len(self.indices_with_class[c]) > 0, f"Cityscapes: no file with more than {rcs_min_pixels} pixels of class {c}"


def rcs_class_probs(root, temperature):
    """-> (classes from the rarest to the most frequent, their sampling probabilities as fp32 numpy): the pixel counts of
    <root>/sample_class_stats.json summed per class, sorted by count, softmax((1 - frequency) / temperature) -- in torch, with
    the operations and their order as the reference has them (get_rcs_class_probs), so that the probabilities agree to the bit."""
    import torch
    with open(os.path.join(root, "sample_class_stats.json")) as f:
        stats = json.load(f)
    total = {}
    for entry in stats:
        for c, n in entry.items():
            if c != "file":
                total[int(c)] = total.get(int(c), 0) + n
    total = dict(sorted(total.items(), key=lambda item: item[1]))
    freq = torch.tensor(list(total.values()))
    freq = freq / torch.sum(freq)
    freq = 1 - freq
    freq = torch.softmax(freq / temperature, dim=-1)
    return list(total.keys()), freq.numpy()


class ACDC(_Reader):
    """<root>/rgb_anon/<condition>/<split>/<recording>/*_rgb_anon.png, its reference under <split>_ref with the file name's
    `rgb_anon` -> `rgb_ref_anon`, its labels under <root>/gt/... as *_gt_labelTrainIds.png."""
    orig_dims = (1080, 1920)

    def __init__(self, root, stage="train", condition=("fog", "night", "rain", "snow"), load_keys=("image_ref", "image", "semantic"),
                 dims=(1080, 1920), transforms=None, predict_on=None, **kwargs):
        self.root, self.dims = root, dims
        self._stage(stage, predict_on)
        self.condition, self.load_keys = _listed(condition), _listed(load_keys)
        self.paths = {k: [] for k in self.keys}
        images, labels = os.path.join(root, "rgb_anon"), os.path.join(root, "gt")
        self._need(images, labels)
        for cond in self.condition:
            parent = os.path.join(images, cond, self.split)
            for recording in os.listdir(parent):
                img_dir = os.path.join(parent, recording)
                for name in os.listdir(img_dir):
                    self.paths["image"].append(os.path.join(img_dir, name))
                    # the reference pairs them by str.replace on the directory's path; here on the part below the root only,
                    # so that a root whose own path holds the split's name pairs the same way
                    ref_dir = os.path.join(images, os.path.join(cond, self.split, recording).replace(self.split, self.split + "_ref"))
                    self.paths["image_ref"].append(os.path.join(ref_dir, name.replace("rgb_anon", "rgb_ref_anon")))
                    self.paths["semantic"].append(os.path.join(labels, cond, self.split, recording,
                                                               name.replace("rgb_anon.png", "gt_labelTrainIds.png")))


class DarkZurich(_Reader):
    """train: <root>/rgb_anon/<night>_rgb_anon.png with <root>/rgb_anon/<day>_rgb_anon.png for every `night,day` line of the
    pair list; no labels.  val / test: <root>/rgb_anon/<split>/night/<recording>/*_rgb_anon.png, the reference under
    <split>_ref/day/<recording>_ref -- val: the file name's `rgb_anon.png` -> `ref_rgb_anon.png`; test: the first file of that
    directory (as os.listdir gives them) that starts with the frame's prefix -- and the labels under <root>/gt/....
    pairs_csv: the list of training pairs, <root>/lists/zurich_dn_pair_train.csv when not given.  It is no part of this package:
    the reference ships it as data_modules/datasets/lists/zurich_dn_pair_train.csv (it comes from the DANNet / MGCDA projects)."""
    orig_dims = (1080, 1920)

    def __init__(self, root, stage="train", load_keys=("image_ref", "image"), dims=(1080, 1920), transforms=None,
                 predict_on=None, pairs_csv=None, **kwargs):
        self.root, self.dims = root, dims
        self._stage(stage, predict_on)
        self.load_keys = _listed(load_keys)
        if "semantic" in self.load_keys:
            assert self.split != "train", "DarkZurich: the training split has no annotations"
        self.paths = {k: [] for k in self.keys}
        images, labels = os.path.join(root, "rgb_anon"), os.path.join(root, "gt")
        self._need(images, labels)
        if self.split == "train":
            pairs_csv = pairs_csv or os.path.join(root, "lists", "zurich_dn_pair_train.csv")
            if not os.path.isfile(pairs_csv):
                raise FileNotFoundError(f"DarkZurich: the list of training pairs {pairs_csv} is missing (one `night,day` line per "
                                        f"pair; the reference ships it as data_modules/datasets/lists/zurich_dn_pair_train.csv: "
                                        f"copy it there or pass pairs_csv=)")
            with open(pairs_csv) as f:
                for line in f:
                    night, day = line.strip().split(",")
                    self.paths["image"].append(os.path.join(images, night + "_rgb_anon.png"))
                    self.paths["image_ref"].append(os.path.join(images, day + "_rgb_anon.png"))
            return
        parent = os.path.join(images, self.split, "night")
        for recording in os.listdir(parent):
            img_dir = os.path.join(parent, recording)
            # the reference's chain of str.replace, applied to the part of the path below the root only
            ref_dir = os.path.join(images, os.path.join(self.split, "night", recording).replace(self.split, self.split + "_ref")
                                   .replace("night", "day").replace(recording, recording + "_ref"))
            for name in os.listdir(img_dir):
                self.paths["image"].append(os.path.join(img_dir, name))
                if self.split == "val":
                    self.paths["image_ref"].append(os.path.join(ref_dir, name.replace("rgb_anon.png", "ref_rgb_anon.png")))
                elif self.split == "test":
                    start = name.split("rgb_anon.png")[0]
                    self.paths["image_ref"].append(os.path.join(ref_dir, next(f for f in os.listdir(ref_dir) if f.startswith(start))))
                self.paths["semantic"].append(os.path.join(labels, self.split, "night", recording,
                                                           name.replace("rgb_anon.png", "gt_labelTrainIds.png")))


ROBOTCAR_PAIRS_CSV = os.path.join("lists", "correspondence_pairs.csv")
# raw RobotCar label id -> train id (datasets/robotcar.py `id_to_trainid`, ids 0 ... 33; its key -1 never matches a uint8 pixel)
_ROBOTCAR_TRAIN_IDS = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13, 27: 14,
                       28: 15, 31: 16, 32: 17, 33: 18}


class RobotCar(_Reader):
    """Three forms (datasets/robotcar.py, restated):
      train with `semantic` among the load_keys: <root>/segmented_images/training/imgs/* with .../annos/<the same name>;
      train with image + image_ref: one pair per line `im_i_path,im_j_path` of <root>/lists/correspondence_pairs.csv, both
        relative to <root>/images; im_i_path is image_ref, im_j_path is image, `filename` the basename of im_j_path.  The
        reference reads the two names out of the MATLAB v7.3 files <root>/correspondence_data/*.mat with h5py, one file per
        sample, in the order of that directory's listing; write_robotcar_pairs(root) writes the CSV from them in that order.
        pairs_csv: another place for the list;
      val / test / predict: <root>/segmented_images/{validation,testing}/imgs with .../annos (predict reads testing); image_ref
        is refused, as the reference asserts.
    The label files hold RAW ids: decode returns them as stored (a 2-D uint8 array, or ValueError), and label_lut() is the table
    that makes train ids of them -- applied on the device (resample.resize_nearest_u8(lut=))."""
    orig_dims = (1024, 1024)

    def __init__(self, root, stage="train", load_keys=("image_ref", "image", "semantic"), dims=(1024, 1024), transforms=None,
                 pairs_csv=None, **kwargs):
        self.root, self.dims = root, dims
        if not os.path.isdir(root):
            raise RuntimeError(_MISSING.format(root, "segmented_images (and images, lists for the training pairs)"))
        if stage not in _STAGES:
            raise AssertionError(f"RobotCar: stage must be one of {_STAGES}, got {stage!r}")
        self.stage = stage
        self.split = {"train": "train", "val": "val", "test": "test", "predict": "test"}[stage]
        self.load_keys = _listed(load_keys)
        if self.split == "train" and "semantic" not in self.load_keys:
            self.paths = {"image": [], "image_ref": []}
            self.images_dir = os.path.join(root, "images")
            pairs_csv = pairs_csv or os.path.join(root, ROBOTCAR_PAIRS_CSV)
            if not os.path.isfile(pairs_csv):
                raise FileNotFoundError(f"RobotCar: the list of training pairs {pairs_csv} is missing (one `im_i_path,im_j_path` line "
                                        f"per file of correspondence_data/; datasets.write_robotcar_pairs(root) writes it from the "
                                        f".mat files and needs h5py for that)")
            with open(pairs_csv) as f:
                for line in f:
                    if line.strip():
                        ref, img = line.strip().split(",")
                        self.paths["image_ref"].append(os.path.join(self.images_dir, ref))
                        self.paths["image"].append(os.path.join(self.images_dir, img))
            return
        if self.split != "train":
            assert "image_ref" not in self.load_keys, "RobotCar: the val and test splits have no image_ref"
        folder = {"train": "training", "val": "validation", "test": "testing"}[self.split]
        images = os.path.join(root, "segmented_images", folder, "imgs")
        labels = os.path.join(root, "segmented_images", folder, "annos")
        self._need(images, labels)
        self.paths = {k: [] for k in self.load_keys}
        for name in os.listdir(images):
            for k in self.load_keys:
                if k == "image":
                    self.paths[k].append(os.path.join(images, name))
                elif k == "semantic":
                    self.paths[k].append(os.path.join(labels, name))

    def _check_label(self, a, path):
        if a.ndim != 2 or a.dtype != np.uint8:
            raise ValueError(f"{path}: a single-channel uint8 map of raw label ids is required, got {a.dtype} {a.shape}")

    @staticmethod
    def label_lut():
        """the 256-entry uint8 table of encode_semantic_map: ids 0 ... 33 to their train id or 255, every other code to itself
        (the reference leaves a code outside its map unchanged)"""
        lut = np.arange(256, dtype=np.uint8)
        lut[:34] = 255
        for raw, train in _ROBOTCAR_TRAIN_IDS.items():
            lut[raw] = train
        return lut


def write_robotcar_pairs(root, out_csv=None):
    """<root>/lists/correspondence_pairs.csv (or out_csv) from <root>/correspondence_data/*.mat: per file, in the order of the
    directory's listing filtered to names ending in `mat` (the reference's), one line `im_i_path,im_j_path` -- the two datasets of
    that name, (n, 1) arrays of character codes.  Needs h5py (the files are MATLAB v7.3, i.e. HDF5).  -> the number of lines."""
    try:
        import h5py
    except ImportError as e:
        raise ImportError("datasets.write_robotcar_pairs needs h5py to read the MATLAB v7.3 files under correspondence_data/ (it is "
                          "needed for this one conversion only; the RobotCar reader itself reads the CSV it writes)") from e
    corr_dir = os.path.join(root, "correspondence_data")
    if not os.path.isdir(corr_dir):
        raise RuntimeError(_MISSING.format(root, "correspondence_data"))
    lines = []
    for name in [fn for fn in os.listdir(corr_dir) if fn.endswith("mat")]:
        f = h5py.File(os.path.join(corr_dir, name), "r")
        try:
            content = {k: np.array(v) for k, v in f.items()}
        finally:
            if hasattr(f, "close"):
                f.close()
        pair = ["".join(chr(int(a[0])) for a in content[k]) for k in ("im_i_path", "im_j_path")]
        if any("," in p or "\n" in p for p in pair):
            raise ValueError(f"{name}: an image path with a comma or a line break cannot go into the list")
        lines.append(",".join(pair) + "\n")
    out_csv = out_csv or os.path.join(root, ROBOTCAR_PAIRS_CSV)
    os.makedirs(os.path.dirname(out_csv), exist_ok=True)
    with open(out_csv, "w") as f:
        f.writelines(lines)
    return len(lines)


class NighttimeDriving(_Reader):
    """test only: <root>/leftImg8bit/test/night/*_leftImg8bit.png with <root>/gtCoarse_daytime_trainvaltest/test/night/
    *_gtCoarse_labelTrainIds.png (datasets/nighttimedriving.py, restated)"""
    orig_dims = (1080, 1920)

    def __init__(self, root, stage="test", load_keys=("image", "semantic"), dims=(1080, 1920), transforms=None, **kwargs):
        self.root, self.dims = root, dims
        images, labels = os.path.join(root, "leftImg8bit"), os.path.join(root, "gtCoarse_daytime_trainvaltest")
        self._need(images, labels)
        assert stage == "test", f"NighttimeDriving: stage must be 'test', got {stage!r}"
        self.stage = self.split = "test"
        self.load_keys = _listed(load_keys)
        self.paths = {"image": [], "semantic": []}
        for name in os.listdir(os.path.join(images, "test", "night")):
            self.paths["image"].append(os.path.join(images, "test", "night", name))
            self.paths["semantic"].append(os.path.join(labels, "test", "night",
                                                       name.replace("leftImg8bit.png", "gtCoarse_labelTrainIds.png")))


class BDD100kNight(_Reader):
    """test only: every line `a/b/<split>/<name>.jpg` of the file list gives <root>/images/10k/<split>/<name>.jpg with
    <root>/labels/sem_seg/masks/<split>/<name>.png (datasets/bdd100knight.py, restated).
    file_list: <root>/lists/images_trainval_night_correct_filenames.txt when not given.  It is no part of this package: the
    reference ships it as data_modules/datasets/lists/images_trainval_night_correct_filenames.txt."""
    orig_dims = (720, 1280)
    LIST = "images_trainval_night_correct_filenames.txt"

    def __init__(self, root, stage="test", load_keys=("image", "semantic"), dims=(720, 1280), transforms=None, file_list=None,
                 **kwargs):
        self.root, self.dims = root, dims
        if not os.path.isdir(root):
            raise RuntimeError(_MISSING.format(root, "images/10k and labels/sem_seg/masks"))
        assert stage == "test", f"BDD100kNight: stage must be 'test', got {stage!r}"
        self.stage = self.split = "test"
        self.load_keys = _listed(load_keys)
        file_list = file_list or os.path.join(root, "lists", self.LIST)
        if not os.path.isfile(file_list):
            raise FileNotFoundError(f"BDD100kNight: the file list {file_list} is missing (one `a/b/<split>/<name>.jpg` line per "
                                    f"image; the reference ships it as data_modules/datasets/lists/{self.LIST}: copy it there or "
                                    f"pass file_list=)")
        self.paths = {"image": [], "semantic": []}
        with open(file_list) as f:
            for line in f:
                _, _, split, name = line.strip().split("/")
                self.paths["image"].append(os.path.join(root, "images", "10k", split, name))
                self.paths["semantic"].append(os.path.join(root, "labels", "sem_seg", "masks", split, name.replace(".jpg", ".png")))


# READERS: the three data sets of the Cityscapes -> ACDC / -> Dark Zurich training configurations, as before.  MORE_READERS: the
# RobotCar configurations' data set and the two night test sets.  SEGMENTATION_READERS, both together, is the registry that
# SegmentationDataModule reads; the matcher's two data sets (below) stay in a registry of their own.
READERS = {"Cityscapes": Cityscapes, "ACDC": ACDC, "DarkZurich": DarkZurich}
MORE_READERS = {"RobotCar": RobotCar, "NighttimeDriving": NighttimeDriving, "BDD100kNight": BDD100kNight}
SEGMENTATION_READERS = {**READERS, **MORE_READERS}


def write_class_stats(root, out_dir=None, device=None, num_classes=19):
    """The rare-class tables of a Cityscapes tree from the *_labelTrainIds.png files of its train split that are already there
    (making those from the polygon files needs cityscapesscripts and is not done here):
      sample_class_stats.json       [{class: pixels, ..., "file": label file}] -- classes with no pixel left out
      sample_class_stats_dict.json  {label file: {class: pixels}}
      samples_with_class.json       {class: [[label file, pixels], ...]}
    in `out_dir` (the root when not given).  device: the counts come from datastep.device_label_hists, one whole-image box per
    file; None: from numpy.  -> the list written to the first file."""
    labels = os.path.join(root, "gtFine", "train")
    if not os.path.isdir(labels):
        raise RuntimeError(_MISSING.format(root, "gtFine/train"))
    out_dir = out_dir or root
    os.makedirs(out_dir, exist_ok=True)
    files = sorted(os.path.join(d, f) for d, _, names in os.walk(labels) for f in names if f.endswith("_labelTrainIds.png"))
    from PIL import Image
    stats = []
    for path in files:
        with Image.open(path) as im:
            lbl = np.ascontiguousarray(np.asarray(im))
        if lbl.dtype != np.uint8 or lbl.ndim != 2:
            raise ValueError(f"{path}: a single-channel uint8 label map is required")
        if device is None:
            hist = np.bincount(lbl.ravel(), minlength=256)
        else:
            import torch
            from .datastep import device_label_hists
            hist = device_label_hists(torch.from_numpy(lbl).to(device), [(0, 0, lbl.shape[0], lbl.shape[1])])[0]
        entry = {int(c): int(hist[c]) for c in range(num_classes) if hist[c] > 0}
        entry["file"] = path
        stats.append(entry)
    with open(os.path.join(out_dir, "sample_class_stats.json"), "w") as f:
        json.dump(stats, f, indent=2)
    by_file = {e["file"]: {c: n for c, n in e.items() if c != "file"} for e in stats}
    with open(os.path.join(out_dir, "sample_class_stats_dict.json"), "w") as f:
        json.dump(by_file, f, indent=2)
    with_class = {}
    for file, counts in by_file.items():
        for c, n in counts.items():
            with_class.setdefault(c, []).append((file, n))
    with open(os.path.join(out_dir, "samples_with_class.json"), "w") as f:
        json.dump(with_class, f, indent=2)
    return stats


# ---------------------------------------------------------------------------------------------------------------------------
# The matcher's two data sets (data_modules/datasets/{megadepth,robotcarmatching}.py, restated).  They are NOT in READERS:
# SegmentationDataModule keeps refusing them; datamodule.MatchingDataModule reads them through MATCHING_READERS.
def _read_pairs_csv(path):
    """the rows of test1600Pairs.csv / test6511.csv as dicts of strings (the reference reads them with pandas, dtype=str)"""
    import csv
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def _floats(text):
    return np.array(list(map(float, text.split(";")))).astype(np.float32)


class _PairReader:
    """what the two matching readers share: the CSV form of a sample, `filename`, `pair_paths`, `sizes`, `decode`.
    decode(index, exchange=False, out=None) -> {"image_ref", "image": uint8 (H, W, 3) as stored; "corr_pts_ref", "corr_pts":
    fp32 (n, 2) (x, y) in the pixels of the stored files; "exchange": bool}.  Neither the images nor the points are brought to
    `dims`: the resize and the points' scaling (dims[1] / w, dims[0] / h) belong to the place that resizes (resample.EvalIngest,
    MatchingDataModule's training path)."""
    keys = ("image_ref", "image")

    def _csv_sample(self, index):
        row = self.rows[index]
        scene = "." if row["scene"] == "/" else row["scene"]
        pts = np.stack((_floats(row["XB"]), _floats(row["YB"])), axis=1)          # of the target image: corr_pts
        pts_ref = np.stack((_floats(row["XA"]), _floats(row["YA"])), axis=1)      # of the source image: corr_pts_ref
        return os.path.join(scene, row["source_image"]), os.path.join(scene, row["target_image"]), pts_ref, pts

    def filename(self, index):
        return self.pair_paths(index)[1].split("/")[-1]

    def pair_paths(self, index, exchange=False):
        """(image_ref's path, image's path) below `images_dir`"""
        ref, img = self._sample(index)[:2]
        return (img, ref) if exchange else (ref, img)

    def sizes(self, index, exchange=False):
        """{key: (H, W)} of the two files, from their headers"""
        from PIL import Image
        out = {}
        for k, rel in zip(self.keys, self.pair_paths(index, exchange)):
            with Image.open(os.path.join(self.images_dir, rel)) as im:
                out[k] = (im.size[1], im.size[0])
        return out

    def decode(self, index, exchange=False, out=None):
        from PIL import Image
        ref, img, pts_ref, pts = self._sample(index)
        if exchange:
            ref, img, pts_ref, pts = img, ref, pts, pts_ref
        sample = {}
        for k, rel in (("image_ref", ref), ("image", img)):
            with Image.open(os.path.join(self.images_dir, rel)) as im:
                a = np.array(im.convert("RGB"))
            if out is not None and k in out:
                np.copyto(out[k], a)
                a = out[k]
            sample[k] = a
        sample.update(corr_pts_ref=np.array(pts_ref, dtype=np.float32), corr_pts=np.array(pts, dtype=np.float32),
                      exchange=bool(exchange))
        return sample


class MegaDepth(_PairReader):
    """stage -> split: train -> train, val -> val, test / predict -> test; debug: train_debug whatever the stage.
    test: <root>/Test/test1600Pairs.csv (scene, source_image, target_image, XA / YA / XB / YB as `;`-separated floats) with the
    images under <root>/Test/test1600Pairs; image_ref is the source image.
    train / val: for every scene of the split's list, <root>/scene_info/<scene>.0.npz (image_paths, depth_paths,
    points3D_id_to_2D, overlap_matrix); images without a path or a depth map are dropped, the pairs with an overlap in (0.3, 1.0]
    are the candidates, at most `*_num_per_scene` of them are kept per scene (RandomState(400).choice(len(pairs), num,
    replace=False)) and the list of all scenes' items is shuffled once (RandomState(400).shuffle).  An item's points are the 2-D
    positions of the 3-D points both images see, in the iteration order of `keys() & keys()`.
    store_scene_info_in_memory: the scenes' tables are kept and an item is (scene, i, j, overlap), resolved when it is read;
    otherwise an item is the resolved bundle.  `item(index)` gives the bundle in both forms.
    The scene lists are <lists_dir>/{train,train_debug,validation,test}_scenes_MegaDepth.txt, <root>/lists when not given.  They
    are no part of this package: the reference ships them as data_modules/datasets/lists/*_scenes_MegaDepth.txt.
    len: the reference returns 30000 for `train` whatever the number of items and would index past the end of a shorter list;
    here it is min(30000, len(items)).
    The coin `random.random() < exchange_images_with_proba` of a two-view sample is NOT thrown here: decode(index, exchange=)
    takes the decision from the caller, who draws it on the thread that owns the stream."""
    cfg = {"train_split": "train_scenes_MegaDepth.txt", "train_debug_split": "train_debug_scenes_MegaDepth.txt",
           "val_split": "validation_scenes_MegaDepth.txt", "test_split": "test_scenes_MegaDepth.txt",
           "train_debug_num_per_scene": 10, "train_num_per_scene": 300, "val_num_per_scene": 25,
           "min_overlap_ratio": 0.3, "max_overlap_ratio": 1.0}
    TRAIN_LEN = 30000

    def __init__(self, root, stage="train", load_keys=("image_ref", "image", "image_prime"), dims=None,
                 exchange_images_with_proba=0, store_scene_info_in_memory=False, debug=False, transforms=None, lists_dir=None):
        self.root, self.dims, self.exchange_images_with_proba = root, dims, exchange_images_with_proba
        if stage not in _STAGES:
            raise AssertionError(f"MegaDepth: stage must be one of {_STAGES}, got {stage!r}")
        self.stage = stage
        self.split = "train_debug" if debug else {"train": "train", "val": "val", "test": "test", "predict": "test"}[stage]
        self.load_keys = _listed(load_keys)
        if self.split == "test":
            assert "image_prime" not in self.load_keys, "MegaDepth: the test split has no image_prime"
            assert self.exchange_images_with_proba == 0, "MegaDepth: the test split does not exchange its images"
            self.rows = _read_pairs_csv(os.path.join(root, "Test", "test1600Pairs.csv"))
            self.images_dir = os.path.join(root, "Test", "test1600Pairs")
            return
        self.images_dir = root
        self.scene_info_path = os.path.join(root, "scene_info")
        name = self.cfg[self.split + "_split"]
        path = os.path.join(lists_dir or os.path.join(root, "lists"), name)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"MegaDepth: the scene list {path} is missing (scene names separated by white space; the "
                                    f"reference ships it as data_modules/datasets/lists/{name}: copy it there or pass lists_dir=)")
        with open(path) as f:
            self.scenes = f.read().split()
        if not ("image_ref" in self.load_keys and "image" in self.load_keys):
            raise NotImplementedError(f"MegaDepth: load_keys {self.load_keys}: the single-view form is not read here (image_ref "
                                      f"and image together are what the matcher trains and validates on)")
        self.store_scene_info_in_memory = bool(store_scene_info_in_memory)
        self.items = []
        if self.store_scene_info_in_memory:
            self.save_scene_info()
        self.sample_new_items()

    def _info(self, scene, **kw):
        path = os.path.join(self.scene_info_path, "%s.0.npz" % scene)
        return np.load(path, allow_pickle=True, **kw) if os.path.exists(path) else None

    def _tables(self, info):
        """-> (paths, points3D_id_to_2D, overlap matrix) of the images that have a path and a depth map, [N, 2] candidate pairs"""
        valid = ((info["image_paths"] != None) & (info["depth_paths"] != None))  # noqa: E711  (element-wise, object arrays)
        mat = info["overlap_matrix"][valid][:, valid]
        pairs = (mat > self.cfg["min_overlap_ratio"]) & (mat <= self.cfg["max_overlap_ratio"])
        return info["image_paths"][valid], info["points3D_id_to_2D"][valid], mat, np.stack(np.where(pairs), -1)

    def save_scene_info(self):
        self.images, self.points3D_id_to_2D, self.pairs = {}, {}, {}
        for scene in self.scenes:
            info = self._info(scene)
            if info is None:
                continue
            paths, points, mat, pairs = self._tables(info)
            self.images[scene], self.points3D_id_to_2D[scene] = paths.copy(), points.copy()
            self.pairs[scene] = [(i, j, mat[i, j]) for i, j in pairs]

    @staticmethod
    def _bundle(paths, points, idx1, idx2):
        matches = np.array(list(points[idx1].keys() & points[idx2].keys()))
        return {"image_path1": paths[idx1], "image_path2": paths[idx2],
                "2d_matches_1": [np.array(points[idx1][m], dtype=np.float32).reshape(1, 2) for m in matches],
                "2d_matches_2": [np.array(points[idx2][m], dtype=np.float32).reshape(1, 2) for m in matches]}

    def sample_new_items(self, seed=400):
        self.items = []
        num = self.cfg[self.split + "_num_per_scene"]
        for scene in self.scenes:
            if self.store_scene_info_in_memory:
                if scene not in self.pairs:
                    continue
                pairs = np.array(self.pairs[scene])
                if len(pairs) > num:
                    pairs = pairs[np.random.RandomState(seed).choice(len(pairs), num, replace=False)]
                self.items.extend((scene, int(i), int(j), k) for i, j, k in pairs)
            else:
                info = self._info(scene, mmap_mode="r")
                if info is None:
                    continue
                paths, points, _, pairs = self._tables(info)
                if len(pairs) > num:
                    pairs = pairs[np.random.RandomState(seed).choice(len(pairs), num, replace=False)]
                self.items.extend(self._bundle(paths, points, pairs[n, 0], pairs[n, 1]) for n in range(len(pairs)))
        if "debug" in self.split:
            import copy
            orig = copy.deepcopy(self.items)
            for _ in range(10):
                self.items = self.items + copy.deepcopy(orig)
        np.random.RandomState(seed).shuffle(self.items)

    def __len__(self):
        if self.split == "test":
            return len(self.rows)
        return min(self.TRAIN_LEN, len(self.items)) if self.split == "train" else len(self.items)

    def item(self, index):
        """the pair bundle {image_path1, image_path2, 2d_matches_1, 2d_matches_2} of a train / val item, in either form"""
        it = self.items[index]
        if isinstance(it, dict):
            return it
        scene, idx1, idx2, _ = it
        return self._bundle(self.images[scene], self.points3D_id_to_2D[scene], idx1, idx2)

    def _sample(self, index):
        if self.split == "test":
            return self._csv_sample(index)
        it = self.item(index)
        cat = lambda parts: np.concatenate(parts, axis=0) if parts else np.zeros((0, 2), np.float32)  # noqa: E731
        return it["image_path1"], it["image_path2"], cat(it["2d_matches_1"]), cat(it["2d_matches_2"])

    def decode(self, index, exchange=False, out=None):
        if exchange and self.split == "test":
            raise AssertionError("MegaDepth: the test split does not exchange its images")
        return super().decode(index, exchange, out)


class RobotCarMatching(_PairReader):
    """<root>/test6511.csv (the columns of MegaDepth's test file) with the images under <root>/images; stages test and predict.
    dims and resize_filter are kept for the caller (the reader's own default dims are (1024, 1024), Lanczos)."""

    def __init__(self, root, stage="test", load_keys=("image_ref", "image"), dims=(1024, 1024), resize_filter="lanczos",
                 transforms=None, **kwargs):
        self.root, self.dims, self.resize_filter = root, dims, resize_filter
        assert stage in ["test", "predict"], f"RobotCarMatching: stage must be 'test' or 'predict', got {stage!r}"
        self.stage, self.load_keys = stage, _listed(load_keys)
        for k in self.load_keys:
            if k not in self.keys:
                raise ValueError(f"RobotCarMatching: invalid load_key {k!r}")
        if not os.path.isdir(root):
            raise RuntimeError(_MISSING.format(root, "images"))
        self.rows = _read_pairs_csv(os.path.join(root, "test6511.csv"))
        self.images_dir = os.path.join(root, "images")

    def __len__(self):
        return len(self.rows)

    def _sample(self, index):
        return self._csv_sample(index)

    def decode(self, index, exchange=False, out=None):
        if exchange:
            raise AssertionError("RobotCarMatching does not exchange its images")
        return super().decode(index, False, out)


MATCHING_READERS = {"MegaDepth": MegaDepth, "RobotCarMatching": RobotCarMatching}

"""CPU: the RobotCar, NighttimeDriving and BDD100kNight readers over a tiny tree (tests/golden/robotcar_tree.py, rebuilt from the
recipe in tests/golden/robotcar_ref.json) against what the reference's own three classes found there
(tests/golden/make_golden_robotcar.py); RobotCar's code table and the numpy restatement of encode + NEAREST resize against the
reference's encode_semantic_map; the pair list's writer under a stand-in h5py; the refusals; the config plans of the shipped
RobotCar and Dark Zurich configurations.  A directory's listing order is the file system's: path lists are compared as sets of
tuples, the pair list's order against the listing of THIS tree."""
import json
import os
import sys

import numpy as np
import pytest
from robotcar_tree import build_tree, night_test_section, robotcar_section, standin_h5py, write_bdd_list

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_CONFIGS = "/root/reference/configs"
needs_reference = pytest.mark.skipif(not os.path.isdir(REF_CONFIGS), reason="the reference checkout is absent")


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLDEN, "robotcar_ref.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tree(tmp_path_factory, ref):
    from refign_amd import datasets
    data_dir = str(tmp_path_factory.mktemp("rc"))
    build_tree(data_dir, ref["recipe"])
    write_bdd_list(data_dir, ref["recipe"])
    had = sys.modules.get("h5py")
    sys.modules["h5py"] = standin_h5py()
    try:
        assert datasets.write_robotcar_pairs(os.path.join(data_dir, "RobotCar")) == len(ref["recipe"]["RobotCar"]["pairs"])
    finally:
        if had is None:
            del sys.modules["h5py"]
        else:
            sys.modules["h5py"] = had
    return data_dir


CASES = [("RobotCar", "train|labelled", "train", {"load_keys": ["image", "semantic"]}),
         ("RobotCar", "train|pairs", "train", {"load_keys": ["image", "image_ref"]}),
         ("RobotCar", "val", "val", {"load_keys": ["image", "semantic"]}),
         ("RobotCar", "test", "test", {"load_keys": ["image", "semantic"]}),
         ("RobotCar", "predict", "predict", {"load_keys": ["image"]}),
         ("NighttimeDriving", "test", "test", {}), ("BDD100kNight", "test", "test", {})]


@pytest.mark.parametrize("name,key,stage,kwargs", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_readers_find_what_the_reference_finds(tree, ref, name, key, stage, kwargs):
    from refign_amd import datasets
    want = ref["readers"][name]["stages"][key]
    root = os.path.join(tree, name)
    ds = datasets.SEGMENTATION_READERS[name](root, stage=stage, **kwargs)
    assert len(ds) == want["len"] and ds.split == want["split"] and list(ds.load_keys) == want["load_keys"]
    assert list(ds.orig_dims) == ref["readers"][name]["orig_dims"] and list(ds.dims) == ref["readers"][name]["default_dims"]
    got = {(ds.filename(i),) + tuple(os.path.relpath(ds.paths[k][i], root) for k in ds.load_keys) for i in range(len(ds))}
    assert got == {(s["filename"],) + tuple(s["opened"][k] for k in want["load_keys"]) for s in want["samples"]}
    assert len(got) == want["len"]
    s = ds.decode(0)
    h, w = ref["recipe"][name]["size"]
    assert set(s) == set(ds.load_keys) and ds.size(0) == (h, w)
    assert all(a.dtype == np.uint8 and a.shape == ((h, w) if k == "semantic" else (h, w, 3)) for k, a in s.items())
    if key == "train|pairs":
        # the CSV follows the listing of correspondence_data filtered to *.mat, in this file system's order
        listing = [f for f in os.listdir(os.path.join(root, "correspondence_data")) if f.endswith("mat")]
        assert sorted(listing) == sorted(want["corr_files"]) and len(listing) == len(ds)
        pairs = ref["recipe"]["RobotCar"]["pairs"]
        for i, f in enumerate(listing):
            assert os.path.relpath(ds.paths["image_ref"][i], os.path.join(root, "images")) == pairs[f][0]
            assert os.path.relpath(ds.paths["image"][i], os.path.join(root, "images")) == pairs[f][1]
            assert ds.filename(i) == pairs[f][1].split("/")[-1]


def test_label_table_and_restatement_equal_the_reference_encode(ref):
    from refign_amd.datasets import RobotCar
    from refign_amd.resample import nearest_table, resize_nearest_reference
    want = np.array(ref["encode_semantic_map"]["output"], dtype=np.uint8)
    lut = RobotCar.label_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256,) and np.array_equal(lut, want)
    assert np.array_equal(lut[34:], np.arange(34, 256)) and set(lut[:34].tolist()) == set(range(19)) | {255}
    codes = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(resize_nearest_reference(codes, (16, 16), lut=lut), want.reshape(16, 16))
    # encode, then Pillow's NEAREST: the order the reader has them in
    from PIL import Image
    enc = Image.fromarray(want.reshape(16, 16)).resize((7, 11), resample=Image.NEAREST)
    assert np.array_equal(resize_nearest_reference(codes, (11, 7), lut=lut), np.asarray(enc))
    assert np.array_equal(resize_nearest_reference(codes, (11, 7)), codes[nearest_table(16, 11)][:, nearest_table(16, 7)])
    with pytest.raises(ValueError, match="256-element uint8"):
        resize_nearest_reference(codes, (4, 4), lut=np.arange(255, dtype=np.uint8))


def test_robotcar_labels_must_be_single_channel_uint8(tree, tmp_path):
    from PIL import Image
    from refign_amd.datasets import RobotCar
    root = tmp_path / "RobotCar"
    for sub in ("imgs", "annos"):
        (root / "segmented_images" / "validation" / sub).mkdir(parents=True)
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(root / "segmented_images" / "validation" / "imgs" / "a.png")
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(root / "segmented_images" / "validation" / "annos" / "a.png")
    ds = RobotCar(str(root), stage="val", load_keys=["image", "semantic"])
    with pytest.raises(ValueError, match=r"annos/a\.png"):
        ds.decode(0)
    ok = RobotCar(os.path.join(tree, "RobotCar"), stage="val", load_keys=["image", "semantic"])
    raw = ok.decode(0)["semantic"]
    with Image.open(ok.paths["semantic"][0]) as im:
        assert np.array_equal(raw, np.asarray(im))                 # raw ids as stored: nothing is encoded on the host
    assert raw.max() > 33 and ((raw > 18) & (raw < 34)).any()


def test_pair_list_writer_and_its_messages(tree, ref, tmp_path, monkeypatch):
    from refign_amd import datasets
    root = os.path.join(tree, "RobotCar")
    pairs = ref["recipe"]["RobotCar"]["pairs"]
    listing = [f for f in os.listdir(os.path.join(root, "correspondence_data")) if f.endswith("mat")]
    with open(os.path.join(root, "lists", "correspondence_pairs.csv")) as f:
        assert f.read().splitlines() == [",".join(pairs[name]) for name in listing]
    monkeypatch.setitem(sys.modules, "h5py", standin_h5py())
    out = tmp_path / "elsewhere" / "pairs.csv"
    assert datasets.write_robotcar_pairs(root, str(out)) == len(pairs)
    assert datasets.RobotCar(root, load_keys=["image", "image_ref"], pairs_csv=str(out)).paths == \
        datasets.RobotCar(root, load_keys=["image", "image_ref"]).paths
    # without h5py: an ImportError that says what the function needs (None in sys.modules makes the import fail)
    monkeypatch.setitem(sys.modules, "h5py", None)
    with pytest.raises(ImportError, match="write_robotcar_pairs needs h5py"):
        datasets.write_robotcar_pairs(root, str(out))
    # a tree without the CSV: FileNotFoundError naming the function; the labelled and the val forms do not need the list
    bare = tmp_path / "RobotCar"
    bare.mkdir()
    with pytest.raises(FileNotFoundError, match="write_robotcar_pairs"):
        datasets.RobotCar(str(bare), stage="train", load_keys=["image", "image_ref"])
    with pytest.raises(AssertionError, match="image_ref"):
        datasets.RobotCar(root, stage="val", load_keys=["image", "image_ref"])
    assert ref["readers"]["RobotCar"]["val_refuses_image_ref"]


def test_missing_lists_and_folders(tree, tmp_path):
    from refign_amd import datasets
    for name in ("RobotCar", "NighttimeDriving", "BDD100kNight"):
        with pytest.raises(RuntimeError, match="not found or incomplete"):
            datasets.SEGMENTATION_READERS[name](str(tmp_path / "nowhere"), stage="test")
    bare = tmp_path / "BDD100kNight"
    bare.mkdir()
    with pytest.raises(FileNotFoundError, match="data_modules/datasets/lists/images_trainval_night_correct_filenames.txt"):
        datasets.BDD100kNight(str(bare))
    pkg = os.path.dirname(datasets.__file__)
    assert not any("images_trainval_night" in f or "correspondence_pairs" in f for _, _, files in os.walk(pkg) for f in files)
    for cls in (datasets.NighttimeDriving, datasets.BDD100kNight):
        with pytest.raises(AssertionError, match="stage must be 'test'"):
            cls(os.path.join(tree, cls.__name__), stage="val")


def test_the_flag_needs_a_second_labelled_section(tree):
    from refign_amd import config
    from refign_amd.datamodule import SegmentationDataModule
    from refign_amd.datasets import write_class_stats
    write_class_stats(os.path.join(tree, "Cityscapes"))
    sec = robotcar_section(batch_size=4)
    train = sec["init_args"]["load_config"]["train"]
    train["RobotCar"] = train["RobotCar"][1:]                        # the pairs alone: one labelled source
    dm = SegmentationDataModule({"data": sec}, tree, "cpu")
    assert dm.ignore_every_second_semantic_training_batch and dm.train_on == ["Cityscapes", "RobotCar"]
    with pytest.raises(ValueError, match="can only ignore in semi-supervised case"):
        dm.train_batches()
    with pytest.raises(config.OutOfScopeError, match="ignore_every_second_semantic_training_batch"):
        dm.train_batches()
    # a data set the configuration names and the user does not hold: the section is named, with the way round it
    import tempfile
    with tempfile.TemporaryDirectory() as empty:
        with pytest.raises(config.OutOfScopeError, match=r"NighttimeDriving \(test\).*datasets="):
            SegmentationDataModule({"data": night_test_section()}, empty, "cpu").loaders("test", datasets=["NighttimeDriving"])
    # the full recipe parses as the reference parses it; a shape outside the three-loader recipe is refused by name
    dm = SegmentationDataModule({"data": robotcar_section()}, tree, "cpu")
    assert dm.train_on == ["Cityscapes", "RobotCar", "RobotCar"] and dm.batch_size == 6 and dm.val_batch_size == 1
    assert dm.idx_to_name["train"] == {0: "Cityscapes", 1: "RobotCar", 2: "RobotCar"}
    assert dm.orig_dims == {"Cityscapes": (1024, 2048), "RobotCar": (1024, 1024)}         # the data sets the configuration names
    with pytest.raises(RuntimeError, match="HIP device"):
        dm.train_batches()
    night = SegmentationDataModule({"data": night_test_section()}, tree, "cpu")
    assert sorted(night.loaders("test")) == ["BDD100kNight", "DarkZurich", "NighttimeDriving"]
    assert night.orig_dims == {"DarkZurich": (1080, 1920), "NighttimeDriving": (1080, 1920), "BDD100kNight": (720, 1280)}
    assert isinstance(config.OutOfScopeError("x"), Exception)


ROBOTCAR_YAMLS = ["refign_daformer", "refign_deeplabv2"]


@needs_reference
@pytest.mark.parametrize("name", ROBOTCAR_YAMLS)
def test_plans_of_the_shipped_robotcar_configurations(name):
    from refign_amd import config
    from refign_amd.datamodule import _one_section_cfg, _sections
    cfg = config.load_config(os.path.join(REF_CONFIGS, "cityscapes_robotcar", name + ".yaml"))
    args = cfg["data"]["init_args"]
    assert args["ignore_every_second_semantic_training_batch"] is True and args["batch_size"] == 6
    secs = _sections(args["load_config"], "train")
    assert [n for n, _ in secs] == ["Cityscapes", "RobotCar", "RobotCar"]
    plans = [config.train_section_plan(_one_section_cfg("train", n, conf), n) for n, conf in secs]
    # the same through the list form the function documents
    assert plans[1] == config.train_section_plan(cfg, "RobotCar", 0) and plans[2] == config.train_section_plan(cfg, "RobotCar", 1)
    assert plans[0] == config.train_section_plan(cfg, "Cityscapes")
    assert [p["load_keys"] for p in plans] == [["image", "semantic"], ["image", "semantic"], ["image", "image_ref"]]
    assert [p["crop_size"] for p in plans] == [(512, 512)] * 3 and [p["flip"] for p in plans] == [0.5] * 3
    assert [p["dims"] for p in plans] == [(512, 1024), (720, 720), (720, 720)]
    assert plans[0]["cat_max_ratio"] == 0.75 and plans[0]["rotation"] is None and plans[0]["jitter"] is None
    assert plans[1]["rotation"] == {"degrees": (-10.0, 10.0)} and plans[1]["cat_max_ratio"] == 1.0    # next to init_args: dropped
    assert plans[1]["jitter"]["hue"] == (-0.1, 0.1) and plans[1]["jitter"]["brightness"] == (0.75, 1.25)
    assert plans[2]["rotation"] is None and plans[2]["jitter"] is None
    for split in ("val", "test"):
        plan = config.ingest_plan(cfg, split, "RobotCar")
        assert plan["dims"] is None and plan["resize"] is None and plan["load_keys"] == ["image", "semantic"]
    metric = cfg["model"]["init_args"]["metrics"]["test"]["RobotCar"][0]["init_args"]
    assert metric["over_present_classes"] is True


@needs_reference
@pytest.mark.parametrize("name", ["refign_daformer", "refign_hrda_star", "refign_deeplabv2"])
def test_ingest_plans_of_the_three_night_test_sections(name):
    from refign_amd import config
    cfg = config.load_config(os.path.join(REF_CONFIGS, "cityscapes_darkzurich", name + ".yaml"))
    assert list(cfg["data"]["init_args"]["load_config"]["test"]) == ["DarkZurich", "NighttimeDriving", "BDD100kNight"]
    for ds in ("DarkZurich", "NighttimeDriving", "BDD100kNight"):
        plan = config.ingest_plan(cfg, "test", ds)
        # refign_hrda_star tests at full size; the other two halve the image alone (Resize(img_only=True)), for all three sets
        assert (plan["resize"], plan["img_only"]) == ((None, False) if name == "refign_hrda_star" else ((540, 960), True))
        assert plan["dims"] is None and plan["pad"] is None and plan["crop_size"] is None
        assert plan["load_keys"] == ["image", "semantic"] and plan["dims_interpolation"] == "bilinear"

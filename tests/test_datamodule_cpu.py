"""CPU: the readers of refign_amd/datasets.py against what the reference's readers found in the same tiny tree
(tests/golden/datamodule_ref.json, made by tests/golden/make_golden_datamodule.py; the tree is built again here from the recipe
stored in it), SegmentationDataModule's reading of `data.init_args`, its refusals, write_class_stats, the epoch permutation and
the command line of refign_amd.run.  Path lists are compared as sets: the order of os.listdir belongs to the file system."""
import copy
import json
import os
import random

import numpy as np
import pytest
import torch
from datamodule_tree import build_tree, data_section

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "datamodule_ref.json")) as _f:
    REF = json.load(_f)
REF_CONFIGS = "/root/reference/configs"


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from refign_amd.datasets import write_class_stats
    data_dir = str(tmp_path_factory.mktemp("dm"))
    build_tree(data_dir, REF["recipe"])
    write_class_stats(os.path.join(data_dir, "Cityscapes"))
    return data_dir


def _cases():
    for name, rec in REF["readers"].items():
        for key in rec["stages"]:
            yield name, key


def _kwargs(key):
    stage, *rest = key.split("|")
    return stage, dict(kv.split("=") for kv in rest)


def _triples(ds, root):
    rel = lambda p: os.path.relpath(p, root)  # noqa: E731
    return {tuple(rel(ds.paths[k][i]) if ds.paths.get(k) else None for k in ("image", "image_ref", "semantic")) for i in range(len(ds))}


@pytest.mark.parametrize("name,key", list(_cases()))
def test_reader_finds_the_reference_readers_files(tree, name, key):
    from refign_amd import datasets
    want = REF["readers"][name]["stages"][key]
    stage, kwargs = _kwargs(key)
    if "rcs_classes" in want:
        kwargs.update(rcs_enabled=True, rcs_min_pixels=40)
    root = os.path.join(tree, name)
    ds = datasets.READERS[name](root, stage=stage, **kwargs)
    assert ds.split == want["split"] and len(ds) == want["len"] and len(want["triples"]) == want["len"]
    assert _triples(ds, root) == {tuple(t) for t in want["triples"]}
    assert list(ds.orig_dims) == REF["readers"][name]["orig_dims"]
    assert ds.filename(0) == os.path.basename(ds.paths["image"][0])
    for k in ds.load_keys:                                    # every file a section would decode is in the tree
        if k == "semantic" and ds.split == "test":
            continue
        assert all(os.path.isfile(p) for p in ds.paths[k]), (k, ds.paths[k])


def test_stage_to_split_and_predict_on(tree):
    from refign_amd.datasets import ACDC, Cityscapes, DarkZurich
    for cls in (Cityscapes, ACDC, DarkZurich):
        root = os.path.join(tree, cls.__name__)
        keys = {"load_keys": ["image"]} if cls is DarkZurich else {}
        assert [cls(root, stage=s, **keys).split for s in ("train", "val", "test", "predict")] == ["train", "val", "val", "test"]
    assert ACDC(os.path.join(tree, "ACDC"), stage="predict", predict_on="val").split == "val"
    assert DarkZurich(os.path.join(tree, "DarkZurich"), stage="predict", predict_on="val").split == "val"
    assert ACDC(os.path.join(tree, "ACDC"), stage="val", predict_on="test").split == "val"      # read in `predict` only
    with pytest.raises(AssertionError):
        ACDC(os.path.join(tree, "ACDC"), stage="fit")


def test_rare_class_tables_equal_the_reference(tree):
    from refign_amd.datasets import Cityscapes
    want = REF["readers"]["Cityscapes"]["stages"]["train"]
    root = os.path.join(tree, "Cityscapes")
    ds = Cityscapes(root, stage="train", rcs_enabled=True, rcs_min_pixels=40, transforms="ignored")
    assert [int(c) for c in ds.rcs_classes] == want["rcs_classes"]
    assert ds.rcs_classprob.dtype == np.float32
    assert ds.rcs_classprob.tolist() == np.asarray(want["rcs_classprob"], dtype=np.float32).tolist()      # the same torch operations
    got = {str(c): sorted(os.path.relpath(ds.paths["semantic"][i], root) for i in idx) for c, idx in ds.indices_with_class.items()}
    assert got == want["files_with_class"]
    with pytest.raises(AssertionError):                       # the non-empty assertion
        Cityscapes(root, stage="train", rcs_enabled=True, rcs_min_pixels=10 ** 6)


def test_rare_class_file_names_go_through_expandvars(tree, tmp_path, monkeypatch):
    from refign_amd.datasets import Cityscapes
    root = os.path.join(tree, "Cityscapes")
    plain = Cityscapes(root, stage="train", rcs_enabled=True, rcs_min_pixels=40)
    alt = tmp_path / "Cityscapes"
    alt.mkdir()
    for sub in ("leftImg8bit", "gtFine"):
        os.symlink(os.path.join(root, sub), alt / sub)
    for name in ("sample_class_stats.json", "samples_with_class.json"):
        with open(os.path.join(root, name)) as f:
            (alt / name).write_text(f.read().replace(root, "$RFN_TEST_CS_ROOT"))
    monkeypatch.setenv("RFN_TEST_CS_ROOT", str(alt))
    ds = Cityscapes(str(alt), stage="train", rcs_enabled=True, rcs_min_pixels=40)
    names = lambda d: {c: sorted(d.filename(i) for i in idx) for c, idx in d.indices_with_class.items()}  # noqa: E731
    assert names(ds) == names(plain)


def test_dark_zurich_pairs(tree, tmp_path):
    from refign_amd.datasets import DarkZurich
    root = os.path.join(tree, "DarkZurich")
    ds = DarkZurich(root, stage="train", load_keys=["image", "image_ref"])
    want = [(os.path.join(root, "rgb_anon", n + "_rgb_anon.png"), os.path.join(root, "rgb_anon", d + "_rgb_anon.png"))
            for n, d in REF["recipe"]["DarkZurich"]["pairs"]]
    assert list(zip(ds.paths["image"], ds.paths["image_ref"])) == want and len(ds) == 3 and ds.paths["semantic"] == []
    assert all(os.path.isfile(p) for pair in want for p in pair)
    with pytest.raises(AssertionError, match="no annotations"):
        DarkZurich(root, stage="train", load_keys=["image", "semantic"])
    # another list, by keyword
    other = tmp_path / "pairs.csv"
    other.write_text("a/b,c/d\n")
    ds = DarkZurich(root, stage="train", pairs_csv=str(other))
    assert ds.paths["image"] == [os.path.join(root, "rgb_anon", "a/b_rgb_anon.png")]
    # test split: the reference frame is the first file of the _ref directory that starts with the night frame's prefix
    ds = DarkZurich(root, stage="predict", load_keys=["image", "image_ref"])
    assert len(ds) == 2
    for img, ref in zip(ds.paths["image"], ds.paths["image_ref"]):
        assert os.path.basename(ref).startswith(os.path.basename(img).split("rgb_anon.png")[0]) and os.path.isfile(ref)
        assert os.path.dirname(ref).endswith(os.path.join("rgb_anon", "test_ref", "day", "GOPR0364_ref"))


def test_decode_returns_the_file_as_it_is(tree):
    from PIL import Image
    from refign_amd.datasets import ACDC
    ds = ACDC(os.path.join(tree, "ACDC"), stage="val", load_keys=["image", "image_ref", "semantic"], dims=(54, 96))
    s = ds.decode(1)
    h, w = REF["recipe"]["ACDC"]["size"]
    assert s["image"].shape == s["image_ref"].shape == (h, w, 3) and s["semantic"].shape == (h, w)         # not resized
    assert all(v.dtype == np.uint8 for v in s.values())
    assert np.array_equal(s["image_ref"], np.asarray(Image.open(ds.paths["image_ref"][1]).convert("RGB")))
    assert np.array_equal(s["semantic"], np.asarray(Image.open(ds.paths["semantic"][1])))
    out = {"image": np.zeros((h, w, 3), np.uint8)}
    t = ds.decode(1, out)
    assert t["image"] is out["image"] and np.array_equal(out["image"], s["image"])
    assert ds.size(1) == (h, w)


def test_refusals(tree, tmp_path):
    from refign_amd import config, datasets
    from refign_amd.datamodule import SegmentationDataModule
    for cls in datasets.READERS.values():
        with pytest.raises(RuntimeError, match="not found or incomplete"):
            cls(str(tmp_path / "nowhere"), stage="val")
    # the list of training pairs is no part of the package
    bare = tmp_path / "DarkZurich"
    (bare / "rgb_anon").mkdir(parents=True)
    (bare / "gt").mkdir()
    with pytest.raises(FileNotFoundError, match="data_modules/datasets/lists/zurich_dn_pair_train.csv"):
        datasets.DarkZurich(str(bare), stage="train")
    assert not any("zurich_dn_pair" in f for _, _, files in os.walk(os.path.dirname(datasets.__file__)) for f in files)
    # data sets without a reader: refused when the section is asked for, not at construction
    sec = data_section("DarkZurich")
    lc = sec["init_args"]["load_config"]
    lc["test"]["NighttimeDriving"] = copy.deepcopy(lc["test"]["DarkZurich"])
    lc["val"]["MegaDepth"] = copy.deepcopy(lc["val"]["DarkZurich"])
    dm = SegmentationDataModule({"data": sec}, tree, "cpu")
    assert dm.test_on == ["DarkZurich", "NighttimeDriving"]
    with pytest.raises(config.OutOfScopeError, match=r"NighttimeDriving \(test\)"):
        dm.loaders("test")
    with pytest.raises(config.OutOfScopeError, match=r"MegaDepth \(val\)"):
        dm.loaders("val")
    assert list(dm.loaders("test", datasets=["DarkZurich"])) == ["DarkZurich"]
    assert list(dm.loaders("predict")) == ["DarkZurich"]
    sec = data_section("ACDC")
    sec["init_args"]["load_config"]["train"]["RobotCar"] = [copy.deepcopy(sec["init_args"]["load_config"]["train"]["ACDC"])]
    sec["init_args"]["batch_size"] = 6
    dm = SegmentationDataModule({"data": sec}, tree, "cpu")
    assert dm.train_on == ["Cityscapes", "ACDC", "RobotCar"]
    with pytest.raises(config.OutOfScopeError, match=r"RobotCar \(train\)"):
        dm.train_batches()
    sec = data_section("ACDC")
    sec["init_args"]["ignore_every_second_semantic_training_batch"] = True
    dm = SegmentationDataModule({"data": sec}, tree, "cpu")
    with pytest.raises(config.OutOfScopeError, match="ignore_every_second_semantic_training_batch"):
        dm.train_batches()
    with pytest.raises(ValueError):
        dm.loaders("train")
    with pytest.raises(RuntimeError, match="HIP device"):       # and no quiet CPU path
        SegmentationDataModule({"data": data_section("ACDC")}, tree, "cpu").train_batches()


def test_module_parses_the_data_section(tree):
    from refign_amd.datamodule import MAX_WORKERS, SegmentationDataModule
    sec = data_section("ACDC", batch_size=8, num_workers=64)
    sec["init_args"]["batch_size_divisor"] = 2
    lc = sec["init_args"]["load_config"]
    lc["val"]["DarkZurich"] = [copy.deepcopy(lc["val"]["ACDC"])]                   # a list under a data set: its sections
    dm = SegmentationDataModule({"data": sec}, tree, "cpu")
    assert (dm.batch_size, dm.val_batch_size, dm.test_batch_size) == (4, 1, 1)
    assert dm.train_on == ["Cityscapes", "ACDC"] and dm.val_on == ["ACDC", "DarkZurich"]
    assert dm.idx_to_name == {"train": {0: "Cityscapes", 1: "ACDC"}, "val": {0: "ACDC", 1: "DarkZurich"}, "test": {0: "ACDC"},
                              "predict": {0: "ACDC"}}
    assert dm.num_workers == MAX_WORKERS == 16 and dm.prefetch == 2
    assert SegmentationDataModule({"data": data_section("ACDC")}, tree, "cpu").prefetch == 0
    assert dm.orig_dims == {"Cityscapes": (1024, 2048), "ACDC": (1080, 1920), "DarkZurich": (1080, 1920)}
    loaders = dm.loaders("val")
    assert list(loaders) == ["ACDC", "DarkZurich"] and len(loaders["ACDC"]) == 5 and len(loaders["DarkZurich"]) == 2
    dm.close()
    odd = data_section("ACDC", batch_size=3)
    with pytest.raises(AssertionError, match="divisible by number of train datasets"):
        SegmentationDataModule({"data": odd}, tree, "cpu")
    # config.build / config.resolve keep their hands off data_modules.* (tests/test_config_cpu.py pins it; restated for the module)
    from refign_amd import config
    assert config.build(sec) is sec
    with pytest.raises(config.OutOfScopeError):
        config.resolve("data_modules.CombinedDataModule")


def test_write_class_stats_counts_and_round_trips(tree, tmp_path):
    from PIL import Image
    from refign_amd.datasets import Cityscapes, write_class_stats
    root = os.path.join(tree, "Cityscapes")
    out = tmp_path / "stats"
    stats = write_class_stats(root, str(out))
    train = Cityscapes(root, stage="train")
    assert {e["file"] for e in stats} == set(train.paths["semantic"])
    for e in stats:
        lbl = np.asarray(Image.open(e["file"]))
        brute = {}
        for v in lbl.ravel().tolist():
            if v < 19:
                brute[v] = brute.get(v, 0) + 1
        assert {k: v for k, v in e.items() if k != "file"} == brute
    with open(out / "sample_class_stats.json") as f:
        listed = json.load(f)
    with open(out / "sample_class_stats_dict.json") as f:
        by_file = json.load(f)
    with open(out / "samples_with_class.json") as f:
        with_class = json.load(f)
    assert by_file == {e["file"]: {c: n for c, n in e.items() if c != "file"} for e in listed}
    assert {c: sorted(map(tuple, v)) for c, v in with_class.items()} == {
        c: sorted((file, n[c]) for file, n in by_file.items() if c in n) for c in {c for n in by_file.values() for c in n}}
    # the files the tree fixture wrote with the root as out_dir are what Cityscapes(rcs_enabled=True) reads
    for name in ("sample_class_stats.json", "samples_with_class.json"):
        with open(out / name) as a, open(os.path.join(root, name)) as b:
            assert json.load(a) == json.load(b)
    ds = Cityscapes(root, stage="train", rcs_enabled=True, rcs_min_pixels=40)
    for c, idx in ds.indices_with_class.items():
        assert sorted(ds.paths["semantic"][i] for i in idx) == sorted(f for f, n in by_file.items() if n.get(str(c), 0) > 40)


@pytest.mark.parametrize("n", [1, 7, 2975])
def test_epoch_order_is_random_samplers(n):
    from torch.utils.data import RandomSampler
    from refign_amd.datamodule import epoch_permutation
    torch.manual_seed(1234)
    want = [list(RandomSampler(range(n))) for _ in range(2)]
    tail = torch.rand(3)
    torch.manual_seed(1234)
    got = [epoch_permutation(n) for _ in range(2)]              # two successive epochs
    assert got == want and torch.equal(torch.rand(3), tail)     # and the global stream stands where the sampler leaves it
    assert n < 3 or got[0] != got[1]


def test_run_arguments_and_set_edits(tmp_path, monkeypatch):
    import yaml
    from refign_amd import run
    cfg = {"seed_everything": 3, "trainer": {"max_steps": 40000, "callbacks": [{"class_path": "helpers.callbacks.ValEveryNSteps",
                                                                                 "init_args": {"every_n_steps": 4000}}]},
           "model": {"init_args": {"backbone": {"init_args": {"model_type": "mit_b5", "pretrained": "cityscapes"}}}}}
    out = run.apply_set(copy.deepcopy(cfg), ["trainer.precision=16", "trainer.max_steps=2", "trainer.callbacks.0.init_args.every_n_steps=1",
                                             "model.init_args.backbone.init_args.pretrained=null",
                                             "model.init_args.head.init_args.in_channels=[32, 64, 160, 256]",
                                             "model.init_args.backbone.init_args.model_type=mit_b0", "trainer.deterministic=true"])
    assert out["trainer"]["precision"] == 16 and out["trainer"]["max_steps"] == 2 and out["trainer"]["deterministic"] is True
    assert out["trainer"]["callbacks"][0]["init_args"]["every_n_steps"] == 1
    assert out["model"]["init_args"]["backbone"]["init_args"] == {"model_type": "mit_b0", "pretrained": None}
    assert out["model"]["init_args"]["head"]["init_args"]["in_channels"] == [32, 64, 160, 256]
    with pytest.raises(ValueError, match="dotted.key=value"):
        run.apply_set({}, ["trainer.precision"])
    a = run.parse_args(["fit", "--config", "x.yaml", "--data_dir", "/d", "--set", "a.b=1", "--set", "c=2", "--ckpt_path", "p"])
    assert (a.command, a.config, a.data_dir, a.edits, a.ckpt_path, a.save_dir) == ("fit", "x.yaml", "/d", ["a.b=1", "c=2"], "p", None)
    with pytest.raises(SystemExit):
        run.parse_args(["train", "--config", "x.yaml", "--data_dir", "/d"])
    with pytest.raises(SystemExit):
        run.parse_args(["fit", "--data_dir", "/d"])
    # seeded as seed_everything seeds; and nothing is built off a HIP device
    path = tmp_path / "c.yaml"
    path.write_text(yaml.safe_dump(cfg))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP device"):
        run.main(["validate", "--config", str(path), "--data_dir", "/d", "--set", "seed_everything=11"])
    got = (random.random(), float(np.random.rand()), float(torch.rand(())))
    random.seed(11); np.random.seed(11); torch.manual_seed(11)
    assert got == (random.random(), float(np.random.rand()), float(torch.rand(())))


@pytest.mark.parametrize("name", sorted(REF["configs"]))
def test_reference_yaml_parses_into_the_reference_sections(name):
    from refign_amd import config
    from refign_amd.datamodule import SegmentationDataModule
    path = os.path.join(REF_CONFIGS, name)
    if not os.path.isfile(path):
        pytest.skip("the reference's configs are not on this machine")
    want = REF["configs"][name]
    dm = SegmentationDataModule(config.load_config(path), "/nowhere", "cpu")
    for k in ("train_on", "val_on", "test_on", "predict_on", "batch_size", "val_batch_size", "test_batch_size"):
        assert getattr(dm, k) == want[k], k
    assert {s: {str(i): n for i, n in d.items()} for s, d in dm.idx_to_name.items()} == want["idx_to_name"]
    assert dm.num_workers == 4 and dm.prefetch == 2

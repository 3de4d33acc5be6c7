"""CPU: the matcher's readers (datasets.MegaDepth / RobotCarMatching) against what the reference's readers made of the same tiny
tree (tests/golden/matching_ref.json, written by make_golden_matching.py; the tree is rebuilt here from the recipe stored in
it), config.matching_train_plan on the two shipped training sections and its refusals, and the command line's new flag.
Everything is compared exactly: item lists in their order, paths, points bit for bit (JSON holds the fp32 values as doubles)."""
import copy
import json
import os
import random

import numpy as np
import pytest
from matching_tree import LIST_FILES, build_tree, data_section

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"train": ("train", False), "val": ("val", False), "debug": ("train", True)}
KEYS = ["image_ref", "image"]


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLDEN, "matching_ref.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tree(ref, tmp_path_factory):
    return build_tree(str(tmp_path_factory.mktemp("match")), ref["recipe"])


def _f32(rows):
    return np.asarray(rows, dtype=np.float32).reshape(-1, 2)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()


def _megadepth(tree, stage, debug=False, **kw):
    from refign_amd.datasets import MegaDepth
    return MegaDepth(os.path.join(tree, "MegaDepth"), stage=stage, load_keys=KEYS, debug=debug, **kw)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("in_memory", [True, False])
def test_items_equal_the_reference(ref, tree, case, in_memory):
    """the item list in its order after the shuffle, in both storage forms; len (train: min(30000, items), see the reader)"""
    stage, debug = CASES[case]
    want = ref["megadepth"][case]["in_memory" if in_memory else "on_demand"]
    ds = _megadepth(tree, stage, debug, store_scene_info_in_memory=in_memory)
    got = [[b["image_path1"], b["image_path2"], len(b["2d_matches_1"])] for b in (ds.item(i) for i in range(len(ds.items)))]
    assert got == want["items"] and len(ds.items) == want["n_items"]
    assert isinstance(ds.items[0], tuple if in_memory else dict)
    if case == "train":
        assert want["len"] == 30000 and len(ds) == min(30000, want["n_items"]) == 12      # the one deviation
    else:
        assert len(ds) == want["len"]
    assert {"val": 28, "debug": 110, "train": 12}[case] == want["n_items"]                # 25 of 27 + 3; 10 x 11; 3 + 9


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("in_memory", [True, False])
def test_samples_equal_the_reference(ref, tree, case, in_memory):
    """paths and points of decode(i, exchange=) bit for bit; the points at `dims` through EvalIngest's reader-side rule"""
    from refign_amd.resample import EvalIngest
    stage, debug = CASES[case]
    ds = _megadepth(tree, stage, debug, store_scene_info_in_memory=in_memory)
    ingest = EvalIngest(dims=tuple(ref["dims"]), dims_interpolation="lanczos")
    samples = ref["megadepth"][case]["in_memory"]["samples"]
    assert len(samples) >= 6
    for key, want in samples.items():
        i, exchange = (int(v) for v in key.split("|"))
        assert list(ds.pair_paths(i, bool(exchange))) == [want["image_ref"], want["image"]]
        s = ds.decode(i, exchange=bool(exchange))
        assert set(s) == {"image_ref", "image", "corr_pts_ref", "corr_pts", "exchange"} and s["exchange"] is bool(exchange)
        sizes = ds.sizes(i, bool(exchange))
        for k in KEYS:
            assert s[k].dtype == np.uint8 and s[k].shape == (*sizes[k], 3)
        assert s["corr_pts"].shape[0] == s["corr_pts_ref"].shape[0] > 0
        for k, img in (("corr_pts_ref", "image_ref"), ("corr_pts", "image")):
            assert _same_bits(s[k], _f32(want[k])), (key, k)
            assert _same_bits(ingest.points(s[k], *sizes[img]).numpy(), _f32(want[k + "_dims"])), (key, k, "dims")
    plain, swapped = ds.decode(0), ds.decode(0, exchange=True)
    assert np.array_equal(plain["image"], swapped["image_ref"]) and _same_bits(plain["corr_pts_ref"], swapped["corr_pts"])


def test_valid_mask_and_overlap_window(ref, tree):
    """the image without a path and the one without a depth map never appear; (0.3, 1.0]: the pair at exactly 0.3 is out, the
    pairs at exactly 1.0 are in"""
    ds = _megadepth(tree, "train", store_scene_info_in_memory=True)
    pairs = {(ds.item(i)["image_path1"], ds.item(i)["image_path2"]) for i in range(len(ds.items))}
    used = {p for pair in pairs for p in pair}
    name = lambda scene, k: f"Undistorted_SfM/{scene}/images/{scene}_{k:02d}.jpg"  # noqa: E731
    assert None not in used and name("9001", 1) not in used and name("9005", 3) not in used
    scenes = ref["recipe"]["scenes"]
    assert scenes["9001"]["overlap"][0][3] == 0.3 and scenes["9001"]["overlap"][2][0] == 1.0
    assert (name("9001", 0), name("9001", 3)) not in pairs
    assert (name("9001", 2), name("9001", 0)) in pairs
    assert (name("9001", 3), name("9001", 0)) not in pairs                                 # 0.29
    assert scenes["9005"]["overlap"][1][4] == 0.3 and (name("9005", 1), name("9005", 4)) not in pairs
    assert (name("9005", 4), name("9005", 1)) in pairs                                     # 0.30000001
    assert (name("9005", 0), name("9005", 4)) in pairs and (name("9005", 4), name("9005", 0)) in pairs   # 1.0 both ways
    assert not any("9099" in p for p in used)                                              # listed, no info file: passed over


def test_exchange_coin_is_the_callers(ref, tree):
    """The reader throws no coin.  Thrown by the caller once per sample -- also at probability 0 -- the decisions and the stream's
    next value are the reference's."""
    from refign_amd.datamodule import _exchange_coin
    want = ref["megadepth"]["exchange"]
    ds = _megadepth(tree, "val", store_scene_info_in_memory=True, exchange_images_with_proba=want["proba"])
    random.seed(ref["seed"])
    state = random.getstate()
    ds.decode(0), ds.decode(1, exchange=True), ds.item(2), len(ds)
    assert random.getstate() == state
    got = [_exchange_coin(random, ds.exchange_images_with_proba) for _ in range(len(ds))]
    assert got == want["exchanged"] and True in got and False in got
    assert random.random() == want["next"]
    zero = _megadepth(tree, "val", store_scene_info_in_memory=True)
    random.seed(ref["seed"])
    assert [_exchange_coin(random, zero.exchange_images_with_proba) for _ in range(3)] == [False] * 3
    assert random.random() == want["next_after_3_at_proba_0"]


@pytest.mark.parametrize("name", ["MegaDepth", "RobotCarMatching"])
def test_csv_readers(ref, tree, name):
    """scene `/` -> `.`, XB / YB are corr_pts (the target image's) and XA / YA corr_pts_ref, len; points at dims"""
    from refign_amd.datasets import MATCHING_READERS
    from refign_amd.resample import EvalIngest
    want = ref["megadepth"]["test"] if name == "MegaDepth" else ref["robotcar"]
    ds = MATCHING_READERS[name](os.path.join(tree, name), stage="test", load_keys=KEYS)
    assert len(ds) == want["len"] == 3
    ingest = EvalIngest(dims=tuple(ref["dims"]), dims_interpolation="lanczos")
    recipe = ref["recipe"]["MegaDepthTest" if name == "MegaDepth" else name]
    for i, row in enumerate(want["rows"]):
        assert list(ds.pair_paths(i)) == [row["image_ref"], row["image"]]
        s = ds.decode(i)
        assert s["exchange"] is False
        for k in KEYS:
            assert list(s[k].shape) == row["sizes"][k] + [3] and s[k].dtype == np.uint8
            assert list(ds.sizes(i)[k]) == row["sizes"][k]
        for k, img in (("corr_pts_ref", "image_ref"), ("corr_pts", "image")):
            assert _same_bits(s[k], _f32(row[k])), (i, k)
            assert _same_bits(ingest.points(s[k], *row["sizes"][img]).numpy(), _f32(row[k + "_dims"])), (i, k, "dims")
        assert row["sizes"]["image_ref"] == recipe[i][2] and row["sizes"]["image"] == recipe[i][4]
        assert s["corr_pts"].shape == (recipe[i][5], 2)
        assert ds.filename(i) == recipe[i][3]
    assert want["rows"][1]["image_ref"] == "./" + recipe[1][1]                              # the row of scene `/`
    with open(os.path.join(tree, name, "Test/test1600Pairs.csv" if name == "MegaDepth" else "test6511.csv")) as f:
        cells = f.readlines()[1].strip().split(",")
    xa, ya, xb, yb = (np.array(c.split(";"), dtype=np.float64).astype(np.float32) for c in cells[4:8])
    first = ds.decode(0)
    assert _same_bits(first["corr_pts_ref"], np.stack([xa, ya], 1)) and _same_bits(first["corr_pts"], np.stack([xb, yb], 1))
    if name == "MegaDepth":
        assert len(MATCHING_READERS[name](os.path.join(tree, name), stage="predict", load_keys=KEYS)) == 3   # predict -> test
        with pytest.raises(AssertionError):
            MATCHING_READERS[name](os.path.join(tree, name), stage="test", load_keys=KEYS + ["image_prime"])
        with pytest.raises(AssertionError):
            MATCHING_READERS[name](os.path.join(tree, name), stage="test", load_keys=KEYS, exchange_images_with_proba=0.5)


def test_missing_scene_list_names_the_reference_file(tree, tmp_path):
    from refign_amd.datasets import MegaDepth
    with pytest.raises(FileNotFoundError, match="data_modules/datasets/lists/validation_scenes_MegaDepth.txt"):
        MegaDepth(os.path.join(tree, "MegaDepth"), stage="val", load_keys=KEYS, lists_dir=str(tmp_path))
    with pytest.raises(FileNotFoundError, match="data_modules/datasets/lists/train_debug_scenes_MegaDepth.txt"):
        MegaDepth(os.path.join(tree, "MegaDepth"), stage="val", load_keys=KEYS, lists_dir=str(tmp_path), debug=True)
    lists = tmp_path / "lists"
    lists.mkdir()
    (lists / LIST_FILES["validation"]).write_text("9001\n")
    assert len(MegaDepth(os.path.join(tree, "MegaDepth"), stage="val", load_keys=KEYS, lists_dir=str(lists))) == 3


def test_robotcar_matching_stages(ref, tree):
    from refign_amd.datasets import RobotCarMatching
    assert ref["robotcar"]["train_stage"] == "AssertionError"
    for stage in ("train", "val"):
        with pytest.raises(AssertionError):
            RobotCarMatching(os.path.join(tree, "RobotCarMatching"), stage=stage)
    ds = RobotCarMatching(os.path.join(tree, "RobotCarMatching"), stage="predict")
    assert len(ds) == 3 and tuple(ds.dims) == (1024, 1024) and ds.resize_filter == "lanczos"


def test_segmentation_module_still_refuses_them():
    from refign_amd import datasets
    assert set(datasets.READERS) == {"Cityscapes", "ACDC", "DarkZurich"}
    assert set(datasets.MATCHING_READERS) == {"MegaDepth", "RobotCarMatching"}


# ---- the plan --------------------------------------------------------------------------------------------------------------
IMNET = {"mean": (0.485, 0.456, 0.406), "std": (0.229, 0.224, 0.225)}


def _shipped(stage2):
    """the `data:` section of configs/megadepth/uawarpc_stage{1,2}.yaml (they differ in CompositeFlow's three ranges and the
    elastic field)"""
    sec = data_section(dims=(750, 750), crop=(520, 520), val_dims=(480, 720), test_resize=480, batch_size=6, num_workers=4)
    flow = sec["init_args"]["load_config"]["train"]["MegaDepth"]["transforms"][6]["init_args"]
    if not stage2:
        flow.update(random_t_hom=0.333, random_t_tps=0.333, random_t_tps_for_afftps=0.08, add_elastic=False)
    return {"data": sec}


@pytest.mark.parametrize("stage2", [False, True])
def test_matching_train_plan_of_the_shipped_sections(stage2):
    from refign_amd import config
    cfg = _shipped(stage2)
    plan = config.matching_train_plan(cfg)
    composite = {"include_transforms": ["hom", "tps", "afftps"], "random_alpha": 0.26, "random_s": 0.45, "random_tx": 0.25,
                 "random_ty": 0.25, "random_t_tps": 0.4 if stage2 else 0.333, "random_t_hom": 0.4 if stage2 else 0.333,
                 "random_t_tps_for_afftps": 0.26 if stage2 else 0.08, "parameterize_with_gaussian": False, "add_elastic": stage2}
    assert plan == {
        "reader": {"load_keys": ["image", "image_ref", "image_prime"], "dims": [750, 750], "exchange_images_with_proba": 0.5,
                   "store_scene_info_in_memory": True},
        "dims": (750, 750), "crop": (520, 520), **IMNET,
        "photometric": {"brightness": (0.4, 1.6), "contrast": (0.4, 1.6), "saturation": (0.4, 1.6), "shuffle": True,
                        "blur": {"p": 0.2, "kernel_size": 7, "sigma": (0.2, 2.0)}, **IMNET},
        "warp": {"composite": composite, "crop": (520, 520), "min_fraction_valid_corr": 0.1}}
    assert plan["photometric"] == config.photometric_plan(cfg) and plan["warp"] == config.warp_supervision_plan(cfg)
    with pytest.raises(config.OutOfScopeError):                 # the file-to-tensor planner keeps refusing the section
        config.ingest_plan(cfg, "train", "MegaDepth")
    assert config.ingest_plan(cfg, "val", "MegaDepth")["dims_interpolation"] == "lanczos"


def _edited(edit):
    cfg = _shipped(True)
    sec = cfg["data"]["init_args"]["load_config"]["train"]["MegaDepth"]
    edit(sec, sec["transforms"])
    return cfg


@pytest.mark.parametrize("edit, cause", [
    (lambda sec, t: t.insert(1, t.pop(5)), "ColorJitter"),                                # Normalize in front of the jitter
    (lambda sec, t: t.insert(6, t.pop(7)), "CompositeFlow"),                              # CenterCrop in front of CompositeFlow
    (lambda sec, t: t[1]["init_args"].pop("apply_keys"), "apply_keys"),
    (lambda sec, t: sec["load_keys"].remove("image_prime"), "image_prime"),
    (lambda sec, t: t.append(copy.deepcopy(t[7])), "second CenterCrop"),
    (lambda sec, t: t.pop(7), "CenterCrop"),
    (lambda sec, t: t.insert(1, {"class_path": "data_modules.transforms.RandomHorizontalFlip"}), "RandomHorizontalFlip"),
    (lambda sec, t: t[6]["init_args"].update(parameterize_with_gaussian=True), "parameterize_with_gaussian"),
    (lambda sec, t: sec.pop("dims"), "dims"),
])
def test_matching_train_plan_refusals(edit, cause):
    from refign_amd import config
    with pytest.raises(config.OutOfScopeError, match=cause):
        config.matching_train_plan(_edited(edit))


def test_plan_without_the_photometric_chain():
    from refign_amd import config
    plan = config.matching_train_plan(_edited(lambda sec, t: [t.pop(1) for _ in range(3)]))
    assert plan["photometric"] is None and plan["crop"] == (520, 520)


# ---- the module and the command line, as far as they go without a device ---------------------------------------------------
def test_module_reads_the_section_as_combined_data_module(tree):
    import torch
    from refign_amd import config
    from refign_amd.datamodule import MatchingDataModule
    dm = MatchingDataModule(_shipped(True), tree, torch.device("cpu"))
    assert (dm.batch_size, dm.val_batch_size, dm.test_batch_size, dm.num_workers, dm.prefetch) == (6, 3, 1, 4, 2)
    assert dm.train_on == ["MegaDepth"] == dm.val_on and dm.test_on == ["MegaDepth", "RobotCarMatching"] and dm.predict_on == []
    assert dm.idx_to_name["test"] == {0: "MegaDepth", 1: "RobotCarMatching"}
    with pytest.raises(config.OutOfScopeError, match="predict_step"):
        dm.loaders("predict")
    with pytest.raises(RuntimeError, match="HIP device"):
        dm.train_batches()
    dm.close()
    dm.close()


def test_pinned_arena_hands_out_by_capacity():
    from refign_amd.datamodule import _PinnedArena
    arena = _PinnedArena(False, step=4096)
    shapes = [(40, 56, 3), (41, 57, 3), (30, 45, 3), (36, 37, 3)]                           # 6720, 7011, 4050, 3996 bytes
    for _ in range(3):
        taken = [arena.take(s) for s in shapes]
        assert all(tuple(v.shape) == s and v.is_contiguous() for (_, v), s in zip(taken, shapes))
        assert [b.numel() for b, _ in taken] == [8192, 8192, 4096, 4096]
        arena.give([b for b, _ in taken], None)
    assert arena.allocated == 2 * 8192 + 2 * 4096                                           # two classes, not four shapes
    buf, view = arena.take((10, 10, 3))
    view.fill_(7)
    assert int(buf[:300].sum()) == 2100 and arena.allocated == 2 * 8192 + 2 * 4096


def test_parse_args_takes_graph_step():
    from refign_amd import run
    base = ["fit", "--config", "x.yaml", "--data_dir", "d"]
    assert run.parse_args(base).graph_step is False
    assert run.parse_args(base + ["--graph_step"]).graph_step is True

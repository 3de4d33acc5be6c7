"""GPU: SegmentationDataModule over the tiny RobotCar / night-test tree (tests/golden/robotcar_tree.py, rebuilt from the recipe in
tests/golden/robotcar_ref.json): the three-loader semi-supervised recipe against a composition by hand, decoding ahead, the
evaluation loaders of the three new readers, and the command line end to end.

Sizes: RobotCar files 64 x 64 read at dims 56 x 56, Cityscapes files 64 x 128 read at 56 x 112, crops 48 x 48, two samples per
loader and batch: 6, 5 and 5 training files give two batches per epoch.  The end-to-end cases need the 128 x 128 crops of the
existing step tests (mit_b0 with HRDA): there the load-time dims enlarge the files (RobotCar to 136 x 136, Cityscapes to
128 x 256; the night sets to twice their size for the sliding window of 64 x 64).
Batches are compared exactly: the kernels on the path are pinned bit-equal to Pillow elsewhere (tests/test_resample_gpu.py,
tests/test_resample_lut_gpu.py, tests/test_robotcar_ingest_gpu.py)."""
import copy
import json
import os
import random
import sys
import threading

import numpy as np
import pytest
import torch
from robotcar_tree import build_tree, night_test_section, robotcar_section, standin_h5py, write_bdd_list

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("image_src", "semantic_src", "image_trg", "image_ref")
CROP, DIMS, CS_DIMS = (48, 48), (56, 56), (56, 112)
SEED = 5             # chosen so that the first four batches see both sides of the coin (asserted below)
FIT_SEED = 0         # ... and so do the first four steps of `run fit`


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLDEN, "robotcar_ref.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tree(tmp_path_factory, ref):
    from refign_amd.datasets import write_class_stats, write_robotcar_pairs
    data_dir = str(tmp_path_factory.mktemp("rcdm"))
    build_tree(data_dir, ref["recipe"])
    write_bdd_list(data_dir, ref["recipe"])
    write_class_stats(os.path.join(data_dir, "Cityscapes"))
    had = sys.modules.get("h5py")
    sys.modules["h5py"] = standin_h5py()
    try:
        write_robotcar_pairs(os.path.join(data_dir, "RobotCar"))
    finally:
        if had is None:
            del sys.modules["h5py"]
        else:
            sys.modules["h5py"] = had
    return data_dir


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def _pil(path, dims, label=False, lut=None):
    """the reader's load of one file on the host: (encode,) Pillow's resize to dims; images come back (3, H, W)"""
    from PIL import Image
    im = Image.open(path) if label else Image.open(path).convert("RGB")
    if lut is not None:
        im = Image.fromarray(lut[np.asarray(im)])
    if im.size != (dims[1], dims[0]):
        im = im.resize((dims[1], dims[0]), resample=Image.NEAREST if label else Image.BILINEAR)
    a = np.asarray(im)
    return torch.from_numpy((a if label else a.transpose(2, 0, 1)).copy())


def test_train_batches_equal_the_composition_by_hand(dev, tree, ref):
    """prefetch=0, two epochs of two batches: bit-equal to Pillow's resize of the same files, the reference's code table applied
    in numpy, and the three existing samplers fed with the resized arrays (dims=None, no table) in loader order under the same
    seeds, torch's own RandomSampler giving each loader's order and ONE coin after each batch's samples; both random streams
    end where the composition's end; both sides of the coin occur."""
    from torch.utils.data import RandomSampler
    from refign_amd import config
    from refign_amd.datamodule import SegmentationDataModule, _one_section_cfg
    from refign_amd.datasets import Cityscapes, RobotCar
    from refign_amd.datastep import PairSampler, RareClassSourceSampler, RotatedLabelledSampler
    sec = robotcar_section(CROP, DIMS, CS_DIMS)
    _seed(SEED)
    dm = SegmentationDataModule({"data": sec}, tree, dev, prefetch=0)
    it = dm.train_batches()
    got = []
    for _ in range(4):
        b = next(it)
        assert set(b) == set(KEYS)
        got.append({k: v.clone() for k, v in b.items()})
    torch.cuda.synchronize()
    got_state = (random.getstate(), torch.get_rng_state())
    assert it.epoch == 2 and it.per_loader == 2 and it.n_batches == 2
    dm.close()

    lut = np.array(ref["encode_semantic_map"]["output"], dtype=np.uint8)        # the reference's own encode_semantic_map
    src = Cityscapes(os.path.join(tree, "Cityscapes"), stage="train", rcs_enabled=True, rcs_min_pixels=40, rcs_min_crop_ratio=2.0)
    lab = RobotCar(os.path.join(tree, "RobotCar"), stage="train", load_keys=["image", "semantic"])
    trg = RobotCar(os.path.join(tree, "RobotCar"), stage="train", load_keys=["image", "image_ref"])
    assert (len(src), len(lab), len(trg)) == (6, 5, 5)
    source = RareClassSourceSampler(lambda i: (_pil(src.paths["image"][i], CS_DIMS), _pil(src.paths["semantic"][i], CS_DIMS, True)),
                                    src.rcs_classes, src.rcs_classprob, src.indices_with_class, CROP, dev, cat_max_ratio=0.75,
                                    rcs_min_pixels=40, rcs_min_crop_ratio=2.0)
    plan = config.train_section_plan(_one_section_cfg("train", "RobotCar", sec["init_args"]["load_config"]["train"]["RobotCar"][0]),
                                     "RobotCar")
    assert plan["rotation"] is not None and plan["jitter"]["hue"] is not None and plan["dims"] == DIMS
    labelled = RotatedLabelledSampler(
        lambda i: (_pil(lab.paths["image"][i], DIMS).permute(1, 2, 0).contiguous(), _pil(lab.paths["semantic"][i], DIMS, True, lut)),
        dict(plan, dims=None), dev)
    pairs = PairSampler(lambda i: (_pil(trg.paths["image"][i], DIMS), _pil(trg.paths["image_ref"][i], DIMS)), CROP, dev)
    _seed(SEED)
    want, coins = [], []
    for _ in range(2):
        list(RandomSampler(range(len(src))))                    # the first loader's order: drawn, unused under rcs_enabled
        lab_order = list(RandomSampler(range(len(lab))))
        trg_order = list(RandomSampler(range(len(trg))))
        for b in range(2):                                      # drop_last, the shortest loader: 5 // 2
            s = [source.sample() for _ in range(2)]
            s += [labelled.sample(i) for i in lab_order[2 * b:2 * b + 2]]
            t = [pairs.sample(i) for i in trg_order[2 * b:2 * b + 2]]
            heads = random.random() < 0.5
            coins.append(heads)
            n = 2 if heads else 4
            want.append({"image_src": torch.stack([x[0] for x in s])[:n], "semantic_src": torch.stack([x[1] for x in s])[:n],
                         "image_trg": torch.stack([x[0] for x in t]), "image_ref": torch.stack([x[1] for x in t])})
    torch.cuda.synchronize()
    print(f"\ncoins of seed {SEED}: {coins}")
    assert True in coins and False in coins, f"seed {SEED} shows one side of the coin only: {coins}"
    for n, (g, w) in enumerate(zip(got, want)):
        for k in KEYS:
            assert g[k].shape == w[k].shape, f"batch {n}: {k} has {tuple(g[k].shape)}, the composition {tuple(w[k].shape)}"
            assert g[k].dtype == w[k].dtype and torch.equal(g[k], w[k]), f"batch {n}: {k} differs"
    assert got_state[0] == random.getstate() and torch.equal(got_state[1], torch.get_rng_state())
    # RobotCar's labels went through the table: train ids, 255 and the codes the map leaves alone
    seen = set(torch.cat([g["semantic_src"][2:].flatten() for g in got if g["semantic_src"].shape[0] == 4]).tolist())
    assert seen <= set(range(19)) | {255} | set(ref["recipe"]["RobotCar"]["codes_above_33"])


def test_decoding_ahead_chooses_the_same_files(dev, tree):
    """prefetch=2 with four threads against prefetch=0 from one seed: over two epochs and a batch the same target and labelled
    RobotCar indices reach the assembler (the permutations come from the torch stream, which both modes consume alike); halved
    batches are views of the assembler's buffers and hand them back; no decoding thread is left after close()."""
    from refign_amd.datamodule import SegmentationDataModule

    def run(workers, prefetch):
        _seed(11)
        dm = SegmentationDataModule({"data": robotcar_section(CROP, DIMS, CS_DIMS, num_workers=workers)}, tree, dev, prefetch=prefetch)
        it = dm.train_batches()
        real, chosen, sizes = it.asm.assemble, [], []

        def recording(pair_indices, labelled_indices=None):
            chosen.append((list(pair_indices), list(labelled_indices)))
            return real(pair_indices, labelled_indices)
        it.asm.assemble = recording
        for _ in range(5):
            b = next(it)
            sizes.append(b["image_src"].shape[0])
            sets = it.asm._sets
            assert any(b["image_src"].data_ptr() == st["image_src"].data_ptr() and b["image_trg"] is st["image_trg"] for st in sets)
            assert b["semantic_src"].shape[0] == sizes[-1] and b["image_src"].is_contiguous()
        torch.cuda.synchronize()
        alive = [t for t in threading.enumerate() if t.name.startswith("refign-decode")]
        halved = it.halved
        dm.close()
        return chosen, sizes, alive, halved

    ahead, sizes, alive, halved = run(4, 2)
    assert 0 < len(alive) <= 4 and set(sizes) <= {2, 4} and halved == sizes.count(2)
    assert not [t for t in threading.enumerate() if t.name.startswith("refign-decode")], "close() left a decoding thread"
    plain, _, alive, _ = run(0, 0)
    assert not alive
    assert ahead == plain and len(plain) == 5
    for epoch in (plain[0:2], plain[2:4]):                      # an epoch: four distinct files of five, per loader
        assert len({i for p, _ in epoch for i in p}) == 4 and len({i for _, l in epoch for i in l}) == 4


def test_robotcar_val_loader_equals_the_host(dev, tree, ref):
    """the val section as the configuration ships it (no `dims`: the reader's 1024 x 1024) and with dims at the file's size (the
    encode alone): images and labels bit-equal to Pillow's resize, the reference's table in numpy, u8 / 255 and (x - mean) / std
    in fp32 on the host"""
    from refign_amd.datamodule import SegmentationDataModule
    from refign_amd.datasets import RobotCar
    from refign_amd.datastep import IMNET_MEAN, IMNET_STD
    lut = np.array(ref["encode_semantic_map"]["output"], dtype=np.uint8)
    mean, std = torch.tensor(IMNET_MEAN).view(3, 1, 1), torch.tensor(IMNET_STD).view(3, 1, 1)
    ds = RobotCar(os.path.join(tree, "RobotCar"), stage="val", load_keys=["image", "semantic"])
    for eval_dims, size in ((None, (1024, 1024)), ((64, 64), (64, 64)), ((40, 72), (40, 72))):
        dm = SegmentationDataModule({"data": robotcar_section(CROP, DIMS, CS_DIMS, eval_dims=eval_dims)}, tree, dev)
        assert dm.val_batch_size == 1
        batches = list(dm.loaders("val")["RobotCar"])
        assert len(batches) == len(ds) == 3
        for i, b in enumerate(batches):
            assert set(b) == {"image", "semantic", "filename"} and b["filename"] == [ds.filename(i)]
            assert b["image"].shape == (1, 3, *size) and b["semantic"].shape == (1, *size) and b["semantic"].dtype == torch.int64
            img = (_pil(ds.paths["image"][i], size).to(torch.float32) / 255.0 - mean) / std
            lbl = _pil(ds.paths["semantic"][i], size, True, lut).to(torch.int64)
            assert torch.equal(b["image"][0].cpu(), img), f"dims {eval_dims}: image {i} differs"
            assert torch.equal(b["semantic"][0].cpu(), lbl), f"dims {eval_dims}: label {i} differs"
            assert set(lbl.unique().tolist()) <= set(range(19)) | {255} | set(ref["recipe"]["RobotCar"]["codes_above_33"])
        dm.close()


NIGHT_DIMS = {"DarkZurich": (108, 192), "NighttimeDriving": (108, 192), "BDD100kNight": (96, 160)}


def test_night_test_loaders_give_batches_for_each_set(dev, tree, ref):
    from refign_amd import datasets
    from refign_amd.datamodule import SegmentationDataModule
    from refign_amd.resample import EvalIngest
    dm = SegmentationDataModule({"data": night_test_section(NIGHT_DIMS)}, tree, dev)
    loaders = dm.loaders("test")                                # every section, without datasets=
    assert list(loaders) == ["DarkZurich", "NighttimeDriving", "BDD100kNight"] == dm.test_on
    for name, n in (("DarkZurich", 2), ("NighttimeDriving", 3), ("BDD100kNight", 3)):
        ds = datasets.SEGMENTATION_READERS[name](os.path.join(tree, name), stage="test", load_keys=["image", "semantic"])
        by_hand = EvalIngest(dims=NIGHT_DIMS[name], device=dev)
        batches = list(loaders[name])
        assert len(batches) == n == len(ds)
        for i, b in enumerate(batches):
            s = ds.decode(i)
            assert s["image"].shape[:2] == tuple(ref["recipe"][name]["size"])
            want = by_hand(s["image"], semantic=s["semantic"])
            assert b["filename"] == [ds.filename(i)] and b["image"].shape == (1, 3, *NIGHT_DIMS[name])
            assert torch.equal(b["image"], want["image"]) and torch.equal(b["semantic"], want["semantic"])
    # the sections as the configuration ships them: the readers' own sizes
    full = SegmentationDataModule({"data": night_test_section()}, tree, dev).loaders("test")
    assert next(iter(full["BDD100kNight"]))["image"].shape == (1, 3, 720, 1280)
    assert next(iter(full["NighttimeDriving"]))["semantic"].shape == (1, 1080, 1920)
    dm.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------
SHRINK = ["model.init_args.backbone.init_args.model_type=mit_b0", "model.init_args.backbone.init_args.pretrained=null",
          "model.init_args.head.init_args.in_channels=[32, 64, 160, 256]",
          "model.init_args.hrda_scale_attention.init_args.in_channels=[32, 64, 160, 256]",
          "model.init_args.alignment_backbone.init_args.pretrained=null", "model.init_args.alignment_head.init_args.pretrained=null",
          "model.init_args.inference_crop_size=[64, 64]", "model.init_args.inference_stride=[40, 48]"]
SHRINK = [a for s in SHRINK for a in ("--set", s)]


def _yaml(tmp_path_factory, name, data, metrics, precision):
    """refign_hrda_star.yaml's model, optimizer and scheduler sections (bench.REF_CFG holds them) with the tree's data section"""
    import bench
    import yaml
    cfg = copy.deepcopy(bench.REF_CFG)
    cfg["model"]["init_args"]["metrics"] = metrics
    cfg["seed_everything"] = FIT_SEED
    cfg["data"] = data
    cfg["trainer"] = {"max_steps": 20000, "sync_batchnorm": True, "precision": precision,
                      "callbacks": [{"class_path": "pytorch_lightning.callbacks.LearningRateMonitor"},
                                    {"class_path": "helpers.callbacks.ValEveryNSteps", "init_args": {"every_n_steps": 2000}},
                                    {"class_path": "pytorch_lightning.callbacks.ModelCheckpoint", "init_args": {"save_last": True}}]}
    path = tmp_path_factory.mktemp("cfg") / name
    path.write_text(yaml.safe_dump(cfg, sort_keys=False))       # the sections' order is part of a configuration
    return str(path)


def _iou(**kw):
    return [{"class_path": "helpers.metrics.IoU", "init_args": dict({"ignore_index": 255, "num_classes": 19, "compute_on_step": False}, **kw)}]


@pytest.fixture(scope="module")
def robotcar_yaml(tmp_path_factory):
    data = robotcar_section((128, 128), (136, 136), (128, 256), num_workers=4, eval_dims=(72, 72))
    metrics = {"val": {"RobotCar": _iou(over_present_classes=True)}, "test": {"RobotCar": _iou(over_present_classes=True)}}
    return _yaml(tmp_path_factory, "refign_robotcar_tiny.yaml", data, metrics, "bf16")


def test_fit_runs_the_semi_supervised_recipe_from_the_folders(dev, tree, robotcar_yaml, tmp_path, monkeypatch):
    """four steps through the command line, graphs at their defaults: finite losses, four and two source samples both seen"""
    from refign_amd import run
    from refign_amd.trainer import Trainer
    seen, real = [], Trainer.step

    def recording(self, batch, batch_idx=0, next_batch=None):
        out = real(self, batch, batch_idx, next_batch=next_batch)
        seen.append((batch["image_src"].shape[0], batch["image_trg"].shape[0],
                     [float(self.model.logged[k]) for k in ("train_loss_src", "train_loss_uda_trg")]))
        return out
    monkeypatch.setattr(Trainer, "step", recording)
    handles = {}
    hist = run.main(["fit", "--config", robotcar_yaml, "--data_dir", tree, "--save_dir", str(tmp_path), "--set", "trainer.max_steps=4",
                     "--set", "trainer.callbacks.1.init_args.every_n_steps=null"] + SHRINK, handles=handles)
    tr, dm = handles["trainer"], handles["datamodule"]
    try:
        print(f"\nsource / target batch sizes and losses of seed {FIT_SEED}: {seen}")
        assert hist == [] and tr.model.global_step == 4 and len(seen) == 4
        assert all(t == 2 and s in (2, 4) for s, t, _ in seen)
        assert all(np.isfinite(v) for _, _, losses in seen for v in losses)
        assert {s for s, _, _ in seen} == {2, 4}, f"seed {FIT_SEED} shows one source batch size only"
        assert not any(s["failed"] for g in tr.model._graphs.values() for s in g.states.values()), "a graph capture failed"
        assert torch.load(str(tmp_path / "last.ckpt"), map_location="cpu", weights_only=False)["global_step"] == 4
    finally:
        dm.close()
        tr.close()
    assert not [t for t in threading.enumerate() if t.name.startswith("refign-decode")]


def test_robotcar_metric_leaves_absent_classes_out(dev, tree, robotcar_yaml, ref, monkeypatch):
    """`run test` on the RobotCar section: test_RobotCar_IoU is the mean over the classes the LABELS hold (over_present_classes:
    True) of the run's own count matrix, not the mean over all nineteen"""
    from refign_amd import run
    from refign_amd.datasets import RobotCar
    from refign_amd.metrics import IoU
    computed, real = [], IoU.compute

    def recording(self):
        out = real(self)
        computed.append((self.confmat.detach().cpu().clone(), bool(self.over_present_classes), float(out)))
        return out
    monkeypatch.setattr(IoU, "compute", recording)
    out = run.main(["test", "--config", robotcar_yaml, "--data_dir", tree, "--set", "trainer.precision=32"] + SHRINK)
    assert set(out) == {"test_RobotCar_IoU"} and len(computed) == 1
    cm, flag, value = computed[0]
    assert flag is True and abs(out["test_RobotCar_IoU"] - value) < 1e-6
    # the classes of the tree's test labels, through the reference's table and Pillow's resize, on the host
    lut = np.array(ref["encode_semantic_map"]["output"], dtype=np.uint8)
    ds = RobotCar(os.path.join(tree, "RobotCar"), stage="test", load_keys=["image", "semantic"])
    labels = torch.cat([_pil(ds.paths["semantic"][i], (72, 72), True, lut).flatten() for i in range(len(ds))])
    present = sorted(c for c in labels.unique().tolist() if c < 19)
    assert 0 < len(present) < 19, "the tree's test labels must miss a class"
    rows = cm.sum(1)
    assert [c for c in range(19) if rows[c] > 0] == present and int(cm.sum()) == int((labels < 19).sum())
    inter = torch.diag(cm).double()
    union = (cm.sum(0) + cm.sum(1)).double() - inter
    scores = torch.where(union > 0, inter / union.clamp(min=1), torch.zeros_like(inter))
    over_present, over_all = float(scores[present].mean()), float(scores.mean())
    print(f"\ntest_RobotCar_IoU {value}: over the {len(present)} present classes {over_present}, over all nineteen {over_all}")
    assert abs(value - over_present) < 1e-6
    if over_present > 0:
        assert abs(value - over_all) > 1e-6


def test_test_runs_all_three_night_sets_without_datasets(dev, tree, tmp_path_factory, monkeypatch):
    """`run test` over the Dark Zurich configurations' test section: three metrics, and the fused evaluation tail gives what
    RFN_EVAL_FUSED=0 gives (fp32: the bound of test_evaltail_gpu.py::test_trainer_validate_on_the_fused_path)"""
    from refign_amd import run
    metrics = {"test": {n: _iou() for n in ("DarkZurich", "NighttimeDriving", "BDD100kNight")}}
    path = _yaml(tmp_path_factory, "refign_night_tiny.yaml", night_test_section(NIGHT_DIMS), metrics, 32)
    argv = ["test", "--config", path, "--data_dir", tree] + SHRINK
    monkeypatch.delenv("RFN_EVAL_FUSED", raising=False)
    fused = run.main(argv)
    monkeypatch.setenv("RFN_EVAL_FUSED", "0")
    plain = run.main(argv)
    print(f"\nfused {fused}\nRFN_EVAL_FUSED=0 {plain}")
    assert set(fused) == {"test_DarkZurich_IoU", "test_NighttimeDriving_IoU", "test_BDD100kNight_IoU"} == set(plain)
    for k in fused:
        assert np.isfinite(fused[k]) and abs(fused[k] - plain[k]) < 1e-6, f"{k}: fused {fused[k]} against {plain[k]}"

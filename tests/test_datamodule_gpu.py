"""GPU: SegmentationDataModule over a tiny tree of PNG files (tests/golden/datamodule_tree.py, rebuilt from the recipe stored in
tests/golden/datamodule_ref.json): training batches against a host restatement, decoding ahead, the evaluation loaders, the
command line end to end, and the class statistics counted on the device.

Sizes: Cityscapes files 128 x 256 read at dims 64 x 128, ACDC files 108 x 192 read at 54 x 96, crops 48 x 48, two samples per
loader and batch: 6 and 8 training files give three batches per epoch.  The end-to-end case needs the 128 x 128 crops of the
existing step tests (mit_b0 with HRDA): Cityscapes at its files' size, ACDC enlarged to 136 x 240.
All comparisons are exact: the kernels on the path are pinned bit-equal to Pillow elsewhere (tests/test_resample_gpu.py)."""
import copy
import json
import os
import random
import threading

import numpy as np
import pytest
import torch
from datamodule_tree import build_tree, data_section

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("image_src", "semantic_src", "image_trg", "image_ref")
CROP, CS_DIMS, TRG_DIMS = (48, 48), (64, 128), (54, 96)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from refign_amd.datasets import write_class_stats
    with open(os.path.join(GOLDEN, "datamodule_ref.json")) as f:
        recipe = json.load(f)["recipe"]
    data_dir = str(tmp_path_factory.mktemp("dm"))
    build_tree(data_dir, recipe)
    write_class_stats(os.path.join(data_dir, "Cityscapes"))
    return data_dir


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def _take(it, n):
    out = []
    for _ in range(n):
        b = next(it)
        assert set(b) == set(KEYS)
        out.append({k: v.clone() for k, v in b.items()})      # the buffers are written again two batches later
    return out


def _same(a, b, keys=KEYS):
    return all(x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in keys) and len(a) == len(b)


def _tails():
    return random.random(), torch.rand(2).tolist()


def _pil(path, dims, label=False):
    from PIL import Image
    im = Image.open(path) if label else Image.open(path).convert("RGB")
    if im.size != (dims[1], dims[0]):
        im = im.resize((dims[1], dims[0]), resample=Image.NEAREST if label else Image.BILINEAR)
    a = np.asarray(im)
    return torch.from_numpy((a if label else a.transpose(2, 0, 1)).copy())


def test_train_batches_equal_a_host_restatement(dev, tree):
    """prefetch=0, two epochs: bit-equal to Pillow's resize of the same files followed by the existing samplers fed with the
    resized arrays (dims=None), under the same seeds and torch's own RandomSampler for the order; both random streams end where
    the restatement's end."""
    from torch.utils.data import RandomSampler
    from refign_amd.datamodule import SegmentationDataModule
    from refign_amd.datasets import ACDC, Cityscapes
    from refign_amd.datastep import PairSampler, RareClassSourceSampler
    cfg = {"data": data_section("ACDC", CROP, CS_DIMS, TRG_DIMS, batch_size=4)}
    _seed(5)
    dm = SegmentationDataModule(cfg, tree, dev, prefetch=0)
    it = dm.train_batches()
    got = _take(it, 6)
    torch.cuda.synchronize()
    got_tails = _tails()
    assert it.epoch == 2 and got[0]["image_src"].shape == (2, 3, 48, 48) and got[0]["semantic_src"].dtype == torch.int64
    dm.close()

    _seed(5)
    src = Cityscapes(os.path.join(tree, "Cityscapes"), stage="train", rcs_enabled=True, rcs_min_pixels=40, rcs_min_crop_ratio=2.0)
    trg = ACDC(os.path.join(tree, "ACDC"), stage="train", load_keys=["image", "image_ref"])
    source = RareClassSourceSampler(lambda i: (_pil(src.paths["image"][i], CS_DIMS), _pil(src.paths["semantic"][i], CS_DIMS, True)),
                                    src.rcs_classes, src.rcs_classprob, src.indices_with_class, CROP, dev, cat_max_ratio=0.75,
                                    rcs_min_pixels=40, rcs_min_crop_ratio=2.0)
    pairs = PairSampler(lambda i: (_pil(trg.paths["image"][i], TRG_DIMS), _pil(trg.paths["image_ref"][i], TRG_DIMS)), CROP, dev)
    want = []
    for _ in range(2):
        list(RandomSampler(range(len(src))))                    # the source loader's order: drawn, unused under rcs_enabled
        order = list(RandomSampler(range(len(trg))))
        for b in range(min(len(src), len(trg)) // 2):           # drop_last, min_size
            s = [source.sample() for _ in range(2)]
            t = [pairs.sample(i) for i in order[2 * b:2 * b + 2]]
            want.append({"image_src": torch.stack([x[0] for x in s]), "semantic_src": torch.stack([x[1] for x in s]),
                         "image_trg": torch.stack([x[0] for x in t]), "image_ref": torch.stack([x[1] for x in t])})
    assert len(want) == 6
    for n, (g, w) in enumerate(zip(got, want)):
        for k in KEYS:
            assert g[k].dtype == w[k].dtype and torch.equal(g[k], w[k]), f"batch {n}: {k} differs"
    assert got_tails == _tails()


def test_decoding_ahead(dev, tree, monkeypatch):
    """prefetch=2 with four threads.  The source half is reproducible: two runs from one seed are bit-equal.  The target half
    equals prefetch=0's: the same permutation (the torch stream is not touched by the source loader) and, for the same crop
    draws, the same tensors.  The crop draws come from the global `random` stream, which the two modes leave in different states
    in front of a target sample -- with prefetch=0 the source's class and file draws are on it, and how many crop candidates a
    source sample draws depends on the file chosen -- so the comparison fixes them: PairSampler.sample runs under a state
    seeded from its index here, in both runs, and puts the stream back.  After close() no decoding thread is left."""
    from refign_amd import datastep
    from refign_amd.datamodule import SegmentationDataModule
    cfg0 = {"data": data_section("ACDC", CROP, CS_DIMS, TRG_DIMS, batch_size=4, num_workers=0)}
    cfg4 = {"data": data_section("ACDC", CROP, CS_DIMS, TRG_DIMS, batch_size=4, num_workers=4)}

    def run(cfg, prefetch):
        _seed(9)
        dm = SegmentationDataModule(cfg, tree, dev, prefetch=prefetch)
        out = _take(dm.train_batches(), 7)                       # into the third epoch, past the depth of the buffer pool
        torch.cuda.synchronize()
        alive = [t for t in threading.enumerate() if t.name.startswith("refign-decode")]
        dm.close()
        return out, alive

    a, alive = run(cfg4, None)
    assert 0 < len(alive) <= 4
    assert not [t for t in threading.enumerate() if t.name.startswith("refign-decode")], "close() left a decoding thread"
    b, _ = run(cfg4, 2)
    assert _same(a, b), "two runs with prefetch=2 from one seed differ"

    real = datastep.PairSampler.sample

    def fixed_draws(self, index, *args, **kw):
        state = random.getstate()
        random.seed(4000 + index)
        try:
            return real(self, index, *args, **kw)
        finally:
            random.setstate(state)

    monkeypatch.setattr(datastep.PairSampler, "sample", fixed_draws)
    ahead, _ = run(cfg4, 2)
    plain, alive = run(cfg0, 0)
    assert not alive                                             # prefetch=0 starts no thread
    assert _same(ahead, plain, ("image_trg", "image_ref")), "the target half differs between prefetch=2 and prefetch=0"
    assert not _same(plain[:1], plain[1:2], ("image_trg",))


@pytest.mark.parametrize("workers", [0, 4])
def test_evaluation_loaders(dev, tree, workers):
    """val (dims, batches of two with a last one of one) and test (the file's size, then Resize(img_only=True): a half-size image
    with the full-size label) equal EvalIngest applied by hand to the same decoded files; predict has images and names only."""
    from refign_amd.datamodule import SegmentationDataModule
    from refign_amd.datasets import ACDC
    from refign_amd.resample import EvalIngest
    cfg = {"data": data_section("ACDC", CROP, CS_DIMS, TRG_DIMS, batch_size=8, num_workers=workers)}
    dm = SegmentationDataModule(cfg, tree, dev)
    assert (dm.val_batch_size, dm.test_batch_size) == (2, 1)
    full = tuple(json.load(open(os.path.join(GOLDEN, "datamodule_ref.json")))["recipe"]["ACDC"]["size"])
    by_hand = {"val": EvalIngest(dims=TRG_DIMS, device=dev), "test": EvalIngest(dims=full, resize=TRG_DIMS, img_only=True, device=dev)}
    for split, sizes in (("val", [2, 2, 1]), ("test", [1] * 5)):
        loaders = dm.loaders(split)
        assert list(loaders) == ["ACDC"]
        ds = ACDC(os.path.join(tree, "ACDC"), stage=split, load_keys=["image", "semantic"])
        for _ in range(2):                                        # a loader can be walked again
            batches = list(loaders["ACDC"])
            assert [len(b["filename"]) for b in batches] == sizes == [b["image"].shape[0] for b in batches]
            at = 0
            for b in batches:
                assert set(b) == {"image", "semantic", "filename"}
                for j, name in enumerate(b["filename"]):
                    assert name == ds.filename(at) and name.endswith("_rgb_anon.png")
                    s = ds.decode(at)
                    want = by_hand[split](s["image"], semantic=s["semantic"])
                    assert torch.equal(b["image"][j:j + 1], want["image"]) and torch.equal(b["semantic"][j:j + 1], want["semantic"])
                    at += 1
                assert b["image"].shape[1:] == (3, *TRG_DIMS) and b["image"].dtype == torch.float32 and b["image"].is_cuda
                assert b["semantic"].shape[1:] == (TRG_DIMS if split == "val" else full) and b["semantic"].dtype == torch.int64
            assert at == len(ds) == 5
    pred = list(dm.loaders("predict")["ACDC"])
    assert len(pred) == 4 and all(set(b) == {"image", "filename"} and b["image"].shape == (1, 3, *TRG_DIMS) for b in pred)
    dm.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------
SHRINK = ["model.init_args.backbone.init_args.model_type=mit_b0", "model.init_args.backbone.init_args.pretrained=null",
          "model.init_args.head.init_args.in_channels=[32, 64, 160, 256]",
          "model.init_args.hrda_scale_attention.init_args.in_channels=[32, 64, 160, 256]",
          "model.init_args.alignment_backbone.init_args.pretrained=null", "model.init_args.alignment_head.init_args.pretrained=null",
          "model.init_args.inference_crop_size=[64, 64]", "model.init_args.inference_stride=[40, 48]"]


@pytest.fixture(scope="module")
def yaml_path(tmp_path_factory):
    """refign_hrda_star.yaml's model, optimizer and scheduler sections (bench.REF_CFG holds them) with the tree's data section"""
    import bench
    import yaml
    cfg = copy.deepcopy(bench.REF_CFG)
    iou = [{"class_path": "helpers.metrics.IoU", "init_args": {"ignore_index": 255, "num_classes": 19, "compute_on_step": False}}]
    cfg["model"]["init_args"]["metrics"] = {"val": {"ACDC": copy.deepcopy(iou)}, "test": {"ACDC": copy.deepcopy(iou)}}
    cfg["seed_everything"] = 0
    cfg["data"] = data_section("ACDC", (128, 128), (128, 256), (136, 240), batch_size=4, num_workers=4)
    cfg["trainer"] = {"max_steps": 40000, "sync_batchnorm": True, "precision": "bf16", "multiple_trainloader_mode": "min_size",
                      "callbacks": [{"class_path": "pytorch_lightning.callbacks.LearningRateMonitor"},
                                    {"class_path": "helpers.callbacks.ValEveryNSteps", "init_args": {"every_n_steps": 4000}},
                                    {"class_path": "pytorch_lightning.callbacks.ModelCheckpoint", "init_args": {"save_last": True}}]}
    path = tmp_path_factory.mktemp("cfg") / "refign_hrda_star_tiny.yaml"
    path.write_text(yaml.safe_dump(cfg, sort_keys=False))       # the sections' order is part of a configuration
    return str(path)


def test_fit_validate_and_predict_from_the_folders(dev, tree, yaml_path, tmp_path):
    from PIL import Image
    from refign_amd import run
    ckpt = tmp_path / "ckpt"
    hist = run.main(["fit", "--config", yaml_path, "--data_dir", tree, "--save_dir", str(ckpt), "--set", "trainer.max_steps=2",
                     "--set", "trainer.callbacks.1.init_args.every_n_steps=1"] + [a for s in SHRINK for a in ("--set", s)])
    assert [s for s, _ in hist] == [1, 2]
    assert all(set(m) == {"val_ACDC_IoU"} and np.isfinite(m["val_ACDC_IoU"]) for _, m in hist)
    last = ckpt / "last.ckpt"
    assert torch.load(str(last), map_location="cpu", weights_only=False)["global_step"] == 2
    assert not [t for t in threading.enumerate() if t.name.startswith("refign-decode")]
    out = tmp_path / "out"
    n = run.main(["predict", "--config", yaml_path, "--data_dir", tree, "--ckpt_path", str(last), "--save_dir", str(out)]
                 + [a for s in SHRINK for a in ("--set", s)])
    files = sorted(os.listdir(out / "preds" / "ACDC"))
    assert n == 8 and len(files) == 4 and files == sorted(os.listdir(out / "color_preds" / "ACDC"))
    assert all(f.endswith("_rgb_anon.png") for f in files)
    for f in files:
        with Image.open(out / "preds" / "ACDC" / f) as im:
            assert im.size == (1920, 1080)                       # ACDC's orig_dims


def test_fit_keeps_the_student_graphs(dev, tree, yaml_path, tmp_path):
    """Five steps straight from the iterator, graphs at their defaults: the student passes are captured on the third call of
    their signature (steps 2 - 4: fit's first step has no prefetched features) and the last step replays them -- next() between
    the steps, with its draws, copies and kernels on the calling thread, loses no capture."""
    from refign_amd import run
    handles = {}
    hist = run.main(["fit", "--config", yaml_path, "--data_dir", tree, "--save_dir", str(tmp_path), "--set", "trainer.max_steps=5",
                     "--set", "trainer.callbacks.1.init_args.every_n_steps=null"] + [a for s in SHRINK for a in ("--set", s)],
                    handles=handles)
    tr, dm = handles["trainer"], handles["datamodule"]
    try:
        assert hist == [] and tr.model.global_step == 5
        for name in ("source_pass", "mixed_pass"):
            g = tr.model._graphs[name]
            st = list(g.states.values())
            assert not any(s["failed"] for s in st), f"{name}: a capture failed"
            assert g.captured(), f"{name}: the last step did not replay its graph"
    finally:
        dm.close()
        tr.close()


def test_class_stats_on_the_device_equal_numpy(dev, tree, tmp_path):
    from refign_amd.datasets import write_class_stats
    root = os.path.join(tree, "Cityscapes")
    host = write_class_stats(root, str(tmp_path / "host"))
    device = write_class_stats(root, str(tmp_path / "device"), device=dev)
    assert host == device and len(host) == 6
    for name in ("sample_class_stats.json", "sample_class_stats_dict.json", "samples_with_class.json"):
        assert (tmp_path / "host" / name).read_text() == (tmp_path / "device" / name).read_text()

"""GPU: MatchingDataModule over the tiny MegaDepth / RobotCarMatching tree of tests/golden/matching_tree.py (rebuilt from the
recipe stored in tests/golden/matching_ref.json): training batches against a composition by hand, decoding ahead, the command
line (fit with and without the graphed step, validation inside fit, test against a hand-fed Trainer.test), teardown.

Sizes: files of 40 x 56 ... 97 x 131 read at dims 160 x 160, crop 128 x 160 (the size of the existing matcher step tests,
tests/test_matcher_trainer_gpu.py), batch 2: 12 training pairs give six batches per epoch; 28 validation pairs at 128 x 160;
three test pairs per data set, their smaller side resized to 128.  The training section is stage 1's (no elastic field: its
bumps need a frame of 240 pixels).
The batch comparisons are exact: the kernels on the path are pinned bit-equal to Pillow elsewhere (tests/test_lanczos_gpu.py)."""
import json
import os
import random
import threading

import numpy as np
import pytest
import torch
from matching_tree import build_tree, data_section

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("image_ref", "image_trg", "image_prime", "flow_prime", "mask_prime", "prime_trg_idx")
DIMS, CROP = (160, 160), (128, 160)
MEAN, STD = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
SEED = 11                                                    # its first four coins hold both outcomes (asserted below)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    with open(os.path.join(GOLDEN, "matching_ref.json")) as f:
        recipe = json.load(f)["recipe"]
    return build_tree(str(tmp_path_factory.mktemp("match")), recipe)


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def _decoders():
    return [t for t in threading.enumerate() if t.name.startswith("refign-decode")]


def _take(it, n):
    out, exchanged = [], []
    for _ in range(n):
        b = next(it)
        assert set(b) == set(KEYS)
        out.append({k: v.clone() for k, v in b.items()})
        exchanged.append(list(it.exchanged))
    return out, exchanged


def _pil(hwc, dims):
    from PIL import Image
    im = Image.fromarray(hwc)
    if im.size != (dims[1], dims[0]):
        im = im.resize((dims[1], dims[0]), resample=Image.LANCZOS)
    return torch.from_numpy(np.asarray(im).transpose(2, 0, 1).copy())


def _normalise(u8):
    return (u8.to(torch.float32) / 255 - MEAN[:, None, None]) / STD[:, None, None]


def test_train_batches_equal_a_composition_by_hand(dev, tree):
    """prefetch=0, two batches: bit-equal to reader.decode, Pillow's own LANCZOS resize on the host, normalisation in torch and
    one WarpSupervision call per sample (which crops image and image_ref and makes the sample's draws) -- with the coin in front
    of each sample, the reference's order.  Both random streams end where the hand run's end."""
    from torch.utils.data import RandomSampler
    from refign_amd import config
    from refign_amd.datamodule import MatchingDataModule
    from refign_amd.datasets import MegaDepth
    from refign_amd.flowsynth import WarpSupervision
    cfg = {"data": data_section(DIMS, CROP, batch_size=2, num_workers=0, exchange=0.5, elastic=False)}
    _seed(SEED)
    dm = MatchingDataModule(cfg, tree, dev, prefetch=0)
    it = dm.train_batches()
    got, exchanged = _take(it, 2)
    torch.cuda.synchronize()
    tails = (random.getstate(), torch.get_rng_state())
    assert not _decoders()                                   # prefetch=0 starts no thread
    dm.close()
    flat = [e for batch in exchanged for e in batch]
    assert True in flat and False in flat, flat
    b0 = got[0]
    assert b0["image_ref"].shape == b0["image_trg"].shape == b0["image_prime"].shape == (2, 3, *CROP)
    assert b0["flow_prime"].shape == (2, 2, *CROP) and b0["mask_prime"].shape == (2, *CROP) and b0["mask_prime"].dtype == torch.bool
    assert b0["prime_trg_idx"].dtype == torch.int64 and b0["prime_trg_idx"].is_cuda and b0["prime_trg_idx"].tolist() == [1, 1]

    _seed(SEED)
    plan = config.matching_train_plan(cfg)
    reader = MegaDepth(os.path.join(tree, "MegaDepth"), stage="train", **plan["reader"])
    ws = WarpSupervision(plan["warp"], photometric=plan["photometric"])
    order = list(RandomSampler(range(len(reader))))
    hand_exchanged = []
    for n in range(2):
        parts = []
        for i in order[2 * n:2 * n + 2]:
            ex = random.random() < 0.5
            hand_exchanged.append(ex)
            s = reader.decode(i, exchange=ex)
            ref, trg = _pil(s["image_ref"], DIMS), _pil(s["image"], DIMS)
            parts.append(ws({"image": _normalise(trg).unsqueeze(0).to(dev), "image_ref": _normalise(ref).unsqueeze(0).to(dev),
                             "image_prime": trg.unsqueeze(0).to(dev)}))
        for k in KEYS[:-1]:
            want = torch.cat([p[k] for p in parts])
            assert got[n][k].dtype == want.dtype and torch.equal(got[n][k], want), f"batch {n}: {k} differs"
    assert hand_exchanged == flat
    torch.cuda.synchronize()
    assert tails[0] == random.getstate() and torch.equal(tails[1], torch.get_rng_state())


def test_decoding_ahead(dev, tree, monkeypatch):
    """prefetch=2 with four threads: two runs from one seed are bit-equal in every key.  Against prefetch=0: the permutation is
    the same (the epoch's is the first draw on the torch stream in both), and for the same coins image_ref and image_trg are the
    same tensors; the coins come from different streams in the two modes, so the comparison fixes them (the k-th coin of a run
    follows one pattern in both; the stream is consumed all the same).  The photometric and composite draws stay in next(), on
    global streams the two modes leave in different states: image_prime is not compared.  After close() no thread is left."""
    from refign_amd import datamodule
    from refign_amd.datamodule import MatchingDataModule
    cfg0 = {"data": data_section(DIMS, CROP, batch_size=2, num_workers=0, elastic=False)}
    cfg4 = {"data": data_section(DIMS, CROP, batch_size=2, num_workers=4, elastic=False)}

    def run(cfg, prefetch, n=5):
        _seed(9)
        dm = MatchingDataModule(cfg, tree, dev, prefetch=prefetch)
        it = dm.train_batches()
        out, exchanged = _take(it, n)
        torch.cuda.synchronize()
        alive = _decoders()
        dm.close()
        dm.close()                                           # harmless
        return out, exchanged, alive, it

    a, _, alive, it = run(cfg4, None, 8)                     # into the second epoch
    assert 0 < len(alive) <= 4 and it.epoch == 2
    assert not _decoders(), "close() left a decoding thread"
    b, _, _, _ = run(cfg4, 2, 8)
    for x, y in zip(a, b):
        assert all(torch.equal(x[k], y[k]) for k in KEYS), "two runs with prefetch=2 from one seed differ"
    # distinct shapes in flight, few capacity classes: staging memory is counted in classes
    assert it.arena.allocated <= 2 * 3 * 2 * 2 * it.arena.step

    count = [0]

    def patterned(rng, proba):
        rng.random()
        count[0] += 1
        return (count[0] * 7) % 3 == 0

    monkeypatch.setattr(datamodule, "_exchange_coin", patterned)
    ahead, ex_ahead, _, _ = run(cfg4, 2)
    count[0] = 0
    plain, ex_plain, alive, _ = run(cfg0, 0)
    assert not alive
    assert ex_ahead == ex_plain and any(e for batch in ex_plain for e in batch)
    for n, (x, y) in enumerate(zip(ahead, plain)):
        for k in ("image_ref", "image_trg"):
            assert torch.equal(x[k], y[k]), f"batch {n}: {k} differs between prefetch=2 and prefetch=0"
    assert not torch.equal(plain[0]["image_trg"], plain[1]["image_trg"])


def test_evaluation_loaders(dev, tree):
    """val (dims, the coin thrown per sample, batches of val_batch_size) and test (Resize 128 Lanczos, padded to one shape;
    RobotCarMatching through its load-time dims first) equal EvalIngest applied by hand to the same decoded pairs"""
    from refign_amd.datamodule import MatchingDataModule
    from refign_amd.datasets import MegaDepth, RobotCarMatching
    from refign_amd.resample import EvalIngest
    cfg = {"data": data_section(DIMS, CROP, batch_size=4, num_workers=2, elastic=False)}
    dm = MatchingDataModule(cfg, tree, dev)
    assert (dm.val_batch_size, dm.test_batch_size) == (2, 1)
    random.seed(3)
    val = list(dm.loaders("val")["MegaDepth"])
    after = random.random()
    random.seed(3)
    [random.random() for _ in range(28)]
    assert after == random.random()                          # one coin per val sample, at probability 0 too
    ds = MegaDepth(os.path.join(tree, "MegaDepth"), stage="val", load_keys=["image", "image_ref"])
    hand = EvalIngest(dims=(128, 160), dims_interpolation="lanczos", device=dev)
    assert len(val) == 14 and all(b["image"].shape == (2, 3, 128, 160) == b["image_ref"].shape for b in val)
    for n, b in enumerate(val):
        assert set(b) == {"image", "image_ref", "corr_pts", "corr_pts_ref", "filename"}
        assert isinstance(b["corr_pts"], list) and len(b["corr_pts"]) == len(b["corr_pts_ref"]) == 2
        for j in range(2):
            s = ds.decode(2 * n + j)
            want = hand(s["image"], image_ref=s["image_ref"], corr_pts=s["corr_pts"], corr_pts_ref=s["corr_pts_ref"])
            assert torch.equal(b["image"][j:j + 1], want["image"]) and torch.equal(b["image_ref"][j:j + 1], want["image_ref"])
            assert torch.equal(b["corr_pts"][j], want["corr_pts"][0]) and torch.equal(b["corr_pts_ref"][j], want["corr_pts_ref"][0])
            assert b["corr_pts"][j].is_cuda and b["corr_pts"][j].shape[1] == 2 and b["filename"][j] == ds.filename(2 * n + j)
    test = dm.loaders("test")
    assert list(test) == ["MegaDepth", "RobotCarMatching"]
    readers = {"MegaDepth": (MegaDepth(os.path.join(tree, "MegaDepth"), stage="test", load_keys=["image", "image_ref"]), None),
               "RobotCarMatching": (RobotCarMatching(os.path.join(tree, "RobotCarMatching"), stage="test"), (96, 96))}
    for name, (ds, dims) in readers.items():
        hand = EvalIngest(dims=dims, dims_interpolation="lanczos", resize=128, interpolation="lanczos", pad="same", device=dev)
        batches = list(test[name])
        assert len(batches) == 3
        for i, b in enumerate(batches):
            s = ds.decode(i)
            want = hand(s["image"], image_ref=s["image_ref"], corr_pts=s["corr_pts"], corr_pts_ref=s["corr_pts_ref"])
            assert b["image"].shape == b["image_ref"].shape and min(b["image"].shape[2:]) >= 128
            for k in ("image", "image_ref"):
                assert torch.equal(b[k], want[k]), (name, i, k)
            for k in ("corr_pts", "corr_pts_ref"):
                assert len(b[k]) == 1 and torch.equal(b[k][0], want[k][0]), (name, i, k)
    assert list(dm.loaders("test", datasets=["RobotCarMatching"])) == ["RobotCarMatching"]
    dm.close()
    assert not _decoders()


# ---- the command line ------------------------------------------------------------------------------------------------------
def _metric():
    return [{"class_path": "helpers.metrics.SparseEPE", "init_args": {"compute_on_step": False, "uncertainty_estimation": True}}]


@pytest.fixture(scope="module")
def yaml_path(tmp_path_factory):
    """uawarpc_stage2.yaml's model, optimizer, scheduler and trainer sections with the tree's data section"""
    import yaml
    logs = tmp_path_factory.mktemp("logs")
    cfg = {"seed_everything": 0, "data": data_section(DIMS, CROP, batch_size=2, num_workers=2, elastic=False),
           "model": {"class_path": "models.AlignmentModel", "init_args": {
               "pretrained": None,
               "alignment_backbone": {"class_path": "models.backbones.VGG",
                                      "init_args": {"model_type": "vgg16", "pretrained": "imagenet", "out_indices": [2, 3, 4]}},
               "alignment_head": {"class_path": "models.heads.UAWarpCHead",
                                  "init_args": {"in_index": [0, 1], "input_transform": "multiple_select",
                                                "estimate_uncertainty": True, "iterative_refinement": True}},
               "selfsupervised_loss": {"class_path": "models.losses.MultiScaleFlowLoss", "init_args": {"loss_type": "HuberLoss"}},
               "unsupervised_loss": {"class_path": "models.losses.WBipathLoss",
                                     "init_args": {"objective": "multi_scale_flow_loss", "loss_type": "HuberLoss",
                                                   "visibility_mask": True}},
               "metrics": {"val": {"MegaDepth": _metric()}, "test": {"MegaDepth": _metric(), "RobotCarMatching": _metric()}}}},
           "optimizer": {"class_path": "torch.optim.Adam", "init_args": {"lr": 0.00005, "weight_decay": 0.0004}},
           "lr_scheduler": {"class_path": "torch.optim.lr_scheduler.MultiStepLR",
                            "init_args": {"milestones": [100000, 150000, 200000], "gamma": 0.5}},
           "trainer": {"max_steps": 225000, "sync_batchnorm": True, "log_every_n_steps": 1,
                       "logger": {"class_path": "pytorch_lightning.loggers.TensorBoardLogger",
                                  "init_args": {"save_dir": str(logs), "name": "uawarpc_tiny"}},
                       "callbacks": [{"class_path": "pytorch_lightning.callbacks.LearningRateMonitor"},
                                     {"class_path": "pytorch_lightning.callbacks.ModelCheckpoint", "init_args": {"save_last": True}},
                                     {"class_path": "helpers.callbacks.ValEveryNSteps", "init_args": {"every_n_steps": 5000}}]}}
    path = tmp_path_factory.mktemp("cfg") / "uawarpc_tiny.yaml"
    path.write_text(yaml.safe_dump(cfg, sort_keys=False))
    return str(path)


NO_VGG = ["--set", "model.init_args.alignment_backbone.init_args.pretrained=null"]
EPE_KEYS = ("AEPE", "PCK_1", "PCK_3", "PCK_5", "PCK_10", "AUSE_AEPE")


@pytest.mark.parametrize("graph_step", [False, True])
def test_fit_from_the_folders(dev, tree, yaml_path, tmp_path, graph_step):
    """Four steps: Trainer(graph_step=True) runs two steps eagerly, captures on the third and replays the fourth."""
    from refign_amd import run
    from refign_amd.datamodule import MatchingDataModule
    handles = {}
    hist = run.main(["fit", "--config", yaml_path, "--data_dir", tree, "--save_dir", str(tmp_path), "--set", "trainer.max_steps=4",
                     "--set", "trainer.callbacks.2.init_args.every_n_steps=null"] + NO_VGG + (["--graph_step"] if graph_step else []),
                    handles=handles)
    tr, dm = handles["trainer"], handles["datamodule"]
    try:
        assert isinstance(dm, MatchingDataModule) and hist == [] and tr.model.global_step == 4
        assert torch.load(str(tmp_path / "last.ckpt"), map_location="cpu", weights_only=False)["global_step"] == 4
        rows = dict(tr.log_history)
        assert sorted(rows) == [0, 1, 2, 3]
        print([rows[s]["train_matching_loss"] for s in range(4)])
        assert all(np.isfinite(rows[s]["train_matching_loss"]) for s in range(4))
        if graph_step:
            assert not tr.step_graph.states or not any(s["failed"] for s in tr.step_graph.states.values()), "the capture failed"
            assert tr.step_graph.captured(), "the last step did not replay the graph"
        else:
            assert tr.step_graph is None
    finally:
        dm.close()
        tr.close()
        dm.close()
    assert not _decoders()


def test_validation_inside_fit(dev, tree, yaml_path, tmp_path):
    from refign_amd import run
    hist = run.main(["fit", "--config", yaml_path, "--data_dir", tree, "--save_dir", str(tmp_path), "--set", "trainer.max_steps=4",
                     "--set", "trainer.callbacks.2.init_args.every_n_steps=2"] + NO_VGG)
    assert [s for s, _ in hist] == [2, 4]
    for _, m in hist:
        assert set(m) == {"val_MegaDepth_SparseEPE_" + k for k in EPE_KEYS} and all(np.isfinite(v) for v in m.values())
    assert not _decoders()


def test_test_from_the_folders_equals_a_hand_fed_trainer(dev, tree, yaml_path, monkeypatch):
    """run.main(["test", ...]) over both sections == Trainer.test over the same decoded files fed by hand through EvalIngest,
    exactly; under RFN_EVAL_FUSED=0 the same keys within the tolerance tests/test_matcher_eval_gpu.py holds the two paths to."""
    from refign_amd import config, run
    from refign_amd.datasets import MegaDepth, RobotCarMatching
    from refign_amd.resample import EvalIngest
    from refign_amd.trainer import Trainer
    monkeypatch.delenv("RFN_EVAL_FUSED", raising=False)
    argv = ["test", "--config", yaml_path, "--data_dir", tree] + NO_VGG
    got = run.main(argv)
    want_keys = {f"test_{name}_SparseEPE_{k}" for name in ("MegaDepth", "RobotCarMatching") for k in EPE_KEYS}
    assert set(got) == want_keys and all(isinstance(v, float) and np.isfinite(v) for v in got.values())
    assert got["test_MegaDepth_SparseEPE_AEPE"] > 0.0 and got["test_RobotCarMatching_SparseEPE_AEPE"] > 0.0

    cfg = run.apply_set(config.load_config(yaml_path), NO_VGG[1:])
    run.seed_everything(0)
    model = config.build_model(cfg).to(dev).train()
    trainer = Trainer(model)
    loaders = {}
    for name, ds, dims in (("MegaDepth", MegaDepth(os.path.join(tree, "MegaDepth"), stage="test", load_keys=["image", "image_ref"]), None),
                           ("RobotCarMatching", RobotCarMatching(os.path.join(tree, "RobotCarMatching"), stage="test"), (96, 96))):
        ingest = EvalIngest(dims=dims, dims_interpolation="lanczos", resize=128, interpolation="lanczos", pad="same", device=dev)
        loaders[name] = []
        for i in range(len(ds)):
            s = ds.decode(i)
            loaders[name].append(ingest(s["image"], image_ref=s["image_ref"], corr_pts=s["corr_pts"], corr_pts_ref=s["corr_pts_ref"]))
    by_hand = trainer.test(loaders)
    trainer.close()
    print(got, by_hand)
    assert got == by_hand

    monkeypatch.setenv("RFN_EVAL_FUSED", "0")
    host = run.main(argv)
    assert set(host) == want_keys
    for k, v in host.items():
        print(k, got[k], v)
        assert abs(got[k] - v) <= 1e-6 * max(1.0, abs(v)), k


def test_predict_is_out_of_scope_and_graph_step_is_the_matchers(dev, tree, yaml_path, tmp_path):
    """predict with the matcher: the module's OutOfScopeError.  --graph_step with the UDA model: the Trainer's own ValueError
    (the small HRDA model of tests/test_datamodule_gpu.py; nothing is read from its folders before the Trainer refuses)."""
    import copy
    import bench
    import yaml
    from datamodule_tree import data_section as uda_section
    from test_datamodule_gpu import SHRINK
    from refign_amd import config, run
    with pytest.raises(config.OutOfScopeError, match="predict_step"):
        run.main(["predict", "--config", yaml_path, "--data_dir", tree] + NO_VGG)
    assert not _decoders()
    cfg = copy.deepcopy(bench.REF_CFG)
    cfg["data"] = uda_section("ACDC", (128, 128), (128, 256), (136, 240), batch_size=4)
    cfg["trainer"] = {"max_steps": 2, "precision": "bf16"}
    uda = tmp_path / "uda.yaml"
    uda.write_text(yaml.safe_dump(cfg, sort_keys=False))
    with pytest.raises(ValueError, match="graph_step=True is for a model with automatic_optimization"):
        run.main(["fit", "--config", str(uda), "--data_dir", tree, "--graph_step"] + [a for s in SHRINK for a in ("--set", s)])

"""Trainer.fit / validate / test on the CPU: the loop logic only -- the model of test_resume_cpu._trainer with
`training_step` / `validation_step` replaced by recording stubs (the product has no CPU compute path) -- plus
IoU.add_confusion, config.trainer_kwargs and a two-rank validation over gloo with loaders of different lengths."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml
from test_ddp_cpu import _free_port
from test_resume_cpu import _trainer


def _batches(n):
    return [{"image_src": torch.tensor([float(i)])} for i in range(n)]


def _stub_training(trainer, log):
    model = trainer.model

    def training_step(batch, batch_idx):
        nxt = batch.get("image_src_next")
        log.append(("step", int(batch["image_src"]), None if nxt is None else int(nxt), model.training))
        model.global_step += 1

    model.training_step = training_step


def _stub_validation(trainer, log, fail_at=None):
    from refign_amd.metrics import IoU, MyMetricCollection
    model = trainer.model
    model.valid_metrics = MyMetricCollection({"val_ACDC_IoU": IoU(num_classes=4, ignore_index=255),
                                              "val_DarkZurich_IoU": IoU(num_classes=4, ignore_index=255)})

    def validation_step(batch, batch_idx=0, dataloader_idx=0, src_name=""):
        log.append(("val", batch_idx, dataloader_idx, src_name, model.training, torch.is_grad_enabled()))
        if fail_at == (dataloader_idx, batch_idx):
            raise RuntimeError("bad batch")
        for k, m in model.valid_metrics.items():
            if src_name in k:
                m(batch["pred"], batch["semantic"])

    model.validation_step = validation_step


def _val_batch(seed, n=1):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, 4, (n, 6, 7), generator=g)
    y[:, 0] = 255
    return {"pred": torch.randint(0, 4, (n, 6, 7), generator=g), "semantic": y}


def test_fit_steps_validates_and_looks_one_batch_ahead():
    tr = _trainer()
    log = []
    _stub_training(tr, log)
    _stub_validation(tr, log)
    tr.model.train()
    out = tr.fit(_batches(4), val_loaders={"ACDC": [_val_batch(1)]}, max_steps=7, val_every_n_steps=3)
    steps = [e for e in log if e[0] == "step"]
    # 7 steps over a 4-batch iterable taken again from its start; each step sees its successor's batch, the last one None
    assert [(e[1], e[2]) for e in steps] == [(0, 1), (1, 2), (2, 3), (3, 0), (0, 1), (1, 2), (2, None)]
    assert all(e[3] for e in steps), "a training step ran in eval mode"
    kinds = [e[0] for e in log]
    assert kinds == ["step"] * 3 + ["val"] + ["step"] * 3 + ["val"] + ["step"]          # after steps 3 and 6 only
    assert [s for s, _ in out] == [3, 6] and all(set(m) == {"val_ACDC_IoU", "val_DarkZurich_IoU"} for _, m in out)
    assert all(isinstance(v, float) for _, m in out for v in m.values())
    assert tr.model.global_step == 7 and tr.model.training
    # without validation loaders nothing is validated, and a run that is already at max_steps takes no step
    del log[:]
    assert tr.fit(_batches(4), max_steps=9, val_every_n_steps=1) == [] and [e[0] for e in log] == ["step"] * 2
    assert tr.fit(_batches(4), max_steps=9) == [] and len(log) == 2
    with pytest.raises(ValueError, match="empty"):
        tr.fit([], max_steps=11)
    tr.close()


def test_fit_keeps_last_ckpt_and_resumes_from_it(tmp_path):
    a = _trainer()
    log, seen = [], []
    _stub_training(a, log)
    _stub_validation(a, log)
    real_validate = a.validate

    def validate(loaders):
        out = real_validate(loaders)
        seen.append(os.path.exists(tmp_path / "last.ckpt"))      # (the file of THIS validation is written after it)
        return out

    a.validate = validate
    real_save = a.save_checkpoint
    saves = []
    a.save_checkpoint = lambda path, **k: (saves.append((path, a.model.global_step)), real_save(path, **k))[1]
    a.fit(_batches(4), val_loaders=[_val_batch(1)], max_steps=7, val_every_n_steps=3, ckpt_dir=str(tmp_path))
    last = str(tmp_path / "last.ckpt")
    assert saves == [(last, 3), (last, 6), (last, 7)] and seen == [False, True]
    assert torch.load(last, map_location="cpu", weights_only=False)["global_step"] == 7
    # saved at step 3: a new trainer continues with exactly 4 steps; from the final file: none
    mid = str(tmp_path / "mid" / "last.ckpt")
    c = _trainer()
    _stub_training(c, [])
    c.fit(_batches(4), max_steps=3, ckpt_dir=str(tmp_path / "mid"))
    assert torch.load(mid, map_location="cpu", weights_only=False)["global_step"] == 3
    c.close()
    for path, want in ((mid, 4), (last, 0)):
        b = _trainer(ckpt_path=path)
        blog = []
        _stub_training(b, blog)
        b.fit(_batches(4), max_steps=7, ckpt_dir=None)
        assert len(blog) == want and b.model.global_step == 7
        b.close()
    # save_last=False writes nothing
    d = _trainer()
    _stub_training(d, [])
    d.fit(_batches(2), max_steps=2, ckpt_dir=str(tmp_path / "none"), save_last=False)
    assert not os.path.exists(tmp_path / "none")
    d.close()
    a.close()


def test_validate_names_modes_and_reset():
    tr = _trainer()
    log = []
    _stub_validation(tr, log)
    model = tr.model.train()
    model.head.eval()                                  # a mode of the caller's own: it comes back as it was
    out = tr.validate({"ACDC": [_val_batch(1), _val_batch(2)], "DarkZurich": [_val_batch(3)]})
    assert [e[1:4] for e in log] == [(0, 0, "ACDC"), (1, 0, "ACDC"), (0, 1, "DarkZurich")]
    assert all(not e[4] and not e[5] for e in log), "validation_step ran in training mode or with autograd on"
    assert model.training and not model.head.training and model.backbone.training
    assert not model.alignment_backbone.training and not model.alignment_head.training
    assert set(out) == {"val_ACDC_IoU", "val_DarkZurich_IoU"} and out["val_ACDC_IoU"] != out["val_DarkZurich_IoU"]
    assert all(int(m.confmat.sum()) == 0 for m in model.valid_metrics.values())          # reset at epoch end
    # one bare iterable: name "", dataloader_idx 0, every metric takes part
    del log[:]
    both = tr.validate([_val_batch(1)])
    assert [e[1:4] for e in log] == [(0, 0, "")] and both["val_ACDC_IoU"] == both["val_DarkZurich_IoU"]
    # an eval-mode model stays in eval mode
    model.eval()
    tr.validate([_val_batch(1)])
    assert not model.training and not model.backbone.training
    # a step that raises: the mode comes back and the half-filled metrics are reset
    model.train()
    _stub_validation(tr, log, fail_at=(0, 1))
    with pytest.raises(RuntimeError, match="bad batch"):
        tr.validate({"ACDC": [_val_batch(1), _val_batch(2)]})
    assert model.training and not model.alignment_head.training
    assert all(int(m.confmat.sum()) == 0 for m in model.valid_metrics.values())
    tr.close()


def test_test_loop_uses_the_test_metrics():
    from refign_amd.metrics import IoU, MyMetricCollection
    tr = _trainer()
    model = tr.model
    model.test_metrics = MyMetricCollection({"test_ACDC_IoU": IoU(num_classes=4, ignore_index=255, average="none")})
    calls = []

    def test_step(batch, batch_idx=0, dataloader_idx=0, src_name=""):
        calls.append((batch_idx, dataloader_idx, src_name))
        model.test_metrics["test_ACDC_IoU"](batch["pred"], batch["semantic"])

    model.test_step = test_step
    out = tr.test({"ACDC": [_val_batch(4), _val_batch(5)]})
    assert calls == [(0, 0, "ACDC"), (1, 0, "ACDC")]
    assert isinstance(out["test_ACDC_IoU"], list) and len(out["test_ACDC_IoU"]) == 4       # per-class values: a list
    tr.close()


def test_add_confusion_equals_update():
    from refign_amd.metrics import IoU
    b = _val_batch(7, n=3)
    a, c = IoU(num_classes=4, ignore_index=255), IoU(num_classes=4, ignore_index=255)
    a.update(b["pred"], b["semantic"])
    keep = b["semantic"] != 255
    delta = torch.zeros(4, 4, dtype=torch.long)
    for t, p in zip(b["semantic"][keep].tolist(), b["pred"][keep].tolist()):
        delta[t, p] += 1
    c.add_confusion(delta)
    c.add_confusion(torch.zeros(4, 4, dtype=torch.int32))
    assert torch.equal(a.confmat, c.confmat) and float(a.compute()) == float(c.compute())
    with pytest.raises(ValueError):
        c.add_confusion(torch.zeros(3, 4, dtype=torch.long))
    with pytest.raises(ValueError):
        c.add_confusion(torch.zeros(4, 4))


TRAINER_YAML = """
trainer:
  max_steps: 40000
  check_val_every_n_epoch: 40000
  sync_batchnorm: True
  multiple_trainloader_mode: min_size
  precision: 16
  logger:
    - class_path: pytorch_lightning.loggers.TensorBoardLogger
      init_args:
        save_dir: lightning_logs
        name: some_run
  callbacks:
    - class_path: pytorch_lightning.callbacks.LearningRateMonitor
    - class_path: helpers.callbacks.ValEveryNSteps
      init_args:
        every_n_steps: 4000
    - class_path: pytorch_lightning.callbacks.ModelCheckpoint
      init_args:
        save_last: True
"""


def test_trainer_kwargs_from_a_yaml():
    from refign_amd import config
    from refign_amd.trainer import ValEveryNSteps
    got = config.trainer_kwargs(yaml.safe_load(TRAINER_YAML))
    assert got == {"max_steps": 40000, "val_every_n_steps": 4000, "save_last": True, "sync_batchnorm": True, "precision": 16}
    bare = config.trainer_kwargs(yaml.safe_load("trainer:\n  max_steps: 100\n"))
    assert bare == {"max_steps": 100, "val_every_n_steps": None, "save_last": False, "sync_batchnorm": False,
                    "precision": None}
    assert config.trainer_kwargs({}) == dict(bare, max_steps=None)
    # the callback still builds from its spec, and carries the rule fit() applies
    cb = config.build({"class_path": "helpers.callbacks.ValEveryNSteps", "init_args": {"every_n_steps": 3}})
    assert isinstance(cb, ValEveryNSteps) and cb.every_n_steps == 3
    assert [s for s in range(8) if cb.should_validate(s)] == [3, 6]


def _two_rank_validate_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RFN_STALL_S="120")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    tr = _trainer()
    log = []
    _stub_validation(tr, log)
    mine = [_val_batch(10)] if rank == 0 else [_val_batch(11), _val_batch(12), _val_batch(13)]
    res = tr.validate({"ACDC": mine})
    torch.save({"iou": res["val_ACDC_IoU"], "batches": len(log), "note": tr.guard.progress[1]}, f"{out}/r{rank}.pt")
    tr.close()
    dist.destroy_process_group()


def test_two_ranks_with_loaders_of_different_lengths(tmp_path):
    """Ranks with 1 and 3 validation batches: nobody waits inside the loop (the only collective is the metrics' sum at the
    end), and both return the IoU of all four batches."""
    from refign_amd.metrics import IoU
    port, out = _free_port(), str(tmp_path)
    mp.spawn(_two_rank_validate_worker, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = (torch.load(f"{out}/r{k}.pt", weights_only=False) for k in range(2))
    assert (r0["batches"], r1["batches"]) == (1, 3)
    whole = IoU(num_classes=4, ignore_index=255)
    for seed in (10, 11, 12, 13):
        b = _val_batch(seed)
        whole.update(b["pred"], b["semantic"])
    assert r0["iou"] == r1["iou"] == float(whole.compute())
    assert r0["note"] == r1["note"] == "validation done"

"""Trainer.save_checkpoint / load_checkpoint on the CPU: the Lightning 1.5.10 layout of the file, the weights-only form
through `pretrained=`, a save that fails part-way, the state that comes back bit for bit, the mismatches that load with a
warning, and the stall guard's pause around checkpoint I/O."""
import os
import random
import time

import numpy as np
import pytest
import torch
from test_checkpoint_cpu import _reference_state_dict, ours

GROUPS = ["head_weight", "head_bias", "backbone_weight", "backbone_bias"]


def _trainer(precision=None, **kw):
    from fill import closed_form_fill
    from refign_amd.trainer import Trainer
    return Trainer(closed_form_fill(ours()), fused_optimizer=False, precision=precision, **kw)


def _advance(trainer, steps=2, seed=3):
    """torch's AdamW steps on seeded gradients + scheduler steps: moments, step counts and LR that a resume must carry."""
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        trainer.grads.flat.copy_(torch.randn(trainer.grads.flat.shape, generator=gen))
        trainer.optimizer.step()
        trainer.scheduler.step()
        trainer.model.global_step += 1


def test_file_has_the_lightning_layout(tmp_path):
    """Top-level keys of Lightning 1.5.10, param groups by name in the reference's order, `state_dict` in the keys the
    reference's strict loader takes (tests/golden/ref_checkpoint_hrda_mit_b0.json), the project's own key alongside."""
    for precision in (None, 16):
        tr = _trainer(precision)
        _advance(tr)
        path = str(tmp_path / f"last_{precision}.ckpt")
        tr.save_checkpoint(path)
        ck = torch.load(path, map_location="cpu", weights_only=False)
        keys = {"epoch", "global_step", "pytorch-lightning_version", "state_dict", "loops", "callbacks", "optimizer_states",
                "lr_schedulers", "refign_amd"} | ({"native_amp_scaling_state"} if precision == 16 else set())
        assert set(ck) == keys
        assert ck["pytorch-lightning_version"] == "1.5.10" and ck["global_step"] == 2 and ck["callbacks"] == {}
        assert ck["loops"]["fit_loop"]["epoch_loop.batch_progress"]["total"]["completed"] == 2
        assert len(ck["optimizer_states"]) == 1 and len(ck["lr_schedulers"]) == 1
        opt = ck["optimizer_states"][0]
        assert [g["name"] for g in opt["param_groups"]] == GROUPS
        assert [g["params"] for g in opt["param_groups"]] == [g["params"] for g in tr.optimizer.state_dict()["param_groups"]]
        assert all(float(s["step"]) == 2.0 for s in opt["state"].values())
        assert ck["lr_schedulers"][0]["last_epoch"] == 2
        sr, sd = _reference_state_dict(), ck["state_dict"]
        assert list(sd) == list(tr.model.state_dict())
        assert set(sd) == set(sr), sorted(set(sd) ^ set(sr))[:10]
        assert all(sd[k].shape == sr[k].shape and sd[k].dtype == sr[k].dtype for k in sr)
        own = ck["refign_amd"]
        assert own["world_size"] == 1 and len(own["rng"]) == 1 and own["precision"] == ("16" if precision == 16 else None)
        if precision == 16:
            assert set(ck["native_amp_scaling_state"]) == {"scale", "growth_factor", "backoff_factor", "growth_interval",
                                                           "_growth_tracker"}
        # the whole file is plain data: torch's restricted loader reads it
        torch.load(path, map_location="cpu", weights_only=True)
        tr.close()


def test_weights_only_file_loads_through_pretrained(tmp_path):
    tr = _trainer()
    with torch.no_grad():
        for p in tr.model.parameters():
            p.mul_(1.25)
    tr.model.global_step = 5
    path = str(tmp_path / "weights.ckpt")
    tr.save_checkpoint(path, weights_only=True)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"epoch", "global_step", "pytorch-lightning_version", "state_dict"} and ck["global_step"] == 5
    b = ours(pretrained=path)
    sa, sb = tr.model.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    with pytest.raises(KeyError, match="model only"):            # not a file to continue a run from
        _trainer(ckpt_path=path)
    tr.close()


def test_failed_save_leaves_the_previous_file(tmp_path, monkeypatch):
    from refign_amd import trainer as T
    tr = _trainer()
    path = str(tmp_path / "last.ckpt")
    tr.save_checkpoint(path)
    before = open(path, "rb").read()
    _advance(tr)

    def failing(obj, f):
        f.write(b"\0" * 4096)
        raise OSError("disk full")

    monkeypatch.setattr(T, "_write_file", failing)
    with pytest.raises(OSError, match="disk full"):
        tr.save_checkpoint(path)
    assert open(path, "rb").read() == before
    assert os.listdir(tmp_path) == ["last.ckpt"]                   # no temporary file left behind
    monkeypatch.undo()
    tr.save_checkpoint(path)
    assert torch.load(path, map_location="cpu", weights_only=False)["global_step"] == 2
    tr.close()


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_state_comes_back_bit_for_bit(tmp_path):
    """Parameters, buffers, moments, step counts, scheduler, loss scaler, global_step and the host RNG streams of a fresh
    trainer built with ckpt_path= equal what was saved; the next draws are the ones the saving process makes next."""
    a = _trainer(16, scaler_args={"init_scale": 2.0 ** 9, "growth_interval": 3})
    _advance(a, 3)
    a.scaler._scale.fill_(1024.0)
    a.scaler._growth_tracker.fill_(2)
    random.seed(21); np.random.seed(21); torch.manual_seed(21)
    path = str(tmp_path / "last.ckpt")
    a.save_checkpoint(path)
    want = (random.random(), float(np.random.uniform()), float(torch.rand(1)))
    b = _trainer(16, ckpt_path=path)
    got = (random.random(), float(np.random.uniform()), float(torch.rand(1)))
    assert got == want
    assert _same(a.model.state_dict(), b.model.state_dict()) and b.model.global_step == 3
    assert _same(a.optimizer.state_dict(), b.optimizer.state_dict())
    assert _same(a.scheduler.state_dict(), b.scheduler.state_dict())
    assert [g["lr"] for g in a.optimizer.param_groups] == [g["lr"] for g in b.optimizer.param_groups]
    assert a.scaler.state_dict() == b.scaler.state_dict() and b.scaler.get_scale() == 1024.0
    a.close()
    b.close()


def test_mismatched_files_load_with_one_warning_each(tmp_path):
    """A scaler state into a trainer without loss scaling is ignored, a file without one into an fp16 trainer starts the
    scaler fresh, a file without the project's key (a Lightning file) seeds the RNGs from (global_step, rank)."""
    a = _trainer(16)
    _advance(a)
    path = str(tmp_path / "fp16.ckpt")
    a.save_checkpoint(path)
    with pytest.warns(UserWarning, match="ignored") as rec:
        _trainer("bf16", ckpt_path=path).close()
    assert len(rec) == 1
    ck = torch.load(path, map_location="cpu", weights_only=False)
    del ck["native_amp_scaling_state"], ck["refign_amd"]
    lightning = str(tmp_path / "lightning.ckpt")
    torch.save(ck, lightning)
    with pytest.warns(UserWarning) as rec:
        b = _trainer(16, scaler_args={"init_scale": 8.0}, ckpt_path=lightning)
    msgs = sorted(str(w.message) for w in rec)
    assert len(msgs) == 2 and "starts fresh" in msgs[1] and "seeded from (global_step, rank)" in msgs[0], msgs
    assert b.scaler.get_scale() == 8.0 and b.model.global_step == 2
    assert _same(a.optimizer.state_dict()["state"], b.optimizer.state_dict()["state"])
    draws = random.random()
    random.seed(2 * 1000003)
    assert draws == random.random()
    a.close()
    b.close()


def test_stall_guard_does_not_fire_while_paused(monkeypatch):
    from refign_amd.trainer import StallGuard
    fired = []
    monkeypatch.setattr(os, "_exit", lambda code: fired.append(code))
    g = StallGuard(0, 2, limit=0.4)
    g.note("step")
    with g.paused("save_checkpoint"):
        time.sleep(1.5)
    assert fired == []
    time.sleep(1.5)                                                # and it still watches once the I/O is over
    assert fired and fired[0] == 17
    g.stop()
    g._thread.join(timeout=5)
    assert not g._thread.is_alive()


def test_close_stops_the_stall_guard(monkeypatch):
    from refign_amd.trainer import StallGuard
    monkeypatch.setattr(os, "_exit", lambda code: None)
    tr = _trainer()
    g = tr.guard = StallGuard(0, 2, limit=60)
    tr.close()
    g._thread.join(timeout=20)
    assert tr.guard is None and not g._thread.is_alive()

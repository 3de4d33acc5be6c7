"""GPU: the matcher (AlignmentModel) trained through Trainer -- one step against the recorded reference step, three steps
against the hand-driven loop, the per-step scheduler, no host synchronisation, fp16 overflow, checkpoints, and the UDA
model's path untouched."""
import numpy as np
import pytest
import torch
from conftest import golden
from test_matcher_gpu import build_matcher, matcher_batch

pytestmark = pytest.mark.gpu

LR, WD = 5e-5, 4e-4
LOSSES = ("train_matching_loss", "train_ss_loss", "train_us_loss")
NEW_ENTRY_POINTS = ("rfn_flowloss_fwd_f32", "rfn_flowloss_bwd_f32", "rfn_flowloss_block_pixels", "rfn_multi_adam_f32",
                    "rfn_multi_adam_amp_f32")
# a loss scale at which this batch's fp16 backward does not overflow: the closed-form-filled head has a gradient norm of 7.3e4
# on it, and a first step at 2^8 .. 2^16 is skipped (measured on an MI355X; 2^4 and 2^0 pass)
FP16_SCALE = 2.0 ** 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def z():
    return golden("matcher_step_128x160")


def build(dev, milestones=(100000, 150000), gamma=0.5):
    model = build_matcher(dev)
    model.optimizer_init = {"class_path": "torch.optim.Adam", "init_args": {"lr": LR, "weight_decay": WD}}
    model.lr_scheduler_init = {"class_path": "torch.optim.lr_scheduler.MultiStepLR",
                               "init_args": {"milestones": list(milestones), "gamma": gamma}}
    return model


class Memory:
    def __init__(self):
        self.rows = []

    def log_metrics(self, metrics, step):
        self.rows.append((step, dict(metrics)))

    def flush(self):
        pass

    def close(self):
        pass


def _logged(model):
    return [float(model.logged[k]) for k in LOSSES]


def _snapshot(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _params(module):
    """(BatchNorm's running statistics move in every training-mode forward, skipped step or not: parameters only)"""
    return {k: v.detach().clone() for k, v in module.named_parameters()}


def test_one_trainer_step_matches_the_reference_step(dev, z):
    """Losses to 2e-4 and per-submodule gradient norms (read from trainer.grads) to 2e-3 of the recorded reference step; the
    step is taken: global_step 1, head parameters changed, the frozen backbone bit-equal."""
    from refign_amd.optim import MultiTensorAdam
    from refign_amd.trainer import Trainer
    model = build(dev)
    before = _snapshot(model)
    trainer = Trainer(model)
    assert isinstance(trainer.fast_step, MultiTensorAdam) and type(trainer.optimizer) is torch.optim.Adam
    assert not trainer.optimizer.param_groups[0].get("fused")
    trainer.step(matcher_batch(z, dev), 0)
    got = _logged(model)
    print(f"\nlogged {got} golden {[float(z[k]) for k in ('loss', 'ss_loss', 'us_loss')]}")
    for v, key in zip(got, ("loss", "ss_loss", "us_loss")):
        assert abs(v - float(z[key])) <= 2e-4 * abs(float(z[key])), key
    flat = trainer.grads.flat
    lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * flat.numel()
    for name, mod in model.alignment_head.named_children():
        key = "gradnorm/" + name
        if key in z:
            g = [p.grad for p in mod.parameters() if p.requires_grad]
            assert all(lo <= x.data_ptr() < hi for x in g)            # views of the trainer's flat buffer
            norm = float(torch.sqrt(sum((x.double() ** 2).sum() for x in g)))
            assert abs(norm - float(z[key])) <= 2e-3 * float(z[key]), (name, norm, float(z[key]))
    assert model.global_step == 1
    after = model.state_dict()
    moved = {k: not torch.equal(before["alignment_head." + k], p.detach()) for k, p in model.alignment_head.named_parameters()}
    assert all(moved.values()), [k for k, m in moved.items() if not m]
    assert all(torch.equal(v, after[k]) for k, v in before.items() if k.startswith("alignment_backbone."))
    trainer.close()


def _hand_loop(dev, batch, steps=3):
    """The loop of test_matcher_gpu.test_matcher_trains with this file's optimizer and scheduler."""
    model = build(dev)
    (opt,), (sch,) = model.configure_optimizers()
    rows = []
    for _ in range(steps):
        opt.zero_grad()
        loss = model.training_step(batch, 0)
        loss.backward()
        opt.step()
        sch["scheduler"].step()
        rows.append(_logged(model))
    return np.asarray(rows)


def test_three_trainer_steps_follow_the_hand_driven_loop(dev, z):
    """Three steps on one batch.  The backward passes add with atomics, so the yardstick is the hand loop's own spread s
    between two runs, per step and loss; the Trainer's losses lie within max(4 s, 1e-4 relative) of the hand loop's.
    Measured on an MI355X (profiles/matcher_trainer_parity.txt): s = 0 for all three losses at step 1 and for the total at every
    step; at step 2 s = 3.1e-5 on train_ss_loss (355.27); at step 3 s = 1.2e-4 on train_ss_loss (345.96) and 1.5e-5 on
    train_us_loss (190.63), i.e. at most 3.5e-7 relative -- so the bound in force is the 1e-4 relative one.  The Trainer's
    losses differed from the hand loop's by exactly those amounts."""
    from refign_amd.trainer import Trainer
    batch = matcher_batch(z, dev)
    a, b = _hand_loop(dev, batch), _hand_loop(dev, batch)
    spread = np.abs(a - b)
    model = build(dev)
    trainer = Trainer(model)
    got = []
    for it in range(3):
        trainer.step(batch, it)
        got.append(_logged(model))
    got = np.asarray(got)
    bound = np.maximum(4 * spread, 1e-4 * np.abs(a))
    print(f"\nhand loop\n{a}\nspread between two hand-loop runs\n{spread}\ntrainer\n{got}\n|trainer - hand|\n{np.abs(got - a)}"
          f"\nbound\n{bound}")
    assert np.isfinite(got).all()
    assert (np.abs(got - a) <= bound).all()
    assert model.global_step == 3
    trainer.close()


def test_scheduler_steps_once_per_trainer_step(dev, z):
    """MultiStepLR(milestones=[2, 3], gamma=0.5): steps 0..3 use lr, lr, lr/2, lr/4 -- in the logged rows and in param_groups."""
    from refign_amd.trainer import Trainer
    model = build(dev, milestones=(2, 3))
    trainer = Trainer(model, logger=Memory(), log_every_n_steps=1)
    batch = matcher_batch(z, dev)
    used = []
    for it in range(4):
        used.append(trainer.optimizer.param_groups[0]["lr"])
        trainer.step(batch, it)
    trainer.flush_log()
    want = [LR, LR, LR / 2, LR / 4]
    assert used == pytest.approx(want, rel=1e-12)
    assert [s for s, _ in trainer.log_history] == [0, 1, 2, 3]
    assert [row["lr-Adam/0"] for _, row in trainer.log_history] == pytest.approx(want, rel=1e-6)
    for _, row in trainer.log_history:
        assert all(k in row and np.isfinite(row[k]) for k in LOSSES) and row["grad_norm/total"] > 0
    assert trainer.optimizer.param_groups[0]["lr"] == pytest.approx(LR / 4, rel=1e-12)
    trainer.close()


@pytest.mark.parametrize("precision", [None, 16])
def test_second_trainer_step_does_not_synchronise(dev, z, precision):
    from refign_amd.trainer import Trainer
    model = build(dev)
    trainer = Trainer(model, precision=precision, scaler_args={"init_scale": FP16_SCALE} if precision else None)
    batch = matcher_batch(z, dev)
    batch["prime_trg_idx"] = torch.tensor(batch["prime_trg_idx"], device=dev)
    trainer.step(batch, 0)
    torch.cuda.synchronize(dev)
    before = _params(model.alignment_head)
    torch.cuda.set_sync_debug_mode("error")
    try:
        trainer.step(batch, 1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert model.global_step == 2 and trainer.fast_step.launches == 1
    assert any(not torch.equal(v, before[k]) for k, v in model.alignment_head.named_parameters())
    assert all(np.isfinite(v) for v in _logged(model))
    trainer.close()


def test_host_list_prime_trg_idx_does_not_synchronise_either(dev, z):
    from refign_amd.trainer import Trainer
    model = build(dev)
    trainer = Trainer(model)
    batch = matcher_batch(z, dev)
    assert isinstance(batch["prime_trg_idx"], list)
    trainer.step(batch, 0)
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        trainer.step(batch, 1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert model.global_step == 2
    trainer.close()


def _optimizer_state(trainer):
    sd = trainer.optimizer.state_dict()
    return {(i, k): (v.detach().cpu().clone() if torch.is_tensor(v) else v) for i, st in sd["state"].items() for k, v in st.items()}


def _same_state(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


def test_fp16_overflow_skips_the_step_and_recovers(dev, z):
    """precision=16 with a scale that overflows: parameters (and, once they exist, both moments) stay bit-equal, the scale
    halves, the scheduler and global_step advance; at a workable scale the next step updates.  The first overflow is decided
    by the host (torch's Adam has no state yet), the later one on the device (rfn_multi_adam_amp_f32)."""
    from refign_amd.trainer import Trainer
    model = build(dev, milestones=(1, 100))
    huge = 2.0 ** 100
    trainer = Trainer(model, precision=16, scaler_args={"init_scale": huge})
    batch = matcher_batch(z, dev)
    p0 = _params(model.alignment_head)
    trainer.step(batch, 0)
    assert all(torch.equal(v, p0[k]) for k, v in model.alignment_head.named_parameters())
    assert trainer.scaler.get_scale() == huge / 2 and trainer.scaler.skipped_steps() == 1
    assert model.global_step == 1 and trainer.scheduler.last_epoch == 1
    assert trainer.optimizer.param_groups[0]["lr"] == pytest.approx(LR / 2)
    for it in (1, 2):                                        # torch's step (creates the state), then the one-launch step
        trainer.scaler._scale.fill_(FP16_SCALE)
        trainer.step(batch, it)
    assert trainer.scaler.skipped_steps() == 1 and trainer.fast_step.launches == 1
    assert any(not torch.equal(v, p0[k]) for k, v in model.alignment_head.named_parameters())
    p1, s1 = _params(model.alignment_head), _optimizer_state(trainer)
    trainer.scaler._scale.fill_(huge)
    trainer.step(batch, 3)
    assert trainer.fast_step.launches == 2                    # launched, and did nothing
    params = dict(model.alignment_head.named_parameters())
    assert all(torch.equal(v, p1[k]) for k, v in params.items())
    assert _same_state(_optimizer_state(trainer), s1)
    assert trainer.scaler.get_scale() == huge / 2 and trainer.scaler.skipped_steps() == 2
    assert model.global_step == 4 and trainer.scheduler.last_epoch == 4
    trainer.scaler._scale.fill_(FP16_SCALE)
    trainer.step(batch, 4)
    assert any(not torch.equal(v, p1[k]) for k, v in params.items())
    assert trainer.scaler.skipped_steps() == 2
    trainer.close()


def test_checkpoint_round_trip_and_fit(dev, z, tmp_path):
    from refign_amd.trainer import Trainer
    batch = matcher_batch(z, dev)
    model = build(dev, milestones=(1, 100))
    trainer = Trainer(model, precision=16, scaler_args={"init_scale": FP16_SCALE, "growth_interval": 3})
    for it in range(2):
        trainer.step(batch, it)
    path = str(tmp_path / "two.ckpt")
    trainer.save_checkpoint(path)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert ckpt["global_step"] == 2 and set(ckpt["state_dict"]) == set(model.state_dict())
    assert "native_amp_scaling_state" in ckpt and len(ckpt["optimizer_states"]) == 1
    fresh = build(dev, milestones=(1, 100))
    with torch.no_grad():
        for p in fresh.alignment_head.parameters():
            p.add_(1.0)                                      # everything that matters must come from the file
    resumed = Trainer(fresh, precision=16, scaler_args={"init_scale": 4.0}, ckpt_path=path)
    assert fresh.global_step == 2
    a, b = model.state_dict(), fresh.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    sa, sb = _optimizer_state(trainer), _optimizer_state(resumed)
    assert any(k[1] == "exp_avg" for k in sa) and all(float(v) == 2.0 for k, v in sa.items() if k[1] == "step")
    assert _same_state(sa, sb)
    assert trainer.scheduler.state_dict() == resumed.scheduler.state_dict()
    assert trainer.scaler.state_dict() == resumed.scaler.state_dict()
    assert resumed.optimizer.param_groups[0]["lr"] == pytest.approx(LR / 2)
    trainer.close()
    out = resumed.fit([batch], max_steps=3, ckpt_dir=str(tmp_path / "run"))
    assert out == [] and fresh.global_step == 3
    last = torch.load(str(tmp_path / "run" / "last.ckpt"), map_location="cpu", weights_only=False)
    assert last["global_step"] == 3
    assert all(float(st["step"]) == 3.0 for st in last["optimizer_states"][0]["state"].values())
    resumed.close()


def test_uda_step_calls_no_new_entry_point(dev, monkeypatch):
    """One step of the small DAFormer model of tests/test_step_gpu.py: none of the entry points this feature added is called."""
    from test_resume_gpu import _seed
    from test_step_gpu import build as build_uda
    from test_step_gpu import make_batch
    from refign_amd import _lib
    from refign_amd.trainer import Trainer
    lib = _lib.load_library()
    calls = {}
    for name in NEW_ENTRY_POINTS:
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    _seed(5)
    t = Trainer(build_uda(False, dev), precision="bf16")
    for it in range(2):
        t.step(make_batch(2, 128, 128, 64, dev), it)
    torch.cuda.synchronize(dev)
    t.close()
    assert calls == {}, calls

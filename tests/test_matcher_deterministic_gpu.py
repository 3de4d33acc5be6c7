"""GPU: Trainer(deterministic=True) for the matcher -- steps of the `matcher_step_128x160` golden repeat bit for bit: two fresh
runs, eager and replayed from a hipGraph, fp32 and the fp16 recipe, and across a save and a resume.  The mode reaches the matcher
through its widening (determinism.scatter_forms: the order-free warp backward of csrc/warp.hip); the UDA model keeps the plain
mode and its refusals, and the default mode calls none of the new entry points."""
import numpy as np
import pytest
import torch
from conftest import golden
from test_matcher_gpu import build_matcher, matcher_batch

pytestmark = pytest.mark.gpu

LR, WD = 5e-5, 4e-4
LOSSES = ("train_matching_loss", "train_ss_loss", "train_us_loss")
FP16_SCALE = 2.0 ** 4                  # as in test_matcher_trainer_gpu.py: this batch's fp16 backward does not overflow at it
NEW_ENTRY_POINTS = ("rfn_warp_bwd_det_f32", "rfn_warp_bwd_det_workspace_bytes", "rfn_corr_bwd_gather_f32")


@pytest.fixture(scope="module")
def z():
    return golden("matcher_step_128x160")


def build(dev):
    """test_matcher_trainer_gpu.build: the matcher with the stage-2 optimizer and scheduler."""
    model = build_matcher(dev)
    model.optimizer_init = {"class_path": "torch.optim.Adam", "init_args": {"lr": LR, "weight_decay": WD}}
    model.lr_scheduler_init = {"class_path": "torch.optim.lr_scheduler.MultiStepLR",
                               "init_args": {"milestones": [100000, 150000], "gamma": 0.5}}
    return model


def _trainer(dev, precision, graph=False, ckpt_path=None):
    from refign_amd.trainer import Trainer
    torch.manual_seed(0)
    np.random.seed(0)
    model = build(dev)
    return model, Trainer(model, deterministic=True, precision=precision, graph_step=graph, ckpt_path=ckpt_path,
                          scaler_args={"init_scale": FP16_SCALE} if precision == 16 else None)


def _state(model, trainer):
    """Every parameter, every buffer, Adam's moments and step counts, the scaler: name -> CPU tensor / number."""
    out = {"param/" + k: v.detach().cpu().clone() for k, v in model.named_parameters()}
    out.update({"buffer/" + k: v.detach().cpu().clone() for k, v in model.named_buffers()})
    for i, st in trainer.optimizer.state_dict()["state"].items():
        for k, v in st.items():
            out[f"adam/{i}/{k}"] = v.detach().cpu().clone() if torch.is_tensor(v) else v
    if trainer.scaler is not None:
        out.update({"scaler/scale": trainer.scaler._scale.cpu().clone(), "scaler/tracker": trainer.scaler._growth_tracker.cpu().clone(),
                    "scaler/skipped": trainer.scaler._skipped.cpu().clone()})
    out["global_step"] = int(model.global_step)
    return out


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _assert_same_state(a, b, what):
    assert a.keys() == b.keys(), what
    assert any(k.startswith("adam/") and k.endswith("exp_avg_sq") for k in a), "no optimizer state was compared"
    bad = [k for k in a if not (torch.equal(_bits(a[k]), _bits(b[k])) if torch.is_tensor(a[k]) else a[k] == b[k])]
    assert not bad, f"{what}: {len(bad)} of {len(a)} entries differ, first {bad[:5]}"


def _run(dev, z, precision, steps, graph=False):
    model, trainer = _trainer(dev, precision, graph)
    batch, rows = matcher_batch(z, dev), []
    for it in range(steps):
        trainer.step(batch, it)
        rows.append([float(model.logged[k]) for k in LOSSES])
    if graph:
        assert trainer.step_graph.captured()
    state = _state(model, trainer)
    trainer.close()
    assert np.isfinite(rows).all()
    return rows, state


@pytest.fixture(scope="module")
def eager32(dev, z):
    """Five uninterrupted eager deterministic fp32 steps, and the state after the third: computed once, read only."""
    model, trainer = _trainer(dev, 32)
    batch, rows, after3 = matcher_batch(z, dev), [], None
    for it in range(5):
        trainer.step(batch, it)
        rows.append([float(model.logged[k]) for k in LOSSES])
        if it == 2:
            after3 = _state(model, trainer)
    state = _state(model, trainer)
    trainer.close()
    return rows, after3, state


def test_two_fresh_fp32_runs_agree_bit_for_bit(dev, z, eager32):
    rows5, after3, _ = eager32
    rows, state = _run(dev, z, 32, 3)
    assert rows == rows5[:3], (rows, rows5[:3])
    _assert_same_state(state, after3, "two eager fp32 runs of 3 steps")
    assert rows[2] != rows[0], "the steps did not train"


def test_two_fresh_fp16_runs_agree_bit_for_bit(dev, z):
    (rows_a, state_a), (rows_b, state_b) = _run(dev, z, 16, 3), _run(dev, z, 16, 3)
    assert rows_a == rows_b, (rows_a, rows_b)
    _assert_same_state(state_a, state_b, "two eager fp16 runs of 3 steps")
    assert float(state_a["scaler/skipped"]) == 0, "the fp16 steps were skipped: nothing was compared"


@pytest.mark.parametrize("precision", [32, 16])
def test_replayed_runs_repeat_themselves(dev, z, precision):
    """graph_step=True over 5 steps (two eager, the capture, replays): the run equals its own repeat."""
    (rows_a, state_a), (rows_b, state_b) = _run(dev, z, precision, 5, graph=True), _run(dev, z, precision, 5, graph=True)
    assert rows_a == rows_b, (rows_a, rows_b)
    _assert_same_state(state_a, state_b, f"two replayed precision={precision} runs of 5 steps")


def test_resume_equals_the_uninterrupted_run(dev, z, eager32, tmp_path):
    rows5, _, state5 = eager32
    path = str(tmp_path / "three.ckpt")
    model, trainer = _trainer(dev, 32)
    batch = matcher_batch(z, dev)
    for it in range(3):
        trainer.step(batch, it)
    trainer.save_checkpoint(path)
    trainer.close()
    fresh, resumed = _trainer(dev, 32, ckpt_path=path)
    assert fresh.global_step == 3
    rows = []
    for it in range(3, 5):
        resumed.step(batch, it)
        rows.append([float(fresh.logged[k]) for k in LOSSES])
    state = _state(fresh, resumed)
    resumed.close()
    assert rows == rows5[3:], (rows, rows5[3:])
    _assert_same_state(state, state5, "3 steps + save + resume + 2 steps against 5 uninterrupted steps")


def test_first_step_agrees_with_the_reference(dev, z, eager32):
    """The first deterministic step's losses against the golden step, within the bound
    test_matcher_gpu.test_matcher_training_step_matches_reference holds the default-mode step to (2e-4 relative)."""
    total, ss, us = eager32[0][0]
    print(f"deterministic step: ss {ss!r} (golden {float(z['ss_loss'])!r}), us {us!r} (golden {float(z['us_loss'])!r})")
    assert abs(ss - float(z["ss_loss"])) <= 2e-4 * float(z["ss_loss"])
    assert abs(us - float(z["us_loss"])) <= 2e-4 * float(z["us_loss"])
    from refign_amd.trainer import Trainer
    model = build(dev)
    trainer = Trainer(model, precision=32)
    trainer.step(matcher_batch(z, dev), 0)
    default = [float(model.logged[k]) for k in LOSSES]
    trainer.close()
    for got, want in zip((total, ss, us), default):
        assert abs(got - want) <= 2e-4 * abs(want), (got, want)


def test_uda_model_keeps_the_plain_mode(dev):
    """The segmentation model: ValueError for precision=32 as before; a deterministic matcher Trainer holds the flag AND the
    widening, and close() drops both."""
    from test_deterministic_gpu import build as build_uda
    from refign_amd import _lib, determinism
    from refign_amd.trainer import Trainer
    lib = _lib.load_library()
    uda = build_uda(False, dev)
    with pytest.raises(ValueError, match="precision=32"):
        Trainer(uda, deterministic=True, precision=32)
    assert lib.rfn_get_deterministic() == 0 and not determinism.enabled() and not determinism.scatter_forms()
    t = Trainer(uda, deterministic=True, precision="bf16")
    assert determinism.enabled() and not determinism.scatter_forms()
    t.close()
    for precision in (32, 16, "bf16", None):
        t = Trainer(build(dev), deterministic=True, precision=precision)
        assert lib.rfn_get_deterministic() == 1 and determinism.enabled() and determinism.scatter_forms()
        t.close()
        assert lib.rfn_get_deterministic() == 0 and not determinism.enabled() and not determinism.scatter_forms()


def test_widening_follows_blocks_and_holders(dev):
    """The widening is what the innermost block says; outside blocks it is on while a holder that asked for it remains; it never
    reads on while the mode is off; the defaults are the plain mode."""
    from refign_amd import determinism as d
    assert not d.enabled() and not d.scatter_forms()
    with d.deterministic(scatter_forms=True):
        assert d.enabled() and d.scatter_forms()
        with d.deterministic():
            assert d.enabled() and not d.scatter_forms()
        with d.deterministic(False, scatter_forms=True):
            assert not d.enabled() and not d.scatter_forms()
        assert d.scatter_forms()
    d.acquire()
    d.acquire(scatter_forms=True)
    try:
        assert d.enabled() and d.scatter_forms()
        with d.deterministic():
            assert not d.scatter_forms()
        d.release(scatter_forms=True)
        assert d.enabled() and not d.scatter_forms()
    finally:
        d.release()
        d.release()
    assert not d.enabled() and not d.scatter_forms()


def test_default_mode_calls_no_new_entry_point(dev, z, monkeypatch):
    """deterministic=False: one matcher step calls none of the entry points this mode added, and the flag reads 0 throughout."""
    from refign_amd import _lib
    from refign_amd.trainer import Trainer
    lib = _lib.load_library()
    calls, flags = {}, []
    for name in NEW_ENTRY_POINTS:
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    real_bwd, bwd_calls = lib.rfn_warp_bwd_f32, []

    def warp_bwd(*a):
        flags.append(lib.rfn_get_deterministic())
        bwd_calls.append(a[7])
        return real_bwd(*a)
    monkeypatch.setattr(lib, "rfn_warp_bwd_f32", warp_bwd)
    model = build(dev)
    trainer = Trainer(model, precision=16, scaler_args={"init_scale": FP16_SCALE})
    assert not trainer.deterministic
    trainer.step(matcher_batch(z, dev), 0)
    trainer.close()
    assert not calls, calls
    assert bwd_calls and set(flags) == {0}, "the default warp backward did not run"
    assert lib.rfn_get_deterministic() == 0

"""CPU: Trainer(gradient_clip_val=, gradient_clip_algorithm=, accumulate_grad_batches=) outside the device -- the YAML helper,
keyword validation, the declarations of the four entry points, the accumulation schedule of step() / fit() / checkpoints on the
stand-in of test_matcher_graph_cpu (automatic optimization, a real training_step), the accumulated gradient against autograd,
and the CPU clip against torch's two functions."""
import math

import pytest
import torch
import yaml
from test_config_cpu import _REF_CONFIG_NAMES, _REF_CONFIGS
from test_fit_cpu import TRAINER_YAML
from test_matcher_graph_cpu import Tiny, _batch
from test_matcher_trainer_cpu import STAGE2_TRAINER_YAML

NEW_ENTRY_POINTS = ("rfn_grad_clip_coef", "rfn_grad_scale_f32", "rfn_grad_clamp_f32", "rfn_amp_unscale_sqnorm_groups_f32")
DEFAULTS = {"gradient_clip_val": None, "gradient_clip_algorithm": "norm", "accumulate_grad_batches": 1}


class Memory:
    def __init__(self):
        self.rows = []

    def log_metrics(self, metrics, step):
        self.rows.append((step, dict(metrics)))

    def flush(self):
        pass

    def close(self):
        pass


def _micro_batch(j):
    """Batches that differ from call to call: their own seed and their own prime_trg_idx."""
    g = torch.Generator().manual_seed(100 + j)
    b = _batch([j % 2, (j + 1) % 2])
    return {k: (torch.randn(v.shape, generator=g) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b.items()}


def _trainer(seed=0, **kw):
    from refign_amd.trainer import Trainer
    torch.manual_seed(seed)
    return Trainer(Tiny(), **kw)


# ---------------------------------------------------------------------------------------------------------------------
# config.trainer_gradients
# ---------------------------------------------------------------------------------------------------------------------
def test_trainer_gradients_on_yaml_text():
    from refign_amd import config
    assert config.trainer_gradients(yaml.safe_load("trainer:\n  max_steps: 10\n")) == DEFAULTS
    assert config.trainer_gradients({}) == DEFAULTS and config.trainer_gradients(None) == DEFAULTS
    assert config.trainer_gradients(yaml.safe_load(TRAINER_YAML)) == DEFAULTS
    assert config.trainer_gradients(yaml.safe_load(STAGE2_TRAINER_YAML)) == DEFAULTS
    got = config.trainer_gradients(yaml.safe_load(
        "trainer:\n  gradient_clip_val: 0.5\n  gradient_clip_algorithm: value\n  accumulate_grad_batches: 4\n"))
    assert got == {"gradient_clip_val": 0.5, "gradient_clip_algorithm": "value", "accumulate_grad_batches": 4}
    with pytest.raises(ValueError, match="accumulate_grad_batches.*schedule"):
        config.trainer_gradients(yaml.safe_load("trainer:\n  accumulate_grad_batches:\n    0: 1\n    4: 2\n"))
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        config.trainer_gradients(yaml.safe_load("trainer:\n  gradient_clip_algorithm: agc\n"))
    with pytest.raises(ValueError, match="gradient_clip_val"):
        config.trainer_gradients(yaml.safe_load("trainer:\n  gradient_clip_val: -1.0\n"))
    # kept out of trainer_kwargs, whose five keys other tests pin
    cfg = yaml.safe_load("trainer:\n  max_steps: 3\n  gradient_clip_val: 1.0\n  accumulate_grad_batches: 2\n")
    assert set(config.trainer_kwargs(cfg)) == {"max_steps", "val_every_n_steps", "save_last", "sync_batchnorm", "precision"}


@pytest.mark.parametrize("name", _REF_CONFIG_NAMES)
def test_trainer_gradients_on_the_reference_configs(name):
    path = next((p for p in _REF_CONFIGS if p.endswith("/configs/" + name)), None)
    if path is None:
        pytest.skip(f"reference checkout not present (configs/{name})")
    from refign_amd import config
    assert config.trainer_gradients(config.load_config(path)) == DEFAULTS


# ---------------------------------------------------------------------------------------------------------------------
# keywords
# ---------------------------------------------------------------------------------------------------------------------
def test_trainer_keyword_validation():
    from refign_amd.trainer import Trainer
    for bad in (-1.0, float("nan"), "1.0", True, [1.0]):
        with pytest.raises(ValueError, match="gradient_clip_val"):
            Trainer(Tiny(), gradient_clip_val=bad)
    for alg in ("agc", None, "Norm"):
        with pytest.raises(ValueError, match="gradient_clip_algorithm"):
            Trainer(Tiny(), gradient_clip_val=1.0, gradient_clip_algorithm=alg)
    for k in (0, -2, 2.0, True, "2", None, {0: 2}):
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            Trainer(Tiny(), accumulate_grad_batches=k)
    with pytest.raises(ValueError, match="accumulate_grad_batches.*automatic_optimization"):
        Trainer(Tiny(automatic=False), accumulate_grad_batches=2)
    # off, as in Lightning
    for off in (None, 0, 0.0):
        t = Trainer(Tiny(), gradient_clip_val=off)
        assert t._clip is None and t.accumulate_grad_batches == 1 and t.optimizer_stepped is False
        t.close()
    t = Trainer(Tiny(automatic=False), gradient_clip_val=2, gradient_clip_algorithm="value")    # clipping serves both kinds
    assert t._clip.value == 2.0 and t._clip.algorithm == "value"
    t.close()


def test_header_declares_the_four_entry_points():
    import ctypes

    import refign_amd
    from refign_amd import _lib
    lib = ctypes.CDLL(refign_amd.library_path())
    p, i, l_, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    want = {"rfn_grad_clip_coef": [p, i, f, p, p], "rfn_grad_scale_f32": [p, l_, p, p], "rfn_grad_clamp_f32": [p, l_, f, p],
            "rfn_amp_unscale_sqnorm_groups_f32": [p, l_, p, i, i, p, p, p, p, p]}
    assert set(want) == set(NEW_ENTRY_POINTS)
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name] == (i, args), name            # rfn_stream_t (a pointer) last
    with open(_lib._HEADER) as fh:
        text = fh.read()
    for name in want:
        decl = text[text.index(f"int {name}("):]
        assert decl[:decl.index(";")].rstrip().endswith("rfn_stream_t stream)"), name
    assert refign_amd.abi_version() == 5
    # argument errors are decided on the host: nothing is launched
    bound = _lib.load_library()
    assert bound.rfn_grad_clip_coef(None, 1, 1.0, 64, None) == -1
    assert bound.rfn_grad_clip_coef(64, 33, 1.0, 64, None) == -1
    assert bound.rfn_grad_clip_coef(64, 1, -1.0, 64, None) == -1
    assert bound.rfn_grad_clip_coef(64, 1, float("nan"), 64, None) == -1
    assert bound.rfn_grad_scale_f32(68, 4, 64, None) == -1                       # not 16-byte aligned
    assert bound.rfn_grad_scale_f32(64, 0, 64, None) == -1
    assert bound.rfn_grad_clamp_f32(64, 4, -0.5, None) == -1
    assert bound.rfn_grad_clamp_f32(None, 4, 0.5, None) == -1
    assert bound.rfn_amp_unscale_sqnorm_groups_f32(64, 4, 64, 1, 1, None, 64, 64, 64, None) == -1
    assert bound.rfn_amp_unscale_sqnorm_groups_f32(64, 4, 64, 1, 33, 64, 64, 64, 64, None) == -1
    assert bound.rfn_amp_unscale_sqnorm_groups_f32(68, 4, 64, 1, 1, 64, 64, 64, 64, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the accumulation schedule
# ---------------------------------------------------------------------------------------------------------------------
def _counted(trainer):
    seen = {"zero": [], "opt": [], "call": 0}
    real_zero = trainer.grads.zero

    def zero():
        seen["zero"].append(seen["call"])
        real_zero()

    trainer.grads.zero = zero
    trainer.optimizer.register_step_post_hook(lambda *a: seen["opt"].append(seen["call"]))
    return seen


def test_accumulation_schedule_over_seven_calls(tmp_path):
    trainer = _trainer(accumulate_grad_batches=3)
    model, seen = trainer.model, _counted(trainer)
    stepped, gs, sched = [], [], []
    for call in range(1, 8):
        seen["call"] = call
        trainer.step(_micro_batch(call), call - 1)
        stepped.append(trainer.optimizer_stepped)
        gs.append(model.global_step)
        sched.append(trainer.scheduler.last_epoch)
        if call == 4:
            with pytest.raises(RuntimeError, match="accumulation"):
                trainer.save_checkpoint(str(tmp_path / "open.ckpt"))
        if call == 6:
            trainer.save_checkpoint(str(tmp_path / "closed.ckpt"))
    assert seen["zero"] == [1, 4, 7] and seen["opt"] == [3, 6]
    assert stepped == [False, False, True, False, False, True, False]
    assert gs == [0, 0, 1, 1, 1, 2, 2] and sched == gs
    ck = torch.load(str(tmp_path / "closed.ckpt"), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 2
    # the window restarts at load_checkpoint: the call after it zeroes
    trainer.load_checkpoint(str(tmp_path / "closed.ckpt"))
    seen["call"] = 8
    trainer.step(_micro_batch(8), 7)
    assert seen["zero"] == [1, 4, 7, 8] and model.global_step == 2
    trainer.close()


def test_fit_counts_optimizer_steps():
    trainer = _trainer(accumulate_grad_batches=3)
    model = trainer.model
    calls, vals = [], []
    real_step = trainer.step

    def step(batch, batch_idx=0, next_batch=None):
        calls.append((batch_idx, next_batch is None, model.global_step))
        return real_step(batch, batch_idx, next_batch=next_batch)

    trainer.step = step
    trainer.validate = lambda loaders: vals.append(model.global_step) or {}
    out = trainer.fit([_micro_batch(j) for j in range(4)], val_loaders={"": []}, max_steps=2, val_every_n_steps=1)
    assert [c[0] for c in calls] == [0, 1, 2, 3, 4, 5]                 # batch_idx: the calls so far
    assert [c[1] for c in calls] == [False] * 5 + [True]                # the look-ahead is None for the very last call only
    assert [c[2] for c in calls] == [0, 0, 0, 1, 1, 1]
    assert vals == [1, 2] and [s for s, _ in out] == [1, 2] and model.global_step == 2
    trainer.close()


def test_accumulated_gradient_is_the_gradient_of_the_mean_loss():
    """After a window of k = 3 the flat buffer holds d(sum_j loss_j / 3) / d(params), and model.logged the undivided loss of the
    last call.  Tolerance: the two sides add the same three fp32 gradients in another order and divide before or after --
    a handful of roundings of 2^-24 each on values of order 1: rtol 1e-5, atol 1e-6."""
    trainer = _trainer(seed=5, accumulate_grad_batches=3)
    model = trainer.model
    torch.manual_seed(5)
    twin = Tiny()
    assert all(torch.equal(a, b) for a, b in zip(model.parameters(), twin.parameters()))
    batches = [_micro_batch(j) for j in range(3)]
    losses = [twin.training_step(b, j) for j, b in enumerate(batches)]
    want = torch.autograd.grad(sum(losses) / 3, list(twin.parameters()))
    for j, b in enumerate(batches):
        trainer.step(b, j)
    assert model.global_step == 1
    for p, w in zip(model.parameters(), want):
        assert torch.allclose(p.grad, w, rtol=1e-5, atol=1e-6), (p.grad, w)
    assert float(model.logged["train_matching_loss"]) == pytest.approx(float(losses[2].detach()), rel=1e-6)
    single = [float(x) for x in torch.autograd.grad(twin.training_step(batches[0], 0), list(twin.parameters()))[0].flatten()]
    assert not torch.allclose(model.lin.weight.grad.flatten(), torch.tensor(single), rtol=1e-3)     # not one batch's gradient
    trainer.close()


# ---------------------------------------------------------------------------------------------------------------------
# the CPU clip
# ---------------------------------------------------------------------------------------------------------------------
def _fill(trainer, values):
    with torch.no_grad():
        for p, v in zip(trainer.grads.params, values):
            p.grad.copy_(v)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("algorithm", ["norm", "value"])
@pytest.mark.parametrize("case", ["over", "under", "nan"])
def test_cpu_clip_is_torchs_bit_for_bit(algorithm, case):
    g = torch.Generator().manual_seed(9)
    values = [torch.randn(1, 4, generator=g) * 3, torch.randn(1, generator=g) * 3]
    clip = {"over": 0.75, "under": 1e3, "nan": 0.75}[case]
    if case == "nan":
        values[0][0, 2] = float("nan")
    trainer = _trainer(gradient_clip_val=clip, gradient_clip_algorithm=algorithm)
    _fill(trainer, values)
    before = trainer.grads.flat.clone()
    trainer._unscale_and_clip()
    refs = [torch.nn.Parameter(torch.zeros_like(v)) for v in values]
    for r, v in zip(refs, values):
        r.grad = v.clone()
    if algorithm == "norm":
        torch.nn.utils.clip_grad_norm_(refs, clip)
    else:
        torch.nn.utils.clip_grad_value_(refs, clip)
    for p, r in zip(trainer.grads.params, refs):
        assert torch.equal(_bits(p.grad), _bits(r.grad))
    if case == "under":
        assert torch.equal(_bits(trainer.grads.flat), _bits(before))         # untouched
    elif case == "over":
        assert not torch.equal(trainer.grads.flat, before)
    if case == "nan":
        nan = torch.isnan(trainer.grads.flat)
        assert bool(nan.any()) and (algorithm == "norm" or int(nan.sum()) == 1)
    trainer.close()


def test_logged_row_holds_the_norm_before_clipping():
    logger = Memory()
    trainer = _trainer(gradient_clip_val=1e-3, logger=logger, log_every_n_steps=1)
    trainer.step(_micro_batch(0), 0)
    trainer.flush_log()
    (step, row), = logger.rows
    after = float(trainer.grads.flat.double().norm())
    assert step == 0 and row["grad_clip/coef"] < 1.0
    assert row["grad_norm/total"] == pytest.approx(after / row["grad_clip/coef"], rel=1e-5)
    assert after == pytest.approx(1e-3, rel=1e-3)                                 # (eps 1e-6 against a threshold of 1e-3)
    assert math.isfinite(row["train_matching_loss"]) and row["grad_norm/nonfinite_chunks"] == 0.0
    trainer.close()
    # value clipping: the norm before the clamp, and no coefficient
    logger = Memory()
    trainer = _trainer(gradient_clip_val=1e-3, gradient_clip_algorithm="value", logger=logger, log_every_n_steps=1)
    trainer.step(_micro_batch(0), 0)
    trainer.flush_log()
    (_, row2), = logger.rows
    assert "grad_clip/coef" not in row2 and row2["grad_norm/total"] == pytest.approx(row["grad_norm/total"], rel=1e-6)
    assert float(trainer.grads.flat.abs().max()) <= float(torch.tensor(1e-3))     # (the fp32 threshold)
    trainer.close()

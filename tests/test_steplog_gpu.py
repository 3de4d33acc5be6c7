"""GPU: the step log (csrc/steplog.hip, refign_amd/steplog.py) and Trainer(logger=...).

1. rfn_steplog_gather over mixed dtypes is bit-equal to tensor.double(); argument errors launch nothing.
2. rfn_grad_sqnorm_groups against sum(g.double() ** 2) per group.  Tolerance on the norm: 2e-8 relative, derived: the terms
   are non-negative, so either fp64 sum of n terms is within (n - 1) * 2^-53 of the exact one in any order, n < 1e8 here
   (1e8 * 2^-53 = 1.1e-8 on the sum of squares for each of the two sums), and the square root halves the relative error.
3. One Trainer.step with a row per step, every precision, graphs on and off: losses bit-equal, norms to 2e-8, amp values equal.
4. Parity with the reference's golden step through Trainer.step with a logger, at the golden test's own tolerances.
5. No waiting, 6. logging does not touch the run, 7. logger=None calls neither entry point, 8. rows under graph replay carry
   their own step's losses, 9. a resumed run continues the labels in a second event file with bit-equal rows."""
import ctypes
import math
import random

import numpy as np
import pytest
import torch
from conftest import golden
from test_deterministic_gpu import _assert_same_trajectory, _bit_equal, _run
from test_resume_gpu import _model, _seed, _steps
from test_step_gpu import build, make_batch
from test_steplog_cpu import _event_files, _rows_of

pytestmark = pytest.mark.gpu
LOSSES = ("train_loss_src", "train_loss_featdist_src", "train_loss_uda_trg")
GROUPS = ["head_weight", "head_bias", "backbone_weight", "backbone_bias"]
NORM_RTOL = 2e-8


class Memory:
    """A logger that keeps what it is handed."""

    def __init__(self):
        self.rows, self.closed = [], False

    def log_metrics(self, metrics, step):
        self.rows.append((step, dict(metrics)))

    def flush(self):
        pass

    def close(self):
        self.closed = True


def _same_rows(a, b):
    return len(a) == len(b) and all(
        sa == sb and list(ra) == list(rb) and all(ra[k] == rb[k] or (math.isnan(ra[k]) and math.isnan(rb[k])) for k in ra)
        for (sa, ra), (sb, rb) in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# 1. gather
# ---------------------------------------------------------------------------------------------------------------------
def test_gather_is_bit_equal_to_double(dev):
    from refign_amd import _lib
    from refign_amd.steplog import gather_scalars
    inf, nan = float("inf"), float("nan")
    f32 = torch.tensor([1.0, -0.0, 3.4028234e38, 1.1754944e-38, inf, -inf, nan, 2.944438934326172, 1 / 3, -7e-30], device=dev)
    bf16 = torch.tensor([1.0, 0.33203125, -3.38e38, inf, nan, 1.18e-38, 65536.0, -2.5], device=dev, dtype=torch.bfloat16)
    f16 = torch.tensor([1.0, 65504.0, -6.104e-5, inf, -inf, nan, 0.333251953125, 2048.0], device=dev, dtype=torch.float16)
    f64 = torch.tensor([1 / 3, 1e300, -1e-300, inf, nan, 2.3e-308], device=dev, dtype=torch.float64)
    i32 = torch.tensor([0, 1, -1, 2 ** 31 - 1, -2 ** 31, 2000], device=dev, dtype=torch.int32)
    tensors = []
    for base in (f32, bf16, f16, f64, i32):
        tensors += [base[i] for i in range(base.numel())]              # 0-dim views, 16-bit ones at odd element offsets too
    tensors.append(torch.tensor([0.75], device=dev).reshape(1, 1))       # one element, not 0-dim
    random.Random(4).shuffle(tensors)                                    # dtypes interleaved
    assert len(tensors) > 32                                             # more than one launch
    row = torch.full((len(tensors) + 3,), -123.0, dtype=torch.float64, device=dev)
    gather_scalars(tensors, row)
    want = torch.stack([t.reshape(()).double() for t in tensors])
    assert _bit_equal(row[:len(tensors)], want)
    assert bool((row[len(tensors):] == -123.0).all())                    # nothing written behind the values
    # argument errors: RFN_EINVAL, and nothing is launched (the row keeps its contents)
    lib = _lib.load_library()
    st = torch.cuda.current_stream(dev).cuda_stream
    ok_p, ok_c = (ctypes.c_void_p * 2)(f32.data_ptr(), bf16.data_ptr()), (ctypes.c_int * 2)(0, 1)
    many_p, many_c = (ctypes.c_void_p * 33)(*[f32.data_ptr()] * 33), (ctypes.c_int * 33)(*[0] * 33)
    row.fill_(-5.0)
    cases = {"n = 0": (ok_p, ok_c, 0, row.data_ptr()), "n = 33": (many_p, many_c, 33, row.data_ptr()),
             "n < 0": (ok_p, ok_c, -1, row.data_ptr()), "row NULL": (ok_p, ok_c, 2, None),
             "table NULL": (None, ok_c, 2, row.data_ptr()), "codes NULL": (ok_p, None, 2, row.data_ptr()),
             "null value": ((ctypes.c_void_p * 2)(f32.data_ptr(), None), ok_c, 2, row.data_ptr()),
             "code 5": (ok_p, (ctypes.c_int * 2)(0, 5), 2, row.data_ptr()),
             "code -1": (ok_p, (ctypes.c_int * 2)(-1, 1), 2, row.data_ptr()),
             "misaligned f32": ((ctypes.c_void_p * 2)(f32.data_ptr() + 2, bf16.data_ptr()), ok_c, 2, row.data_ptr()),
             "misaligned row": (ok_p, ok_c, 2, row.data_ptr() + 4)}
    for what, (p, c, n, r) in cases.items():
        assert lib.rfn_steplog_gather(p, c, n, r, st) == -1, what
        with pytest.raises(RuntimeError, match="steplog_gather"):
            _lib.check(-1, "steplog_gather")
    torch.cuda.synchronize(dev)
    assert bool((row == -5.0).all())
    with pytest.raises(TypeError):
        gather_scalars([torch.zeros(2, device=dev)], row)
    with pytest.raises(TypeError):
        gather_scalars([torch.zeros((), device=dev, dtype=torch.int64)], row)
    with pytest.raises(TypeError):
        gather_scalars([torch.zeros(())], row)                           # a CPU value into a device row


# ---------------------------------------------------------------------------------------------------------------------
# 2. norms per group
# ---------------------------------------------------------------------------------------------------------------------
def _wide(n, seed, dev):
    """fp32 values with magnitudes spread over 1e-20 .. 1e18, mixed signs"""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 38.0 - 20.0)
    return (mag * torch.randn(n, generator=g, dtype=torch.float64).sign()).float().to(dev)


def _reference_sq(flat, runs, G):
    out = [torch.zeros((), dtype=torch.float64, device=flat.device) for _ in range(G)]
    for off, n, gi in runs:
        out[gi] = out[gi] + (flat[off:off + n].double() ** 2).sum()
    return [float(v) for v in out]


@pytest.mark.parametrize("chunk", [32768, 1000])
def test_grad_sqnorm_groups_against_fp64_torch(dev, chunk):
    from refign_amd.steplog import GradNormPlan, grad_sqnorm_groups
    # runs of length 1 (at offsets of every alignment), runs that are no multiple of the chunk, group 3 without a parameter
    lens = [1, 1, 1, 1, 2, 3, 5, 64, 2 * 32768 + 17, 100001, 7, 32768, 31, 4_000_003, 1, 999, 12_345_677]
    groups = [0, 1, 0, 2, 4, 1, 0, 2, 1, 4, 4, 0, 2, 1, 0, 4, 2]
    runs, off = [], 0
    for n, gi in zip(lens, groups):
        runs.append((off, n, gi))
        off += n + (3 if n == 5 else 0)                                   # (a gap that belongs to no run is not summed)
    total = off + 11
    assert total < 1e8
    G = 5
    flat = _wide(total, 7, dev)
    plan = GradNormPlan(runs, G, total, dev, chunk=chunk)
    assert all(n <= chunk for _, n, _ in plan.chunks) and sum(n for _, n, _ in plan.chunks) == sum(lens)
    out = torch.full((G + 1,), -1.0, dtype=torch.float64, device=dev)
    grad_sqnorm_groups(flat, plan, out)
    again = torch.full((G + 1,), -2.0, dtype=torch.float64, device=dev)
    grad_sqnorm_groups(flat, plan, again)
    assert _bit_equal(out, again), "two launches differ"
    got, want = out.tolist(), _reference_sq(flat, runs, G)
    assert got[G] == 0.0 and got[3] == 0.0 and want[3] == 0.0
    for gi in range(G):
        a, b = got[gi] ** 0.5, want[gi] ** 0.5
        print(f"chunk {chunk} group {gi}: norm {a:.17g} reference {b:.17g} relative {abs(a - b) / max(b, 1e-300):.2e}")
        assert abs(a - b) <= NORM_RTOL * b
    # an infinity and a NaN: their groups say so, the others keep their bits, the count is the number of chunks hit
    bad = flat.clone()
    bad[runs[8][0] + 40000] = float("inf")                               # group 1
    bad[runs[16][0] + 5] = float("nan")                                  # group 2
    out2 = torch.zeros(G + 1, dtype=torch.float64, device=dev)
    grad_sqnorm_groups(bad, plan, out2)
    got2 = out2.tolist()
    assert got2[1] == float("inf") and math.isnan(got2[2]) and got2[G] == 2.0
    assert got2[0] == got[0] and got2[4] == got[4] and got2[3] == 0.0
    # a damaged table cannot make the kernel read outside the buffer: such a chunk is not read and counts as non-finite
    table = plan.table.clone()
    plan.table[0, 0] = total                                              # offset + length beyond the end
    plan.table[1, 2] = G                                                  # a group that does not exist
    plan.table[2, 1] = -4                                                 # a negative length
    out3 = torch.zeros(G + 1, dtype=torch.float64, device=dev)
    grad_sqnorm_groups(flat, plan, out3)
    assert out3.tolist()[G] == 3.0
    plan.table.copy_(table)
    with pytest.raises(ValueError):
        GradNormPlan([(0, total + 1, 0)], 1, total, dev)
    with pytest.raises(RuntimeError):
        grad_sqnorm_groups(flat[1:], plan, out)
    with pytest.raises(RuntimeError):
        grad_sqnorm_groups(flat, plan, out[:G])


def test_grad_sqnorm_of_a_trainers_buffer_layout(dev):
    """The table built from FlatGradBuffer._order and the optimizer's groups covers every parameter once: the norms of a random
    fill through the views equal the per-group norms of the .grad tensors."""
    from refign_amd.steplog import GradNormPlan, grad_sqnorm_groups
    from refign_amd.trainer import Trainer
    trainer = Trainer(build(False, dev), fused_optimizer=False)
    g = torch.Generator(device=dev).manual_seed(3)
    for p in trainer.grads.params:
        p.grad.copy_(torch.randn(p.shape, generator=g, device=dev))
    plan = GradNormPlan.for_buffer(trainer.grads, trainer.optimizer.param_groups)
    out = torch.zeros(5, dtype=torch.float64, device=dev)
    grad_sqnorm_groups(trainer.grads.flat, plan, out)
    want = [float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in grp["params"]))) for grp in trainer.optimizer.param_groups]
    assert [grp["name"] for grp in trainer.optimizer.param_groups] == GROUPS
    for a, b in zip(out.tolist()[:4], want):
        assert abs(a ** 0.5 - b) <= NORM_RTOL * b
    assert out.tolist()[4] == 0.0
    trainer.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. one step, every precision
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", ["1", "0"])
@pytest.mark.parametrize("precision", [None, "bf16", 16, 32])
def test_one_step_row_equals_the_steps_own_values(dev, monkeypatch, precision, graphs):
    from refign_amd.trainer import Trainer
    monkeypatch.setenv("RFN_GRAPH_STUDENT", graphs)
    monkeypatch.setenv("RFN_HIP_GRAPH", graphs)
    model = build(False, dev)
    mem = Memory()
    trainer = Trainer(model, fused_optimizer=False, precision=precision, logger=mem, log_every_n_steps=1,
                      scaler_args={"init_scale": 2.0 ** 10} if precision == 16 else None)
    batch = make_batch(2, 96, 128, 32, dev)
    _seed(77)
    seen = {}
    real_step = trainer.optimizer.step

    def recording_step(*a, **k):
        seen["norms"] = [float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in grp["params"])))
                         for grp in trainer.optimizer.param_groups]
        seen["lr"] = [float(grp["lr"]) for grp in trainer.optimizer.param_groups]
        if trainer.scaler is not None:
            seen["amp"] = {"amp/scale": float(trainer.scaler._scale), "amp/found_inf": float(trainer.scaler.found_inf),
                           "amp/skipped_steps": float(trainer.scaler._skipped)}
        return real_step(*a, **k)

    trainer.optimizer.step = recording_step
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision is None):
        assert trainer.step(batch, 0) is None
    assert trainer.flush_log() == 0
    assert "norms" in seen, "the optimizer did not step (a skipped fp16 step?)"
    assert [s for s, _ in trainer.log_history] == [0] and _same_rows(trainer.log_history, mem.rows)
    row = trainer.log_history[0][1]
    names = set(LOSSES) | {f"grad_norm/{g}" for g in GROUPS} | {"grad_norm/total", "grad_norm/nonfinite_chunks"} | \
        {f"lr-AdamW/{g}" for g in GROUPS} | ({"amp/scale", "amp/found_inf", "amp/skipped_steps"} if precision == 16 else set())
    assert set(row) == names
    for k in LOSSES:
        want = float(model.logged[k].double())
        print(f"precision {precision} graphs {graphs}: {k} logged {row[k]!r} step's own {want!r} ({model.logged[k].dtype})")
        assert row[k] == want and math.isfinite(want)
    for g, want in zip(GROUPS, seen["norms"]):
        got = row[f"grad_norm/{g}"]
        print(f"    grad_norm/{g}: {got:.17g} torch fp64 {want:.17g} relative {abs(got - want) / want:.2e}")
        assert abs(got - want) <= NORM_RTOL * want
    tot = math.sqrt(sum(v * v for v in seen["norms"]))
    assert abs(row["grad_norm/total"] - tot) <= NORM_RTOL * tot and row["grad_norm/nonfinite_chunks"] == 0.0
    assert [row[f"lr-AdamW/{g}"] for g in GROUPS] == seen["lr"]
    if precision == 16:
        assert {k: row[k] for k in seen["amp"]} == seen["amp"] and row["amp/scale"] == 1024.0 and row["amp/found_inf"] == 0.0
    trainer.close()
    assert mem.closed


# ---------------------------------------------------------------------------------------------------------------------
# 4. the reference's golden step through Trainer.step with a logger
# ---------------------------------------------------------------------------------------------------------------------
def test_logged_golden_step_matches_reference(dev):
    """tests/golden/step_daformer_96x128.npz set up as test_step_gpu.test_training_step_matches_reference sets it up, driven
    through Trainer.step: logged losses within that test's rtol=2e-3 of the reference's, logged group norms within its
    rtol=2e-2."""
    from refign_amd.trainer import Trainer
    g = golden("step_daformer_96x128")
    H, W = [int(v) for v in g["size"]]
    model = build(False, dev)
    trainer = Trainer(model, fused_optimizer=False, logger=Memory(), log_every_n_steps=1)
    trainer.scheduler = torch.optim.lr_scheduler.LambdaLR(trainer.optimizer, lambda s: 1.0)   # as in the golden run
    model._scheduler = trainer.scheduler
    batch = make_batch(2, H, W, 32, dev)
    random.seed(77); np.random.seed(77); torch.manual_seed(77)
    model.global_step = 3
    trainer.step(batch, 0)
    trainer.flush_log()
    (label, row), = trainer.log_history
    assert label == 3 and model.global_step == 4
    losses = np.array([row[k] for k in LOSSES])
    norms = np.array([row[f"grad_norm/{k}"] for k in GROUPS])
    print(f"\nlogged losses {losses} reference {g['losses']}\nlogged norms {norms} reference {g['grad_norms']}")
    np.testing.assert_allclose(losses, g["losses"], rtol=2e-3)
    np.testing.assert_allclose(norms, g["grad_norms"], rtol=2e-2)
    trainer.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. no waiting
# ---------------------------------------------------------------------------------------------------------------------
def test_recording_never_waits_for_the_device(dev, monkeypatch):
    from refign_amd.steplog import StepLog
    from refign_amd.trainer import Trainer
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    trainer = Trainer(build(True, dev), precision="bf16", logger=Memory(), log_every_n_steps=1)
    _seed(9)
    for it in range(6):                                                  # warm-up: the ring, the table, the library -- and the
        trainer.step(make_batch(2, 128, 128, 64, dev), it)               # student graphs' captures with their stream probes
    torch.cuda.synchronize(dev)
    n0 = len(trainer.log_history) + trainer._steplog.pending
    torch.cuda.set_sync_debug_mode("error")
    try:
        trainer._record_row()                                            # gather + norms + copy + event, on the current stream
        rows = trainer._steplog.poll()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    trainer._hand_over(rows)
    # a whole step cannot run under the detector (training_step itself calls torch.unique): count the waits instead
    waits = {"flush": 0, "event": 0}
    real_flush, real_sync = StepLog.flush, torch.cuda.Event.synchronize

    def flush(self):
        waits["flush"] += 1
        return real_flush(self)

    def synchronize(self):
        waits["event"] += 1
        return real_sync(self)

    monkeypatch.setattr(StepLog, "flush", flush)
    monkeypatch.setattr(torch.cuda.Event, "synchronize", synchronize)
    for it in range(6, 11):
        trainer.step(make_batch(2, 128, 128, 64, dev), it)
    assert waits == {"flush": 0, "event": 0}, waits
    monkeypatch.setattr(StepLog, "flush", real_flush)
    monkeypatch.setattr(torch.cuda.Event, "synchronize", real_sync)
    assert trainer.flush_log() == 0                                      # no stall
    assert len(trainer.log_history) == n0 + 1 + 5
    assert [s for s, _ in trainer.log_history] == [0, 1, 2, 3, 4, 5, 6, 6, 7, 8, 9, 10]   # (the row recorded by hand: label 6 too)
    trainer.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. logging does not touch the run
# ---------------------------------------------------------------------------------------------------------------------
def _logged_trainer(dev, precision, deterministic, logger, watch=None):
    from refign_amd.trainer import Trainer
    _seed(5)
    trainer = Trainer(build(True, dev, enable_fdist=True), precision=precision, deterministic=deterministic, logger=logger,
                      log_every_n_steps=1)
    if watch is not None:                                                # everything the hook could touch, before and after it
        real = trainer._record_row

        def record_row():
            def snap():
                torch.cuda.synchronize(dev)
                out = {"grads": trainer.grads.flat.clone()}
                out.update({"model/" + k: v.clone() for k, v in trainer.model.state_dict().items()})
                for i, s in trainer.optimizer.state.items():
                    out.update({f"adam/{id(i)}/{k}": v.clone() for k, v in s.items() if torch.is_tensor(v)})
                if trainer.scaler is not None:
                    sc = trainer.scaler
                    out.update(scale=sc._scale.clone(), tracker=sc._growth_tracker.clone(), found=sc.found_inf.clone(),
                               skipped=sc._skipped.clone())
                return out
            before = snap()
            real()
            after = snap()
            watch.append([k for k in before if not _bit_equal(before[k], after[k])])
        trainer._record_row = record_row
    return trainer


@pytest.mark.parametrize("precision", ["bf16", 16])
def test_logging_leaves_a_deterministic_run_bit_equal(dev, monkeypatch, precision):
    """Five steps with a row per step and five without, under deterministic=True (which must not refuse the recording): every
    loss, parameter, EMA parameter, buffer, Adam moment and the scaler state bit-equal after every step.  Graphs on."""
    monkeypatch.setenv("RFN_HIP_GRAPH", "1")
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    mem = Memory()
    ta, a = _run(dev, True, precision, n=5, trainer=_logged_trainer(dev, precision, True, mem))
    assert ta.flush_log() == 0
    ta.close()
    tb, b = _run(dev, True, precision, n=5, trainer=_logged_trainer(dev, precision, True, None))
    tb.close()
    _assert_same_trajectory(a, b, f"deterministic {precision}: with a logger against without")
    assert [s for s, _ in mem.rows] == [0, 1, 2, 3, 4]
    for i, (_, row) in enumerate(mem.rows):                              # and the rows are the run's own losses
        assert all(row[k] == float(a[i]["loss/" + k]) for k in LOSSES)


@pytest.mark.parametrize("precision", ["bf16", 16])
def test_logging_leaves_a_default_mode_run_alone(dev, monkeypatch, precision):
    """The same in the default mode, graphs on.  Two default-mode runs of one configuration are not bit-reproducible here (weight
    gradients and the attention backward add with float atomics: test_resume_gpu's docstring has the figures), so a run with a
    logger is compared with a run without AND two runs without are compared with each other: the logged run must equal the
    plain one bit for bit unless the two plain runs already differ from each other.  What holds in either case and is asserted
    on every step: across the recording hook itself no gradient, parameter, buffer, Adam moment or scaler tensor changes a bit."""
    monkeypatch.setenv("RFN_HIP_GRAPH", "1")
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    touched = []
    ta, a = _run(dev, True, precision, n=5, deterministic=False, trainer=_logged_trainer(dev, precision, False, Memory(), touched))
    ta.close()
    assert len(touched) == 5 and not any(touched), touched
    tb, b = _run(dev, True, precision, n=5, deterministic=False, trainer=_logged_trainer(dev, precision, False, None))
    tb.close()
    tc, c = _run(dev, True, precision, n=5, deterministic=False, trainer=_logged_trainer(dev, precision, False, None))
    tc.close()
    differ = lambda x, y: sum(1 for sx, sy in zip(x, y) for k in sx if not _bit_equal(sx[k], sy[k]))  # noqa: E731
    ab, bc = differ(a, b), differ(b, c)
    print(f"\ndefault mode {precision}: tensors differing over 5 steps: logged vs plain {ab}, plain vs plain {bc}")
    assert ab == 0 or bc > 0, "two plain runs agree bit for bit, the logged run does not"


# ---------------------------------------------------------------------------------------------------------------------
# 7. logger=None
# ---------------------------------------------------------------------------------------------------------------------
def test_without_a_logger_neither_entry_point_is_called(dev, monkeypatch):
    from refign_amd import _lib
    from refign_amd.trainer import Trainer
    lib = _lib.load_library()
    calls = {}
    for name in ("rfn_steplog_gather", "rfn_grad_sqnorm_groups"):
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    _seed(5)
    t = Trainer(build(True, dev), precision="bf16", log_every_n_steps=1)
    for it in range(2):
        assert t.step(make_batch(2, 128, 128, 64, dev), it) is None
    torch.cuda.synchronize(dev)
    assert calls == {} and t._steplog is None and t._norm_plan is None and t.log_history == []
    t.close()
    # (and the wrappers do see a call when there is a logger)
    t = Trainer(build(False, dev), precision="bf16", logger=Memory(), log_every_n_steps=2)
    for it in range(2):
        t.step(make_batch(2, 96, 128, 32, dev), it)
    t.close()
    assert calls == {"rfn_steplog_gather": 1, "rfn_grad_sqnorm_groups": 1}
    assert [s for s, _ in t.log_history] == [1]


# ---------------------------------------------------------------------------------------------------------------------
# 8. graph replay
# ---------------------------------------------------------------------------------------------------------------------
def test_rows_under_graph_replay_carry_their_own_steps_losses(dev, monkeypatch):
    """Graphed student passes (captured at step 3), a row per step: the rows of steps 3, 4, 5 hold the losses RFN_LOG_LOSSES=1
    reads right after each of those steps -- the replayed graph's static outputs are read before the next replay overwrites
    them."""
    from refign_amd.trainer import Trainer
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    monkeypatch.setenv("RFN_HIP_GRAPH", "1")
    monkeypatch.setenv("RFN_LOG_LOSSES", "1")
    model = build(True, dev)
    trainer = Trainer(model, precision="bf16", logger=Memory(), log_every_n_steps=1)
    _seed(5)
    direct = []
    for it in range(6):
        batch = make_batch(2, 128, 128, 64, dev)
        batch["image_src"] = batch["image_src"] + 0.1 * it
        direct.append(trainer.step(batch, it))
    trainer.flush_log()
    for name in ("source_pass", "mixed_pass"):
        st = list(model._graphs[name].states.values())
        assert len(st) == 1 and st[0]["graph"] is not None and not st[0]["failed"], f"{name}: not captured"
    assert [s for s, _ in trainer.log_history] == list(range(6))
    for it in (3, 4, 5):
        row = trainer.log_history[it][1]
        print(f"step {it}: logged {[row[k] for k in LOSSES]} read after the step {[direct[it][k] for k in LOSSES]}")
        assert all(row[k] == direct[it][k] for k in LOSSES)
    assert len({trainer.log_history[it][1]["train_loss_src"] for it in (3, 4, 5)}) == 3, "the losses never changed"
    trainer.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. resume
# ---------------------------------------------------------------------------------------------------------------------
def test_resumed_run_continues_the_labels_in_a_second_file(dev, tmp_path, monkeypatch):
    """Deterministic mode, so that equal is exact: save after step 4 with a logger, resume with a new logger on the same
    directory, step to 8: labels 0..7 across the two event files, rows 4..7 bit-equal to an uninterrupted run's."""
    from refign_amd.steplog import TensorBoardLogger
    from refign_amd.trainer import Trainer
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    _seed(5)
    u = Trainer(_model(dev), precision="bf16", deterministic=True, logger=Memory(), log_every_n_steps=1)
    _steps(dev, u, range(8))
    u.flush_log()
    full = list(u.log_history)
    u.close()
    _seed(5)
    la = TensorBoardLogger(str(tmp_path / "logs"), name="run")
    a = Trainer(_model(dev), precision="bf16", deterministic=True, logger=la, log_every_n_steps=1)
    _steps(dev, a, range(4))
    path = str(tmp_path / "last.ckpt")
    a.flush_log()
    a.save_checkpoint(path)
    first = list(a.log_history)
    a.close()
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "global_step", "pytorch-lightning_version", "state_dict", "loops", "callbacks",
                       "optimizer_states", "lr_schedulers", "refign_amd"} and ck["callbacks"] == {}
    lb = TensorBoardLogger(str(tmp_path / "logs"), name="run", version=0)
    b = Trainer(_model(dev), precision="bf16", deterministic=True, ckpt_path=path, logger=lb, log_every_n_steps=1)
    _steps(dev, b, range(4, 8))
    b.flush_log()
    rest = list(b.log_history)
    b.close()
    assert [s for s, _ in full] == list(range(8))
    assert _same_rows(first, full[:4]), "before the save"
    assert _same_rows(rest, full[4:]), "resumed"
    files = _event_files(la.log_dir)
    assert len(files) == 2 and set(files) == {la.path, lb.path}
    on_disk = _rows_of(la.path) + _rows_of(lb.path)
    assert [s for s, _ in on_disk] == list(range(8))
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).float().item()  # noqa: E731
    for (_, got), (_, want) in zip(on_disk, full):
        assert list(got) == list(want) and all(got[k] == f32(want[k]) for k in want)

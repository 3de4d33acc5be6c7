"""GPU: the matcher's training step replayed from a hipGraph -- Trainer(model, graph_step=True): replays against the eager
trainer, inputs read on every replay, no host entry point and no synchronisation during a replay, fp16 overflow, logged rows,
invalidation, the switches, and the two backward kernels that used to zero with memsets inside a capture.

Yardstick wherever eager and replay are compared (the backward passes add with float atomics): s = the spread between two
eager Trainer runs of the same scenario, per step and quantity; the bound is max(4 s, 1e-4 relative).  A tensor-valued
quantity (a BatchNorm layer's running_mean) is measured in the maximum norm, relative to its largest entry.  The measured
spreads and differences are printed (profiles/matcher_graph_bench.txt keeps a copy).  For the losses the 1e-4 term is the bound
in force (s stays below 3e-6 relative over seven steps); for two of the eleven gradient norms of step 5 and for some running
means the run-to-run noise is above 1e-4 relative, so there the bound in force is 4 s, with s from one pair of runs."""
import warnings

import numpy as np
import pytest
import torch
from conftest import golden
from test_matcher_gpu import _grid_sample_warp, build_matcher, matcher_batch

pytestmark = pytest.mark.gpu

LR, WD = 5e-5, 4e-4
LOSSES = ("train_matching_loss", "train_ss_loss", "train_us_loss")
FP16_SCALE = 2.0 ** 4                  # as in test_matcher_trainer_gpu.py: this batch's fp16 backward does not overflow at it


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


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


def _gradnorms(model):
    out = []
    for _, mod in model.alignment_head.named_children():
        g = [p.grad for p in mod.parameters() if p.requires_grad]
        if g:
            out.append(float(torch.sqrt(sum((x.double() ** 2).sum() for x in g))))
    return np.asarray(out)


def _batchnorms(model):
    return [m for m in model.alignment_head.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


def _bound(a, b):
    """max(4 s, 1e-4 relative) from two eager runs a, b of one scenario."""
    return np.maximum(4 * np.abs(a - b), 1e-4 * np.abs(a))


def _check(name, got, a, b):
    got, a, b = np.asarray(got), np.asarray(a), np.asarray(b)
    bound = _bound(a, b)
    print(f"\n{name}: eager\n{a}\nspread between two eager runs\n{np.abs(a - b)}\n|graph - eager|\n{np.abs(got - a)}\nbound\n{bound}")
    assert np.isfinite(got).all(), name
    assert (np.abs(got - a) <= bound).all(), name


def _batches(z, dev):
    """A: the fixture's batch; B: image_ref / image_trg exchanged and prime_trg_idx flipped; C: B with flow_prime * 0.5."""
    A = matcher_batch(z, dev)
    B = dict(A, image_ref=A["image_trg"], image_trg=A["image_ref"], prime_trg_idx=[1 - v for v in A["prime_trg_idx"]])
    C = dict(B, flow_prime=B["flow_prime"] * 0.5)
    return A, B, C


def _run(dev, seq, graph, precision=None, idx_tensor=False):
    """One Trainer over the batches of `seq` -> (losses per step, captured() after every step, model, trainer)."""
    from refign_amd.trainer import Trainer
    model = build(dev)
    trainer = Trainer(model, graph_step=graph, precision=precision,
                      scaler_args={"init_scale": FP16_SCALE} if precision else None)
    rows, captured = [], []
    for it, batch in enumerate(seq):
        if idx_tensor:
            batch = dict(batch, prime_trg_idx=torch.tensor(batch["prime_trg_idx"], device=dev))
        trainer.step(batch, it)
        rows.append(_logged(model))
        captured.append(trainer.step_graph.captured() if trainer.step_graph is not None else None)
    return np.asarray(rows), captured, model, trainer


@pytest.fixture(scope="module")
def eager5(dev, z):
    """Two eager Trainer runs of five steps on the fixture's batch: losses per step, the last step's gradient norms per
    sub-module, every head BatchNorm's running_mean and num_batches_tracked.  Computed once, read only."""
    runs = []
    for _ in range(2):
        rows, _, model, trainer = _run(dev, [matcher_batch(z, dev)] * 5, False)
        runs.append({"losses": rows, "gradnorms": _gradnorms(model),
                     "mean": [m.running_mean.detach().cpu().numpy().copy() for m in _batchnorms(model)],
                     "tracked": [int(m.num_batches_tracked) for m in _batchnorms(model)]})
        trainer.close()
    return runs


def _compare_to_eager5(model, rows, eager5):
    a, b = eager5
    _check("losses", rows, a["losses"], b["losses"])
    _check("gradient norms of the last step", _gradnorms(model), a["gradnorms"], b["gradnorms"])
    bns = _batchnorms(model)
    assert len(bns) == len(a["mean"]) > 0
    worst = 0.0
    for m, ma, mb in zip(bns, a["mean"], b["mean"]):
        got = m.running_mean.detach().cpu().numpy()
        scale = np.abs(ma).max()
        bound = max(4 * np.abs(ma - mb).max(), 1e-4 * scale)
        worst = max(worst, np.abs(got - ma).max() / max(scale, 1e-30))
        assert np.abs(got - ma).max() <= bound, (np.abs(got - ma).max(), bound)
    print(f"running_mean: largest |graph - eager| relative to the layer's largest entry {worst:.3e} over {len(bns)} layers")
    assert [int(m.num_batches_tracked) for m in bns] == a["tracked"] == b["tracked"]


def test_five_steps_replay_and_follow_the_eager_trainer(dev, z, eager5):
    """Steps 1, 2 eager, 3 captured and replayed, 4 and 5 the second and third replay (where a memset node's symptom showed):
    losses of every step, gradient norms of the last, BatchNorm running statistics within the bound of the eager trainer's;
    no warning on the way."""
    from refign_amd.graphs import GraphedStep
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rows, captured, model, trainer = _run(dev, [matcher_batch(z, dev)] * 5, True)
    assert isinstance(trainer.step_graph, GraphedStep)
    assert captured == [False, False, True, True, True]
    assert model.global_step == 5
    assert all(torch.is_tensor(model.logged[k]) for k in LOSSES)
    _compare_to_eager5(model, rows, eager5)
    trainer.close()
    assert not trainer.step_graph.captured()


@pytest.mark.parametrize("idx_tensor", [False, True], ids=["host_list", "device_tensor"])
def test_inputs_are_read_on_every_replay(dev, z, idx_tensor):
    """Batches A A B C B (captured on B, replayed on C and B), prime_trg_idx as a host list and as a device tensor: the losses
    follow the eager trainer's on the same sequence and move from batch to batch by far more than the bound."""
    A, B, C = _batches(z, dev)
    seq = [A, A, B, C, B]
    key = "sequence"
    if key not in _EAGER:
        _EAGER[key] = [_run(dev, seq, False)[0] for _ in range(2)]
    a, b = _EAGER[key]
    rows, captured, _, trainer = _run(dev, seq, True, idx_tensor=idx_tensor)
    assert captured == [False, False, True, True, True]
    _check("losses over A A B C B", rows, a, b)
    bound = _bound(a, b)
    for it in (2, 3, 4):                                   # every change of batch, train_ss_loss (it reads flow_prime directly)
        moved = abs(rows[it, 1] - rows[it - 1, 1])
        print(f"step {it + 1}: train_ss_loss moved by {moved:.4g}, bound {bound[it, 1]:.4g}")
        assert moved > 20 * bound[it, 1]
    trainer.close()


_EAGER = {}


@pytest.mark.parametrize("precision", [None, 16])
def test_a_replay_enters_no_kernel_entry_point_and_does_not_synchronise(dev, z, precision, monkeypatch):
    from refign_amd import _lib
    from refign_amd.trainer import Trainer
    lib = _lib.load_library()
    calls = {}
    for name in ("rfn_flowloss_fwd_f32", "rfn_warp_bwd_f32"):
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    model = build(dev)
    trainer = Trainer(model, graph_step=True, precision=precision,
                      scaler_args={"init_scale": FP16_SCALE} if precision else None)
    batch = matcher_batch(z, dev)
    batch["prime_trg_idx"] = torch.tensor(batch["prime_trg_idx"], device=dev)
    trainer.step(batch, 0)
    assert calls.get("rfn_flowloss_fwd_f32", 0) > 0 and calls.get("rfn_warp_bwd_f32", 0) > 0
    trainer.step(batch, 1)
    trainer.step(batch, 2)
    assert trainer.step_graph.captured()
    torch.cuda.synchronize(dev)
    before = {k: v.detach().clone() for k, v in model.alignment_head.named_parameters()}
    calls.clear()
    torch.cuda.set_sync_debug_mode("error")
    try:
        trainer.step(batch, 3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == {}, calls
    assert model.global_step == 4 and trainer.step_graph.captured()
    assert any(not torch.equal(v, before[k]) for k, v in model.alignment_head.named_parameters())
    assert all(np.isfinite(v) for v in _logged(model))
    trainer.close()


def _optimizer_state(trainer):
    sd = trainer.optimizer.state_dict()
    return {(i, k): (v.detach().cpu().clone() if torch.is_tensor(v) else v) for i, st in sd["state"].items() for k, v in st.items()}


def test_fp16_overflow_under_replay_skips_the_step_and_recovers(dev, z):
    """precision=16, replay established at a passing scale; the scale is then set ON THE DEVICE to one that overflows: the
    replayed backward reads it, the step is skipped (parameters and both Adam moments bit-equal, scale halved), and the next
    step at a passing scale is taken."""
    from refign_amd.trainer import Trainer
    model = build(dev)
    trainer = Trainer(model, graph_step=True, precision=16, scaler_args={"init_scale": FP16_SCALE})
    batch = matcher_batch(z, dev)
    for it in range(4):
        trainer.step(batch, it)
    assert trainer.step_graph.captured() and trainer.scaler.skipped_steps() == 0
    params = dict(model.alignment_head.named_parameters())
    p1 = {k: v.detach().clone() for k, v in params.items()}
    s1 = _optimizer_state(trainer)
    assert any(k[1] == "exp_avg" for k in s1) and any(k[1] == "exp_avg_sq" for k in s1)
    huge = 2.0 ** 100
    trainer.scaler._scale.fill_(huge)
    trainer.step(batch, 4)
    assert trainer.step_graph.captured()
    assert all(torch.equal(v, p1[k]) for k, v in params.items())
    s2 = _optimizer_state(trainer)
    assert s1.keys() == s2.keys() and all(torch.equal(s1[k], s2[k]) if torch.is_tensor(s1[k]) else s1[k] == s2[k] for k in s1)
    assert trainer.scaler.get_scale() == huge / 2 and trainer.scaler.skipped_steps() == 1
    assert model.global_step == 5
    trainer.scaler._scale.fill_(FP16_SCALE)
    trainer.step(batch, 5)
    assert trainer.step_graph.captured() and trainer.scaler.skipped_steps() == 1
    assert any(not torch.equal(v, p1[k]) for k, v in params.items())
    assert all(np.isfinite(v) for v in _logged(model))
    trainer.close()


def test_logged_rows_hold_each_steps_own_losses(dev, z):
    """logger + log_every_n_steps=1 over A A A C A: every row's three losses are that step's model.logged values (the copies
    the trainer left there, read later in stream order), and rows of different batches differ."""
    from refign_amd.trainer import Trainer
    A, _, C = _batches(z, dev)
    model = build(dev)
    trainer = Trainer(model, graph_step=True, logger=Memory(), log_every_n_steps=1)
    kept = []
    for it, batch in enumerate([A, A, A, C, A]):
        trainer.step(batch, it)
        kept.append([model.logged[k] for k in LOSSES])       # read AFTER the later replays: they must not have been overwritten
    seen = [[float(v) for v in row] for row in kept]
    trainer.flush_log()
    assert trainer.step_graph.captured()
    assert [s for s, _ in trainer.log_history] == [0, 1, 2, 3, 4]
    for (_, row), want in zip(trainer.log_history, seen):
        assert [row[k] for k in LOSSES] == want
    assert seen[3] != seen[2] and seen[4] != seen[3] and seen[3][1] != seen[4][1]
    trainer.close()


def _val_loader(z, dev):
    b = matcher_batch(z, dev)
    H, W = b["image_trg"].shape[-2:]
    g = torch.Generator().manual_seed(0)
    pts_t = [torch.stack([torch.rand(50, generator=g) * (W - 1), torch.rand(50, generator=g) * (H - 1)], 1).to(dev)
             for _ in range(2)]
    pts_r = [p + torch.randn(50, 2, generator=g).to(dev) * 3 for p in pts_t]
    return {"MegaDepth": [{"image": b["image_trg"], "image_ref": b["image_ref"], "corr_pts": pts_t, "corr_pts_ref": pts_r}]}


def _with_validation(dev, z, graph):
    from refign_amd.metrics import MyMetricCollection, SparseEPE
    from refign_amd.trainer import Trainer
    model = build(dev)
    model.valid_metrics = MyMetricCollection({"val_MegaDepth_SparseEPE": SparseEPE(uncertainty_estimation=True)})
    trainer = Trainer(model, graph_step=graph)
    batch, rows, captured = matcher_batch(z, dev), [], []

    def state():
        captured.append(trainer.step_graph.captured() if graph else None)
    for it in range(4):
        trainer.step(batch, it)
        rows.append(_logged(model))
    state()
    out = trainer.validate(_val_loader(z, dev))
    assert out and model.training
    state()
    for it in range(4, 7):
        trainer.step(batch, it)
        rows.append(_logged(model))
        state()
    trainer.close()
    return np.asarray(rows), captured


def test_validate_drops_the_graph_and_it_is_captured_again(dev, z):
    a, b = (_with_validation(dev, z, False)[0] for _ in range(2))
    rows, captured = _with_validation(dev, z, True)
    assert captured == [True, False, False, False, True]     # after step 4, after validate, after steps 5, 6, 7
    _check("losses around validate()", rows, a, b)


def _with_resume(dev, z, graph, path):
    from refign_amd.trainer import Trainer
    batch, rows, captured = matcher_batch(z, dev), [], []
    model = build(dev)
    trainer = Trainer(model, graph_step=graph)
    for it in range(3):
        trainer.step(batch, it)
        rows.append(_logged(model))
    captured.append(trainer.step_graph.captured() if graph else None)
    trainer.save_checkpoint(path)
    trainer.close()
    fresh = build(dev)
    resumed = Trainer(fresh, graph_step=graph, ckpt_path=path)
    assert fresh.global_step == 3
    captured.append(resumed.step_graph.captured() if graph else None)
    for it in range(3, 6):
        resumed.step(batch, it)
        rows.append(_logged(fresh))
        captured.append(resumed.step_graph.captured() if graph else None)
    # load_checkpoint on a trainer that is replaying drops its graph too
    resumed.load_checkpoint(path)
    captured.append(resumed.step_graph.captured() if graph else None)
    resumed.close()
    return np.asarray(rows), captured


def test_resume_into_a_graphed_trainer(dev, z, tmp_path):
    path = str(tmp_path / "three.ckpt")
    a, b = (_with_resume(dev, z, False, path)[0] for _ in range(2))
    rows, captured = _with_resume(dev, z, True, path)
    assert captured == [True, False, False, False, True, False]
    _check("losses across save and resume", rows, a, b)


def test_mode_and_dtype_changes_drop_the_graph(dev, z):
    from refign_amd.trainer import Trainer
    model = build(dev)
    trainer = Trainer(model, graph_step=True)
    batch = matcher_batch(z, dev)

    def replaying():
        for it in range(3):
            trainer.step(batch, it)
        return trainer.step_graph.captured()
    assert replaying()
    model.eval()
    assert not trainer.step_graph.captured()
    model.train()
    assert replaying()
    model.to(dev)                                            # _apply
    assert not trainer.step_graph.captured()
    assert replaying()
    trainer.close()
    assert not trainer.step_graph.captured()


def test_switches(dev, z, eager5, monkeypatch):
    """RFN_HIP_GRAPH=0: the keyword is accepted and the step runs eagerly; the UDA model: ValueError; default: no graph."""
    from test_step_gpu import build as build_uda
    from refign_amd.trainer import Trainer
    monkeypatch.setenv("RFN_HIP_GRAPH", "0")
    rows, captured, model, trainer = _run(dev, [matcher_batch(z, dev)] * 5, True)
    assert captured == [False] * 5 and model.global_step == 5
    _check("losses with RFN_HIP_GRAPH=0", rows, eager5[0]["losses"], eager5[1]["losses"])
    trainer.close()
    monkeypatch.delenv("RFN_HIP_GRAPH")
    with pytest.raises(ValueError, match="graphed on their own"):
        Trainer(build_uda(False, dev), graph_step=True)
    plain = Trainer(build(dev))
    assert plain.step_graph is None
    plain.close()


# -- the two backward kernels inside a capture ------------------------------------------------------------------------------
def _capture(fn):
    """torch.cuda.graph around fn() after one eager call on a side stream -> (graph, fn's outputs)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


@pytest.mark.parametrize("B,C,H,W,amp", [(2, 5, 17, 23, 3.0), (1, 33, 32, 40, 12.0), (2, 2, 9, 1, 2.0), (1, 64, 8, 8, 30.0)])
def test_warp_backward_inside_a_capture(dev, B, C, H, W, amp):
    """matching.warp + backward captured once, replayed three times with grad_out, x and flow rewritten in place: every
    replay's grad_x and grad_flow match grid_sample's autograd (the tolerance of
    test_matcher_gpu.test_warp_backward_matches_grid_sample_autograd); one channel group (C <= 32): grad_flow is stored, not
    added -- bit-equal between two replays of the same inputs."""
    from refign_amd.matching import warp
    gen = torch.Generator().manual_seed(B * 100 + C)

    def draw():
        return (torch.randn(B, C, H, W, generator=gen).to(dev), (torch.randn(B, 2, H, W, generator=gen) * amp).to(dev),
                torch.randn(B, C, H, W, generator=gen).to(dev))
    x, flo, go = draw()
    xs, fs = x.clone().requires_grad_(True), flo.clone().requires_grad_(True)

    def fn():
        return torch.autograd.grad(warp(xs, fs, check_zero=False), (xs, fs), go)
    graph, (gx, gf) = _capture(fn)
    for replay in range(3):
        if replay:
            nx, nf, ng = draw()
            with torch.no_grad():
                xs.copy_(nx)
                fs.copy_(nf)
                go.copy_(ng)
        graph.replay()
        x2, f2 = xs.detach().clone().requires_grad_(True), fs.detach().clone().requires_grad_(True)
        _grid_sample_warp(x2, f2).backward(go)
        for a, b, name in ((gx, x2.grad, "grad x"), (gf, f2.grad, "grad flow")):
            assert float((a - b).abs().max()) <= 2e-5 * max(float(b.abs().max()), 1.0), (name, replay)
        if C <= 32:
            first = gf.clone()
            graph.replay()
            assert torch.equal(first, gf), replay


def test_generic_correlation_backward_inside_a_capture(dev):
    """The scatter kernel of the generic fp32 backward (kernel 3, patch 5, stride 2) captured and replayed three times --
    the golden gradients, twice them for a doubled grad_out (exact scaling), and the golden gradients again, at the tolerance
    of test_ops_gpu.test_corr_fwd_bwd_golden."""
    from refign_amd import correlation
    g = golden("corr_gen_k3_p5_s2")
    a = [int(v) for v in g["args"]]
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    in1, in2, go = t(g["in1"]), t(g["in2"]), t(g["grad_out"])
    assert in1.dtype == torch.float32
    graph, (g1, g2) = _capture(lambda: correlation.backward(in1, in2, go, *a))
    for factor in (1.0, 2.0, 1.0):
        go.copy_(t(g["grad_out"]) * factor)
        graph.replay()
        np.testing.assert_allclose(g1.cpu().numpy(), factor * g["grad_in1"], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(g2.cpu().numpy(), factor * g["grad_in2"], rtol=1e-4, atol=1e-4)

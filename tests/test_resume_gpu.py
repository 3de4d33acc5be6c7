"""GPU: a run resumed from Trainer.save_checkpoint continues the uninterrupted run -- the same host draws, losses at the
bound the graphed-vs-eager tests use, the same parameters, LR, Adam step count and loss-scale sequence -- under bf16 with
captured student passes, the fp16 recipe, the fp8 teacher (K5), from a Lightning-layout file without the project's key,
and over two ranks.  A resume from the weights alone misses the trajectory (negative control).
Short LR warm-up (2 steps, lr 1e-4): the moments and the schedule steer the trajectory, so lost optimizer state shows.
At such a rate two runs of the SAME configuration drift apart: the weight-gradient GEMMs and the attention backward
accumulate with float atomics, and Adam turns their last-bit differences on near-zero gradients into lr-sized steps.
Measured on an MI355X over 8 steps (mit_b0, 128 x 128): run-to-run loss deviation up to 1.0 %, resumed run 1.0 %, a
restart from the weights alone 23-37 %.  So the losses are compared at RTOL = 3e-2, the state right after loading, the
host draws, the LR, the step count and the loss scale exactly, and the first resumed step against the saving run itself."""
import os
import random

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from test_step_gpu import build, make_batch

pytestmark = pytest.mark.gpu
LOSSES = ("train_loss_src", "train_loss_featdist_src", "train_loss_uda_trg")
OPT = {"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-4, "weight_decay": 0.01}}
SCH = {"class_path": "helpers.lr_scheduler.LinearWarmupPolynomialLR",
       "init_args": {"warmup_iters": 2, "warmup_ratio": 1e-6, "power": 1.0, "max_steps": 40000}}
RTOL = 3e-2                 # losses of two runs that should follow one trajectory (module docstring)


def _model(dev, teacher_f8=False):
    m = build(True, dev)
    m.optimizer_init, m.lr_scheduler_init = dict(OPT), dict(SCH)
    m.teacher_f8 = teacher_f8
    return m


def _plain(x):
    if torch.is_tensor(x) or isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


@pytest.fixture
def draws(monkeypatch):
    """Every host draw of a step, per step: the DACS coins / classes / jitter / sigmas (uda._dacs_draw) and the HRDA crops."""
    from refign_amd import seg, uda
    rec = []
    real_crop, real_dacs = seg.draw_crop_offsets, uda.DomainAdaptationSegmentationModel._dacs_draw

    def crop(*a, **k):
        off = real_crop(*a, **k)
        rec[-1].append(("crop", off))
        return off

    def dacs(self, *a, **k):
        d = real_dacs(self, *a, **k)
        rec[-1].append(("dacs", d))                # (converted after the step: no host read in the middle of it)
        return d

    monkeypatch.setattr(seg, "draw_crop_offsets", crop)
    monkeypatch.setattr(uda, "draw_crop_offsets", crop)
    monkeypatch.setattr(uda.DomainAdaptationSegmentationModel, "_dacs_draw", dacs)
    return rec


def _steps(dev, trainer, its, rec=None, rank=0, probs=None):
    """Trainer.step over iterations `its`; per step the losses, the LR of every group and the loss scale."""
    model = trainer.model
    rows, lrs, scales = [], [], []
    if probs is not None:                          # the teacher's pseudo-label probabilities, wherever the step takes them
        cls = type(model)
        real_pl = cls._pseudo_labels

        def recording_pl(self, probs_trg):
            if not torch.cuda.is_current_stream_capturing():
                probs.append(probs_trg.detach().float().clone())
            return real_pl(self, probs_trg)
        cls._pseudo_labels = recording_pl
    try:
        for it in its:
            if rec is not None:
                rec.append([])
            batch = make_batch(2, 128, 128, 64, dev)
            batch["image_src"] = batch["image_src"] + 0.1 * it + 0.05 * rank
            trainer.step(batch, it)
            rows.append([float(model.logged[k]) for k in LOSSES])
            lrs.append([g["lr"] for g in trainer.optimizer.param_groups])
            scales.append(trainer.scaler.get_scale() if trainer.scaler is not None else None)
            if rec is not None:
                rec[-1] = _plain(rec[-1])
    finally:
        if probs is not None:
            cls._pseudo_labels = real_pl
    return {"losses": np.array(rows), "lrs": lrs, "scales": scales}


def _abs_sum(model):
    return float(sum(p.detach().double().abs().sum() for p in model.parameters()))


def _adam_steps(trainer):
    return sorted({float(s["step"]) for s in trainer.optimizer.state_dict()["state"].values()})


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def _rng(dev):
    from refign_amd.trainer import _rng_state
    return _rng_state(dev)


def _trajectory_equal(got, want, got_model, want_model):
    np.testing.assert_allclose(got["losses"], want["losses"], rtol=RTOL)
    assert got["lrs"] == want["lrs"]
    assert abs(_abs_sum(got_model) - _abs_sum(want_model)) < 1e-5 * _abs_sum(want_model)


def _resume_case(dev, tmp_path, rec, precision, scaler_args=None, seed=5, n=8):
    """(uninterrupted n steps, n/2 steps + save + fresh model and trainer from the file + n/2 steps) of one configuration;
    asserts that the state right after loading equals the saved one bit for bit and that the first resumed step runs on the
    fused AdamW kernel from the loaded state."""
    from refign_amd.trainer import Trainer
    h = n // 2
    _seed(seed)
    u = Trainer(_model(dev), precision=precision, scaler_args=scaler_args)
    full = _steps(dev, u, range(n), rec)
    full_draws = list(rec)
    del rec[:]
    _seed(seed)
    a = Trainer(_model(dev), precision=precision, scaler_args=scaler_args)
    first = _steps(dev, a, range(h), rec)
    assert u.fast_step.launches == n - 1 and a.fast_step.launches == h - 1        # torch's own first step, then ours
    path = str(tmp_path / "last.ckpt")
    a.save_checkpoint(path)
    saved = {"model": {k: v.clone() for k, v in a.model.state_dict().items()}, "opt": a.optimizer.state_dict(),
             "sch": a.scheduler.state_dict(), "rng": _rng(dev), "gs": a.model.global_step,
             "amp": a.scaler.state_dict() if a.scaler is not None else None}
    a.close()
    b = Trainer(_model(dev), precision=precision, scaler_args=scaler_args, ckpt_path=path)
    # right after loading, before any step: bit for bit what was saved
    assert _same(b.model.state_dict(), saved["model"]) and b.model.global_step == saved["gs"] == h
    assert _same(b.optimizer.state_dict(), saved["opt"])
    assert _same(b.scheduler.state_dict(), saved["sch"])
    assert _same(_rng(dev), saved["rng"])
    if precision == 16:
        assert b.scaler.state_dict() == saved["amp"]
    assert b.fast_step.launches == 0
    rest = _steps(dev, b, range(h, n), rec)
    assert b.fast_step.launches == h                              # the first resumed step on the fused kernel already
    assert len(rec) == n and rec == full_draws, "the resumed steps drew other DACS / crop values"
    got = {"losses": np.concatenate([first["losses"], rest["losses"]]), "lrs": first["lrs"] + rest["lrs"],
           "scales": first["scales"] + rest["scales"]}
    _trajectory_equal(got, full, b.model, u.model)
    assert _adam_steps(b) == _adam_steps(u) == [float(n)]
    for name in ("source_pass", "mixed_pass"):                    # the resumed run captured its own graphs and replayed them
        st = list(b.model._graphs[name].states.values())
        assert len(st) == 1 and st[0]["graph"] is not None and not st[0]["failed"], f"{name}: not captured after resume"
    return u, b, full, got, path


def test_bf16_graphed_resume_continues_the_run(dev, tmp_path, monkeypatch, draws):
    """bf16, student passes captured: 8 steps == 4 steps + save + fresh model / trainer from the file + 4 steps (draws
    identical, losses within RTOL, parameter sum 1e-5, LR and Adam step count exact); a resume from the weights alone, with
    the same random draws, misses the losses by more than that bound."""
    from refign_amd.trainer import Trainer, _set_rng_state
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    u, b, full, got, path = _resume_case(dev, tmp_path, draws, "bf16")
    u.close()
    b.close()
    # negative control: the weights only (load_weights / pretrained=), the RNG streams put back by hand
    c_model = _model(dev)
    c_model.load_weights(path)
    c = Trainer(c_model, precision="bf16")
    _set_rng_state(torch.load(path, map_location="cpu", weights_only=False)["refign_amd"]["rng"][0], dev)
    lost = _steps(dev, c, range(4, 8))
    dev_max = float(np.max(np.abs(lost["losses"] / full["losses"][4:] - 1)))
    print(f"\nresume: loss deviation {np.max(np.abs(got['losses'] / full['losses'] - 1)):.2e}; weights-only restart: {dev_max:.2e}")
    assert dev_max > 3 * RTOL, "a weights-only restart is indistinguishable: the comparison cannot see lost state"
    c.close()


def test_fp16_resume_continues_the_scale_sequence(dev, tmp_path, monkeypatch, draws):
    """precision=16, growth_interval=2: the scale changes before and after the save point; the scale sequence and the skipped
    count equal the uninterrupted run's exactly, the losses / parameters / LR / step count as in the bf16 case."""
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    u, b, full, got, _ = _resume_case(dev, tmp_path, draws, 16, {"init_scale": 2.0 ** 10, "growth_interval": 2})
    assert got["scales"] == full["scales"], (got["scales"], full["scales"])
    assert len(set(full["scales"][:4])) > 1 and len(set(full["scales"][4:])) > 1, full["scales"]
    assert b.scaler.skipped_steps() == u.scaler.skipped_steps()
    assert b.scaler.state_dict() == u.scaler.state_dict()
    u.close()
    b.close()


def test_k5_teacher_resumed_into_a_used_model_labels_like_the_saving_run(dev, tmp_path, monkeypatch):
    """K5 (fp8 EMA teacher): the file is loaded into a trainer that has already run steps of ANOTHER trajectory (fp8 weights
    quantised, 16-bit copies cached, graphs captured).  The teacher's pseudo-labels and the losses of the first resumed step
    equal those of the saving run's next step (same state bit for bit, same draws: no atomics noise between them)."""
    from refign_amd.trainer import Trainer
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    _seed(7)
    a = Trainer(_model(dev, teacher_f8=True), precision="bf16")
    _steps(dev, a, range(4))
    path = str(tmp_path / "k5.ckpt")
    a.save_checkpoint(path)
    p_full = []
    full = _steps(dev, a, range(4, 5), probs=p_full)
    a.close()
    _seed(99)
    b = Trainer(_model(dev, teacher_f8=True), precision="bf16")
    _steps(dev, b, range(10, 13))                                  # another trajectory first: every cache is warm
    b.load_checkpoint(path)
    p_res = []
    rest = _steps(dev, b, range(4, 5), probs=p_res)
    assert len(p_res) == len(p_full) == 1
    assert torch.equal(p_res[0].argmax(1), p_full[0].argmax(1))
    torch.testing.assert_close(p_res[0], p_full[0], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rest["losses"], full["losses"], rtol=1e-4)
    b.close()


@pytest.mark.parametrize("saver_fused", [False, True])
def test_lightning_layout_file_crosses_optimizer_implementations(dev, tmp_path, monkeypatch, saver_fused):
    """A file as Lightning lays it out (state_dict, optimizer_states, lr_schedulers, global_step; no `refign_amd` key) from a
    fused_optimizer=False trainer loads into a fused one, and the other way round: it warns that the draws are not
    restored, and -- with the draws put back by hand -- continues the trajectory within the bf16 case's bounds."""
    from refign_amd.trainer import Trainer, _set_rng_state
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    _seed(11)
    u = Trainer(_model(dev), precision="bf16", fused_optimizer=saver_fused)
    _steps(dev, u, range(4))
    rng = _rng(dev)
    u.save_checkpoint(str(tmp_path / "full.ckpt"))
    ck = torch.load(str(tmp_path / "full.ckpt"), map_location="cpu", weights_only=False)
    path = str(tmp_path / "lightning.ckpt")
    torch.save({k: ck[k] for k in ("epoch", "global_step", "pytorch-lightning_version", "state_dict", "optimizer_states",
                                   "lr_schedulers")}, path)
    _set_rng_state(rng, dev)
    full = _steps(dev, u, range(4, 8))
    with pytest.warns(UserWarning, match="RNG"):
        b = Trainer(_model(dev), precision="bf16", fused_optimizer=not saver_fused, ckpt_path=path)
    assert b.model.global_step == 4
    assert all(bool(g.get("fused")) == (not saver_fused) for g in b.optimizer.param_groups)      # the trainer's own flags
    _set_rng_state(rng, dev)
    rest = _steps(dev, b, range(4, 8))
    if not saver_fused:
        assert b.fast_step.launches == 4
    _trajectory_equal(rest, full, b.model, u.model)
    assert _adam_steps(b) == _adam_steps(u) == [8.0]
    u.close()
    b.close()


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_rank_resume_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RFN_GRAPH_STUDENT="1", RFN_STALL_S="10")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import time

    from refign_amd import trainer as T
    dev = torch.device("cuda:0")
    res = {}
    _seed(5 + rank)
    u = T.Trainer(_model(dev), precision="bf16")
    assert u.guard is not None and u.guard.limit == 10
    res["full"] = _steps(dev, u, range(6), rank=rank)
    res["full_sum"] = _abs_sum(u.model)
    u.close()
    _seed(5 + rank)
    a = T.Trainer(_model(dev), precision="bf16")
    _steps(dev, a, range(3), rank=rank)
    real_write = T._write_file

    def slow_write(obj, f):                        # a slow shared disk: longer than the stall guard's limit
        time.sleep(14)
        real_write(obj, f)

    T._write_file = slow_write
    path = os.path.join(out, "last.ckpt")
    a.save_checkpoint(path)                        # rank 0 writes, rank 1 waits for it: neither guard fires
    T._write_file = real_write
    a.close()
    b = T.Trainer(_model(dev), precision="bf16", ckpt_path=path)
    res["rest"] = _steps(dev, b, range(3, 6), rank=rank)
    res["rest_sum"] = _abs_sum(b.model)
    res["world_in_file"] = torch.load(path, map_location="cpu", weights_only=False)["refign_amd"]["world_size"]
    b.close()
    torch.save(res, f"{out}/r{rank}.pt")
    dist.destroy_process_group()


def test_two_ranks_resume_from_one_file(dev, tmp_path):
    """Two ranks on one GPU over gloo: rank 0 writes one file (through a writer slower than the stall guard's limit), both
    ranks resume from it with their own RNG states, and each rank's losses follow the uninterrupted two-rank run's."""
    port, out = _free_port(), str(tmp_path)
    mp.spawn(_two_rank_resume_worker, args=(2, port, out), nprocs=2, join=True)
    for rank in range(2):
        r = torch.load(f"{out}/r{rank}.pt", weights_only=False)
        assert r["world_in_file"] == 2
        np.testing.assert_allclose(r["rest"]["losses"], r["full"]["losses"][3:], rtol=RTOL)
        assert r["rest"]["lrs"] == r["full"]["lrs"][3:]
        assert abs(r["rest_sum"] - r["full_sum"]) < 1e-5 * r["full_sum"]
    r0, r1 = (torch.load(f"{out}/r{k}.pt", weights_only=False) for k in range(2))
    assert not np.array_equal(r0["full"]["losses"], r1["full"]["losses"])      # the ranks really ran different draws

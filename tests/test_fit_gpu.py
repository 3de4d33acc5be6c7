"""GPU: Trainer.fit / validate / test around the real training step.  Two runs of this step do not agree bit for bit (float
atomics in some backward kernels; test_resume_gpu.py compares trajectories with RTOL = 3e-2 on the losses and 1e-5 on the
parameters' absolute sum for that reason), so what is exact is asserted exactly -- a validation leaves every tensor and
counter a later step reads bit-equal; host draws, LRs, Adam step counts and the loss-scale sequence of a run with
validations equal those of a run without -- and the trajectory is held to those same, existing bounds."""
import copy

import numpy as np
import pytest
import torch
from test_resume_gpu import (LOSSES, _abs_sum, _adam_steps, _model, _plain, _rng, _same, _seed, _trajectory_equal,  # noqa: F401
                             draws)
from test_step_gpu import make_batch

pytestmark = pytest.mark.gpu
SCALER = {"init_scale": 2.0 ** 10, "growth_interval": 2}


def _train_batches(dev, n):
    out = []
    for it in range(n):
        b = make_batch(2, 128, 128, 64, dev)
        b["image_src"] = b["image_src"] + 0.1 * it
        out.append(b)
    return out


def _val_loaders(dev):
    b = make_batch(2, 128, 128, 64, dev)
    return {"ACDC": [{"image": b["image_trg"], "semantic": b["semantic_src"]},
                     {"image": b["image_ref"].cpu(), "semantic": b["semantic_src"].cpu()}],
            "DarkZurich": [{"image": b["image_src"], "semantic": b["semantic_src"]}]}


def _with_metrics(model, dev):
    from refign_amd.metrics import IoU, MyMetricCollection
    model.valid_metrics = MyMetricCollection({f"val_{d}_IoU": IoU(num_classes=19, ignore_index=255)
                                              for d in ("ACDC", "DarkZurich")}).to(dev)
    model.test_metrics = MyMetricCollection({"test_ACDC_IoU": IoU(num_classes=19, ignore_index=255),
                                             "test_ACDC_IoU_classes": IoU(num_classes=19, ignore_index=255,
                                                                          average="none")}).to(dev)
    model.use_slide_inference, model.inference_batched_slide = True, True
    model.inference_crop_size, model.inference_stride = [64, 64], [40, 48]
    return model


def _trainer(dev, precision):
    from refign_amd.trainer import Trainer
    return Trainer(_with_metrics(_model(dev), dev), precision=precision, scaler_args=SCALER if precision == 16 else None)


def _recording(trainer, rec):
    """Wrap trainer.step: per step the host draws (into `rec`, the `draws` fixture's list), the losses, the LR of every group,
    the loss scale and the next_batch it was given."""
    real, model = trainer.step, trainer.model
    log = {"losses": [], "lrs": [], "scales": [], "next": []}

    def step(batch, batch_idx=0, next_batch=None):
        rec.append([])
        out = real(batch, batch_idx, next_batch=next_batch)
        log["losses"].append([float(model.logged[k]) for k in LOSSES])
        log["lrs"].append([g["lr"] for g in trainer.optimizer.param_groups])
        log["scales"].append(trainer.scaler.get_scale() if trainer.scaler is not None else None)
        log["next"].append(next_batch)
        rec[-1] = _plain(rec[-1])
        return out

    trainer.step = step
    return log


def _done(log):
    return dict(log, losses=np.array(log["losses"]))


def _snapshot(tr, dev):
    torch.cuda.synchronize()
    return copy.deepcopy({"model": dict(tr.model.state_dict()), "opt": tr.optimizer.state_dict(),
                          "sch": tr.scheduler.state_dict(), "amp": tr.scaler.state_dict() if tr.scaler is not None else None,
                          "skipped": tr.scaler.skipped_steps() if tr.scaler is not None else None,
                          "gs": tr.model.global_step, "rng": _rng(dev)})


@pytest.mark.parametrize("precision", ["bf16", 16])
def test_validate_leaves_the_run_bit_equal(dev, monkeypatch, precision):
    """Two steps, a snapshot of everything a later step reads (parameters, EMA parameters, BatchNorm running statistics and
    batch counters, optimizer, scheduler, loss scaler, global_step, the four RNG states), then validate() on the fused path
    and again with RFN_EVAL_FUSED=0: every item bit-equal, the model back in training mode with the alignment nets and the
    ImageNet encoder in eval mode."""
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    _seed(5)
    tr = _trainer(dev, precision)
    model = tr.model
    batches = _train_batches(dev, 2)
    tr.step(batches[0], 0, next_batch=batches[1])
    tr.step(batches[1], 1)
    snap = _snapshot(tr, dev)
    assert any(k.endswith("num_batches_tracked") for k in snap["model"]) and snap["gs"] == 2
    val = _val_loaders(dev)
    steps = []
    real = model.validation_step
    model.validation_step = lambda *a, **k: (steps.append(1), real(*a, **k))[1]
    for fused, calls in (("1", 0), ("0", 3)):
        monkeypatch.setenv("RFN_EVAL_FUSED", fused)
        out = tr.validate(val)
        assert len(steps) == calls, f"RFN_EVAL_FUSED={fused}: {len(steps)} validation_step calls"
        assert set(out) == {"val_ACDC_IoU", "val_DarkZurich_IoU"} and all(np.isfinite(v) for v in out.values())
        now = _snapshot(tr, dev)
        for k in snap:
            assert _same(now[k], snap[k]), f"RFN_EVAL_FUSED={fused}: validate() changed {k}"
        assert model.training and model.backbone.training and model.head.training
        assert not model.alignment_backbone.training and not model.alignment_head.training
        assert not model.imnet_backbone.training
    tr.close()


@pytest.mark.parametrize("precision", ["bf16", 16])
def test_validation_inside_fit_does_not_change_the_trajectory(dev, monkeypatch, draws, precision):
    """Run A = fit to step 9; run B = fit to step 4 with a validation after EVERY step, then on to step 9: the same host draws,
    LRs, Adam step counts (and loss-scale sequence under precision=16) exactly, losses and parameter sum within the resume
    tests' bounds; after run B the student graphs are captured again and replaying."""
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    batches = _train_batches(dev, 9)
    _seed(5)
    a = _trainer(dev, precision)
    log_a = _recording(a, draws)
    assert a.fit(batches, max_steps=9) == []
    draws_a = list(draws)
    del draws[:]
    _seed(5)
    b = _trainer(dev, precision)
    log_b = _recording(b, draws)
    hist = b.fit(batches[:4], val_loaders=_val_loaders(dev), max_steps=4, val_every_n_steps=1)
    assert [s for s, _ in hist] == [1, 2, 3, 4]
    assert all(np.isfinite(v) for _, m in hist for v in m.values())
    assert b.fit(batches[4:], max_steps=9) == []
    assert len(draws) == 9 and list(draws) == draws_a, "validation changed the host draws of the training steps"
    got, want = _done(log_b), _done(log_a)
    print(f"\n{precision}: loss deviation with validations {np.max(np.abs(got['losses'] / want['losses'] - 1)):.2e}")
    _trajectory_equal(got, want, b.model, a.model)
    assert _adam_steps(a) == _adam_steps(b) == [9.0]
    if precision == 16:
        assert got["scales"] == want["scales"] and len(set(want["scales"])) > 1, (got["scales"], want["scales"])
        assert a.scaler.skipped_steps() == b.scaler.skipped_steps()
    # (fit's look-ahead gives a pass two input signatures after a validation: step 5 has no prefetched features of its batch and
    # runs once eagerly; steps 6-9 share the signature that is captured on its third call, where the count stops, and step 9
    # replays it)
    for name in ("source_pass", "mixed_pass"):
        g = b.model._graphs[name]
        st = list(g.states.values())
        assert not any(s["failed"] for s in st), f"{name}: a capture failed after validation"
        assert [s["calls"] for s in st if s["graph"] is not None] == [3], f"{name}: not captured after validation: {st}"
        assert g.captured(), f"{name}: the last step did not replay its graph"
    a.close()
    b.close()


def test_fit_equals_hand_written_steps(dev, monkeypatch, draws):
    """fit over 3 steps == step(b0, next_batch=b1), step(b1, next_batch=b2), step(b2): the look-ahead fit does is the one a
    caller would write; same draws, LRs exact, losses and parameter sum within the bounds."""
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    batches = _train_batches(dev, 3)
    _seed(9)
    a = _trainer(dev, "bf16")
    log_a = _recording(a, draws)
    for i in range(3):
        a.step(batches[i], i, next_batch=batches[i + 1] if i < 2 else None)
    draws_a = list(draws)
    del draws[:]
    _seed(9)
    b = _trainer(dev, "bf16")
    log_b = _recording(b, draws)
    b.fit(batches, max_steps=3)
    assert [n is not None for n in log_b["next"]] == [True, True, False]
    assert all(n is batches[i + 1] for i, n in enumerate(log_b["next"][:2]))       # device batches are handed on as they are
    assert list(draws) == draws_a and b.model.global_step == 3
    _trajectory_equal(_done(log_b), _done(log_a), b.model, a.model)
    assert _adam_steps(a) == _adam_steps(b) == [3.0]
    a.close()
    b.close()


def test_test_after_fit_reports_the_configured_metrics(dev, monkeypatch, tmp_path):
    monkeypatch.setenv("RFN_GRAPH_STUDENT", "1")
    _seed(3)
    tr = _trainer(dev, "bf16")
    tr.fit(_train_batches(dev, 2), max_steps=2, ckpt_dir=str(tmp_path))
    assert torch.load(str(tmp_path / "last.ckpt"), map_location="cpu", weights_only=False)["global_step"] == 2
    out = tr.test({"ACDC": _val_loaders(dev)["ACDC"]})
    assert set(out) == set(tr.model.test_metrics.keys()) == {"test_ACDC_IoU", "test_ACDC_IoU_classes"}
    assert isinstance(out["test_ACDC_IoU"], float) and np.isfinite(out["test_ACDC_IoU"])
    assert len(out["test_ACDC_IoU_classes"]) == 19 and all(np.isfinite(v) for v in out["test_ACDC_IoU_classes"])
    assert abs(np.mean(out["test_ACDC_IoU_classes"]) - out["test_ACDC_IoU"]) < 1e-6
    assert tr.model.training
    tr.close()


def test_alignment_model_validates_through_the_trainer(dev):
    """validate() is not tied to the segmentation model: AlignmentModel's validation_step feeds SparseEPE (no fused path
    there), the result equals the metric fed by hand from the model's forward, and the matcher is back in training mode with
    its frozen backbone's norm layers in eval mode."""
    from conftest import golden
    from refign_amd.metrics import MyMetricCollection, SparseEPE
    from refign_amd.trainer import Trainer
    from test_matcher_gpu import build_matcher, matcher_batch
    model = build_matcher(dev)
    model.valid_metrics = MyMetricCollection({"val_MegaDepth_SparseEPE": SparseEPE(uncertainty_estimation=True),
                                              "val_RobotCarMatching_SparseEPE": SparseEPE(uncertainty_estimation=True)})
    tr = Trainer(model)
    b = matcher_batch(golden("matcher_step_128x160"), dev)
    H, W = b["image_trg"].shape[-2:]
    g = torch.Generator().manual_seed(0)
    pts_t = [torch.stack([torch.rand(300, generator=g) * (W - 1), torch.rand(300, generator=g) * (H - 1)], 1).to(dev)
             for _ in range(2)]
    pts_r = [p + torch.randn(300, 2, generator=g).to(dev) * 3 for p in pts_t]
    batch = {"image": b["image_trg"].cpu(), "image_ref": b["image_ref"], "corr_pts": pts_t, "corr_pts_ref": pts_r}
    out = tr.validate({"MegaDepth": [batch]})
    assert model.training and model.alignment_head.training
    model.eval()
    with torch.no_grad():
        flow, unc = model(b["image_trg"], b["image_ref"])
    direct = SparseEPE(uncertainty_estimation=True)
    direct(flow, pts_r, pts_t, (H, W), unc)
    for k, v in direct.compute().items():
        assert abs(out["val_MegaDepth_SparseEPE_" + k] - float(v)) <= 1e-6 * max(1.0, abs(float(v))), k
    assert all(isinstance(v, float) for v in out.values())
    tr.close()

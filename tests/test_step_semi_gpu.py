"""GPU: the training step on the source batches of the semi-supervised RobotCar recipe (two labelled loaders of two samples each
next to two targets, `ignore_every_second_semantic_training_batch`): FOUR source samples, or the first TWO of them by coin.

  * the step on four source samples and two targets against the reference's own training_step
    (tests/golden/step_daformer_semi_96x128.npz, tests/golden/make_golden_step_semi.py), fp32 parity mode, with the bounds of
    test_step_gpu.py::test_training_step_matches_reference for step_daformer_96x128;
  * six Trainer.step calls whose source batches alternate 4, 2, 4, 2, 4, 2 as halved views of one buffer -- two signatures of
    the student's source pass, each captured on its own -- against the same six calls with RFN_HIP_GRAPH=0, with the bounds of
    test_step_gpu.py::test_student_passes_graph_replay_equals_eager."""
import random

import numpy as np
import pytest
import torch
from test_step_gpu import build, golden, make_batch

pytestmark = pytest.mark.gpu
BLK, N_SRC, N_TRG = 32, 4, 2
LOSSES = ("train_loss_src", "train_loss_featdist_src", "train_loss_uda_trg")


def semi_batch(H, W, dev):
    """make_golden_step_semi.semi_batch: make_batch(4, ...)'s source half, make_batch(2, ...)'s target half"""
    src, trg = make_batch(N_SRC, H, W, BLK, dev), make_batch(N_TRG, H, W, BLK, dev)
    return {"image_src": src["image_src"], "semantic_src": src["semantic_src"], "image_trg": trg["image_trg"],
            "image_ref": trg["image_ref"]}


def test_step_with_four_source_samples_matches_reference(dev):
    from refign_amd.trainer import Trainer
    g = golden("step_daformer_semi_96x128")
    H, W = [int(v) for v in g["size"]]
    model = build(False, dev)
    trainer = Trainer(model, fused_optimizer=False)
    trainer.scheduler = torch.optim.lr_scheduler.LambdaLR(trainer.optimizer, lambda s: 1.0)   # as in the golden run
    model._scheduler = trainer.scheduler
    batch = semi_batch(H, W, dev)
    assert batch["image_src"].shape[0] == 4 and batch["image_trg"].shape[0] == 2
    random.seed(77); np.random.seed(77); torch.manual_seed(77)
    model.global_step = 3
    norms = {}
    real_step = trainer.optimizer.step

    def recording_step(*a, **k):
        norms["v"] = [float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in grp["params"])))
                      for grp in trainer.optimizer.param_groups]
        return real_step(*a, **k)

    trainer.optimizer.step = recording_step
    model.training_step(batch, 0)
    losses = np.array([float(model.logged[k]) for k in LOSSES])
    ema = float(sum(p.double().abs().sum() for p in model.ema_parameters()))
    live = float(sum(p.double().abs().sum() for p in model.live_parameters()))
    print(f"\nlosses {losses} vs {g['losses']}; grad norms {norms['v']} vs {g['grad_norms']}; ema {ema} vs {float(g['ema_abs_sum'])}; "
          f"live {live} vs {float(g['live_abs_sum'])}")
    np.testing.assert_allclose(losses, g["losses"], rtol=2e-3)
    np.testing.assert_allclose(np.array(norms["v"]), g["grad_norms"], rtol=2e-2)
    assert abs(ema - float(g["ema_abs_sum"])) < 1e-5 * float(g["ema_abs_sum"])
    assert abs(live - float(g["live_abs_sum"])) < 1e-5 * float(g["live_abs_sum"])
    assert model.global_step == 4


def test_alternating_source_batch_graphed_equals_eager(dev, monkeypatch):
    """graphs at their defaults against RFN_HIP_GRAPH=0: the same three losses per step, the same parameters after six steps.
    The source pass sees (4, 3, H, W) and (2, 3, H, W) in turn, as views of ONE buffer whose content changes from step to step;
    with graphs on, each signature is captured on its own (on its third call) and the sixth step replays."""
    from refign_amd.trainer import Trainer
    H, W = 96, 128
    traj = {}
    for mode in ("default", "0"):
        if mode == "0":
            monkeypatch.setenv("RFN_HIP_GRAPH", "0")
        else:
            monkeypatch.delenv("RFN_HIP_GRAPH", raising=False)
            monkeypatch.delenv("RFN_GRAPH_STUDENT", raising=False)
        model = build(False, dev)
        trainer = Trainer(model, fused_optimizer=False)
        random.seed(6); np.random.seed(6); torch.manual_seed(6)
        base = semi_batch(H, W, dev)
        buf_img, buf_lbl = torch.empty_like(base["image_src"]), base["semantic_src"].clone()
        rows, sizes = [], []
        for it in range(6):
            buf_img.copy_(base["image_src"] + 0.1 * it)
            n = N_SRC if it % 2 == 0 else N_SRC // 2
            batch = dict(base, image_src=buf_img[:n], semantic_src=buf_lbl[:n])
            assert batch["image_src"].data_ptr() == buf_img.data_ptr()
            trainer.step(batch, it)
            sizes.append(n)
            rows.append([float(model.logged[k]) for k in LOSSES])
        assert sizes == [4, 2, 4, 2, 4, 2]
        traj[mode] = (np.array(rows), float(sum(p.double().abs().sum() for p in model.live_parameters())))
        if mode == "default":
            states = list(model._graphs["source_pass"].states.values())
            assert len(states) == 2, f"the source pass has {len(states)} signatures, two batch sizes were run"
            for name in ("source_pass", "mixed_pass"):
                st = list(model._graphs[name].states.values())
                assert all(s["graph"] is not None and not s["failed"] for s in st), f"{name}: a signature was not captured"
        else:
            assert all(len(g_.states) == 0 or all(s["graph"] is None for s in g_.states.values()) for g_ in model._graphs.values())
        trainer.close()
    print(f"\nlosses graphed\n{traj['default'][0]}\neager\n{traj['0'][0]}\nparameters {traj['default'][1]} vs {traj['0'][1]}")
    np.testing.assert_allclose(traj["default"][0], traj["0"][0], rtol=2e-3)
    assert abs(traj["default"][1] - traj["0"][1]) < 1e-5 * traj["0"][1]

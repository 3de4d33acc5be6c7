"""CPU: what Trainer(graph_step=True) does outside the device -- argument handling, the order of the graph's inputs, the
host-list -> tensor conversion of prime_trg_idx, and the invalidation hooks of AlignmentModel."""
import pytest
import torch
import torch.nn as nn


class Tiny(nn.Module):
    """A stand-in with the matcher's interface towards the trainer: automatic optimization, the batch keys, three logged losses."""

    def __init__(self, automatic=True):
        super().__init__()
        self.lin = nn.Linear(4, 1)
        self.logged, self.global_step = {}, 0
        if automatic:
            self.automatic_optimization = True
        self.optimizer_init = {"class_path": "torch.optim.Adam", "init_args": {"lr": 1e-2}}
        self._optimizer = self._scheduler = self._backward = None
        self.seen = []

    def configure_optimizers(self):
        opt = torch.optim.Adam(self.parameters(), lr=1e-2)
        return [opt], [{"scheduler": torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.5), "interval": "step"}]

    def training_step(self, batch, batch_idx=0):
        self.seen.append(batch)
        scale = torch.as_tensor(batch["prime_trg_idx"]).to(torch.float32).sum() + 1   # (a list from the default trainer)
        ss = self.lin(batch["image_ref"]).pow(2).mean() * scale
        us = (self.lin(batch["image_trg"]) - self.lin(batch["image_prime"])).abs().mean() + batch["flow_prime"].mean() \
            + batch["mask_prime"].float().mean()
        loss = ss + us
        for k, v in (("train_matching_loss", loss), ("train_ss_loss", ss), ("train_us_loss", us)):
            self.logged[k] = v.detach()
        return loss


def _batch(idx):
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"mask_prime": torch.ones(2, 3, dtype=torch.bool), "image_prime": r(2, 4), "prime_trg_idx": idx, "flow_prime": r(2, 2),
            "image_trg": r(2, 4), "image_ref": r(2, 4), "extra": "ignored"}


def test_graph_step_needs_automatic_optimization():
    from refign_amd.trainer import Trainer
    with pytest.raises(ValueError, match="graphed on their own"):
        Trainer(Tiny(automatic=False), graph_step=True)


def test_graph_step_is_accepted_off_the_gpu_and_runs_eagerly():
    """Same seeds, same batches: the trainer with graph_step=True takes bit-equal steps to the default one's on the CPU, never
    captures, and hands training_step a device tensor for prime_trg_idx."""
    from refign_amd.graphs import GraphedStep
    from refign_amd.trainer import Trainer
    out = []
    for graph in (False, True):
        torch.manual_seed(0)
        model = Tiny()
        trainer = Trainer(model, graph_step=graph)
        assert (trainer.step_graph is None) == (not graph)
        rows = []
        for it, idx in enumerate(([0, 1], torch.tensor([1, 1]), [1, 0], [0, 1])):
            trainer.step(_batch(idx), it)
            rows.append([float(model.logged[k]) for k in ("train_matching_loss", "train_ss_loss", "train_us_loss")])
            if graph:
                assert isinstance(trainer.step_graph, GraphedStep) and not trainer.step_graph.captured()
                assert torch.is_tensor(model.seen[-1]["prime_trg_idx"]) and model.seen[-1]["prime_trg_idx"].dtype == torch.int64
                assert "extra" not in model.seen[-1]
        assert model.global_step == 4
        out.append((rows, [p.detach().clone() for p in model.parameters()]))
        trainer.close()
    assert out[0][0] == out[1][0]
    assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))
    assert out[0][0][0] != out[0][0][1]


def test_step_graph_inputs_order_and_missing_keys():
    from refign_amd.trainer import STEP_GRAPH_INPUTS, step_graph_inputs
    assert STEP_GRAPH_INPUTS == ("image_ref", "image_trg", "image_prime", "flow_prime", "mask_prime", "prime_trg_idx")
    b = _batch([1, 0])
    got = step_graph_inputs(b, "cpu")
    assert len(got) == 6
    assert all(got[i] is b[k] for i, k in enumerate(STEP_GRAPH_INPUTS[:5]))
    assert got[5].tolist() == [1, 0]
    del b["flow_prime"]
    with pytest.raises(KeyError, match="flow_prime"):
        step_graph_inputs(b, "cpu")


def test_prime_idx_tensor():
    import numpy as np
    from refign_amd.trainer import prime_idx_tensor
    for idx in ([0, 1, 1], (1, 0, 1), np.asarray([1, 1, 0]), [True, False, True]):
        t = prime_idx_tensor(idx, "cpu")
        assert t.dtype == torch.int64 and t.device.type == "cpu" and t.tolist() == [int(v) for v in idx]
    have = torch.tensor([1, 0], dtype=torch.int64)
    assert prime_idx_tensor(have, torch.device("cpu")) is have          # already where and what it has to be: handed through
    assert prime_idx_tensor(torch.tensor([1, 0], dtype=torch.int32), "cpu").dtype == torch.int64


def test_alignment_model_resets_the_step_graph_with_its_own():
    """train() / eval() / _apply / load_state_dict bump the generation of a GraphedStep left in `_step_graph` (and drop its
    states); a pickled or copied model carries none."""
    import copy
    from refign_amd.alignment_model import AlignmentModel
    from refign_amd.graphs import GraphedStep
    m = AlignmentModel(alignment_backbone=nn.Conv2d(1, 1, 1), alignment_head=nn.Conv2d(1, 1, 1))
    g = GraphedStep(lambda *a: a, "stand-in")
    m.__dict__["_step_graph"] = g
    gen = g.generation
    for act in (m.eval, m.train, m.double, lambda: m.load_state_dict(m.state_dict())):
        g.states["key"] = {"calls": 2, "graph": object(), "failed": False}
        g._last = g.states["key"]
        assert g.captured()
        act()
        assert g.generation == gen + 1 and not g.states and not g.captured()
        gen = g.generation
    assert "_step_graph" not in copy.deepcopy(m).__dict__
    assert m.__dict__["_step_graph"] is g

"""CPU: what training the matcher through Trainer added outside the kernels -- the declared and bound entry points, the
hand-over rule of MultiTensorAdam, the torch formulation of the losses for CPU tensors, and the stage-2 config's
`trainer:` section through config.trainer_kwargs."""
import os
import re

import pytest
import torch
import yaml
from conftest import ROOT, golden

NEW_ENTRY_POINTS = ("rfn_flowloss_block_pixels", "rfn_flowloss_fwd_f32", "rfn_flowloss_bwd_f32", "rfn_multi_adam_f32",
                    "rfn_multi_adam_amp_f32")


def test_header_declares_and_library_binds_the_new_entry_points():
    from ctypes import c_double, c_float, c_int, c_void_p
    import refign_amd
    from refign_amd import _lib
    text = open(os.path.join(ROOT, "include", "refign_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES, name
    p, i = c_void_p, c_int
    assert _lib.SIGNATURES["rfn_flowloss_fwd_f32"] == (i, [p, i, i, i, p, p, i, i, c_float, p, i, p, p, p])
    assert _lib.SIGNATURES["rfn_flowloss_bwd_f32"] == (i, [p, i, i, i, p, p, i, i, c_float, p, p, p])
    assert _lib.SIGNATURES["rfn_multi_adam_f32"] == _lib.SIGNATURES["rfn_multi_adamw_f32"]
    assert _lib.SIGNATURES["rfn_multi_adam_amp_f32"] == _lib.SIGNATURES["rfn_multi_adamw_amp_f32"]
    assert c_double not in _lib.SIGNATURES["rfn_flowloss_fwd_f32"][1]
    lib = _lib.load_library()
    for name in NEW_ENTRY_POINTS:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert refign_amd.abi_version() == 5 and _lib.ABI_VERSION == 5
    assert lib.rfn_flowloss_block_pixels() == 1024


def test_flowloss_entry_points_check_their_arguments():
    """Host-side checks only (nothing is launched): null pointers, level counts, loss types."""
    import numpy as np
    from refign_amd import _lib
    lib = _lib.load_library()
    levels = np.asarray([[64, 0, 0, 0, 0, 4, 4, 0]], dtype=np.int64)
    w = np.ones(1)
    ok = (64, 1, 8, 8, levels.ctypes.data, w.ctypes.data)
    assert lib.rfn_flowloss_fwd_f32(None, 1, 8, 8, levels.ctypes.data, w.ctypes.data, 1, 0, 1.0, 64, 1, 64, 64, None) != 0
    assert lib.rfn_flowloss_fwd_f32(*ok, 9, 0, 1.0, 64, 1, 64, 64, None) != 0            # more than 8 levels
    assert lib.rfn_flowloss_fwd_f32(*ok, 1, 3, 1.0, 64, 1, 64, 64, None) != 0            # unknown loss type
    assert lib.rfn_flowloss_fwd_f32(*ok, 1, 0, 1.0, 64, 2, 64, 64, None) != 0            # a workspace of the wrong size
    assert b"workspace" in lib.rfn_last_error()
    bad = levels.copy()
    bad[0, 7] = 3                                                                         # log-variance channels
    assert lib.rfn_flowloss_bwd_f32(64, 1, 8, 8, bad.ctypes.data, w.ctypes.data, 1, 0, 1.0, 64, 64, None) != 0


def test_multi_tensor_adam_plain_accepts_adam_only(monkeypatch):
    """_plain with the device test out of the way: Adam yes; AdamW, amsgrad, maximize no."""
    from refign_amd.optim import MultiTensorAdam
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))

    def fast(cls, **kw):
        p = torch.nn.Parameter(torch.zeros(4))
        p.grad = torch.ones(4)
        return MultiTensorAdam(cls([p], lr=1e-3, **kw))
    assert fast(torch.optim.Adam, weight_decay=4e-4)._plain() is True
    assert fast(torch.optim.AdamW)._plain() is False
    assert fast(torch.optim.Adam, amsgrad=True)._plain() is False
    assert fast(torch.optim.Adam, maximize=True)._plain() is False
    if "decoupled_weight_decay" in torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).param_groups[0]:
        assert fast(torch.optim.Adam, decoupled_weight_decay=True)._plain() is False     # AdamW's arithmetic


def test_losses_keep_the_torch_formulation_on_the_cpu(monkeypatch):
    from refign_amd import flowloss, losses
    assert losses.FUSED_LEVEL_LOSS                       # the default; CPU tensors do not take the fused path all the same
    monkeypatch.setattr(flowloss, "multi_level_flow_loss", lambda *a, **k: pytest.fail("fused path on CPU tensors"))
    z = golden("matcher_losses_128x160")

    def run():
        first = [(torch.from_numpy(z[f"in/f{i}"]).requires_grad_(True), torch.from_numpy(z[f"in/uf{i}"]).requires_grad_(True))
                 for i in range(4)]
        mod = losses.MultiScaleFlowLoss(loss_type='HuberLoss', level_weights=[0.32, 0.08, 0.02, 0.01])
        val = mod(first, torch.from_numpy(z["flow_prime"]), mask=torch.from_numpy(z["mask_prime"]))
        val.backward()
        return val.detach(), [t.grad for pair in first for t in pair]
    on = run()
    assert abs(float(on[0]) - float(z["ss_loss"])) <= 1e-5 * abs(float(z["ss_loss"]))
    monkeypatch.setattr(losses, "FUSED_LEVEL_LOSS", False)
    off = run()
    assert torch.equal(on[0], off[0]) and all(torch.equal(a, b) for a, b in zip(on[1], off[1]))
    # the empty mask is still a zero, and one_scale / probabilistic_one_scale are what they were
    gt, est = torch.randn(2, 2, 16, 20), torch.randn(2, 2, 4, 5)
    mod = losses.MultiScaleFlowLoss()
    assert float(mod([est], gt, mask=torch.zeros(2, 16, 20, dtype=torch.bool))) == 0.0
    assert torch.equal(mod.one_scale(est, gt), mod([est], gt))


def test_device_loss_weights_equal_the_host_rule():
    """AlignmentModel.device_weights: the balancing as tensor arithmetic, the reference's argument-position quirk included."""
    from refign_amd.alignment_model import AlignmentModel
    host, devw = AlignmentModel.weights_selfsupervised_and_unsupervised, AlignmentModel.device_weights
    z = golden("matcher_step_128x160")
    cases = [(float(z["ss_loss"]), float(z["us_loss"])), (2.0, 4.0), (4.0, 2.0), (1.0, 1e-9), (-3.0, 2.0), (2.0, -3.0), (1.5, 1.5)]
    for ss, us in cases:
        for args in ((False,), (), (True,), (1.0, 2.0)):
            a, b = torch.tensor(ss), torch.tensor(us)
            want = host(a, b, *args)
            got = devw(a, b, *args)
            assert (float(got[0]), float(got[1])) == (float(want[0]), float(want[1])), (ss, us, args)


STAGE2_TRAINER_YAML = """
trainer:
  max_steps: 225000
  sync_batchnorm: True
  check_val_every_n_epoch: 225000
  logger:
    class_path: pytorch_lightning.loggers.TensorBoardLogger
    init_args:
      save_dir: lightning_logs
      name: uawarpc_megadepth_stage2
  callbacks:
    - class_path: pytorch_lightning.callbacks.LearningRateMonitor
    - class_path: pytorch_lightning.callbacks.ModelCheckpoint
      init_args:
        save_last: True
    - class_path: helpers.callbacks.ValEveryNSteps
      init_args:
        every_n_steps: 5000
"""


def test_trainer_kwargs_of_the_stage2_config():
    from refign_amd import config
    got = config.trainer_kwargs(yaml.safe_load(STAGE2_TRAINER_YAML))
    assert got["max_steps"] == 225000 and got["val_every_n_steps"] == 5000
    assert got["save_last"] is True and got["sync_batchnorm"] is True
    assert got["precision"] is None                      # the recipe's `--trainer.precision 16` comes from the command line
    assert config.trainer_logging(yaml.safe_load(STAGE2_TRAINER_YAML))["log_lr"] is True


def test_alignment_model_declares_automatic_optimization():
    from refign_amd.alignment_model import AlignmentModel
    m = AlignmentModel(alignment_backbone=torch.nn.Conv2d(1, 1, 1), alignment_head=torch.nn.Conv2d(1, 1, 1))
    assert m.automatic_optimization is True and m.global_step == 0
    assert m.optimizers() is None and m.lr_schedulers() is None
    assert "global_step" not in m.state_dict()

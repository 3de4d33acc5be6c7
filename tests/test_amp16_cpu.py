"""CPU: Trainer(precision=...) accepts the reference's precision values and rejects everything else; the loss scaler's
arguments and its GradScaler-format state (no kernels run here)."""
import pytest
import torch


@pytest.mark.parametrize("value,want", [(None, None), (16, "16"), ("16", "16"), ("16-mixed", "16"), ("bf16", "bf16"),
                                        ("bf16-mixed", "bf16"), (32, "32")])
def test_precision_values_accepted(value, want):
    from refign_amd.amp import parse_precision
    assert parse_precision(value) == want


@pytest.mark.parametrize("value", [8, 64, "fp16", "bf16-true", "16-true", True, 16.5, "mixed", [16]])
def test_trainer_rejects_other_precisions(value):
    from refign_amd.trainer import Trainer
    with pytest.raises(ValueError, match="precision"):
        Trainer(object(), precision=value)


def test_scaler_args_need_fp16():
    from refign_amd.trainer import Trainer
    with pytest.raises(ValueError, match="scaler_args"):
        Trainer(object(), precision="bf16", scaler_args={"init_scale": 1024.0})


def test_loss_scaler_arguments_and_state_dict_format():
    from refign_amd.amp import LossScaler
    for bad in (dict(growth_factor=1.0), dict(backoff_factor=1.5), dict(growth_interval=0), dict(init_scale=0.0)):
        with pytest.raises(ValueError):
            LossScaler("cpu", **bad)
    s = LossScaler("cpu", init_scale=1024.0, growth_interval=3)
    want = torch.amp.GradScaler("cpu", init_scale=1024.0, growth_interval=3).state_dict()
    assert s.state_dict() == want
    s.load_state_dict({"scale": 8.0, "growth_factor": 4.0, "backoff_factor": 0.25, "growth_interval": 7, "_growth_tracker": 2})
    assert s.state_dict() == {"scale": 8.0, "growth_factor": 4.0, "backoff_factor": 0.25, "growth_interval": 7,
                              "_growth_tracker": 2}
    with pytest.raises(RuntimeError):
        s.load_state_dict({})

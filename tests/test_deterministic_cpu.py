"""CPU: the switch of the deterministic mode -- the library's process-wide flag and its two entry points, the
`refign_amd.determinism` module on top of it, the YAML helper, Trainer's argument checking.  No kernel runs here."""
import ctypes
import os

import pytest
import torch
import yaml
from conftest import ROOT


def test_library_exports_the_flag_and_it_round_trips():
    import refign_amd
    from refign_amd import _lib
    raw = ctypes.CDLL(refign_amd.library_path())
    assert hasattr(raw, "rfn_set_deterministic") and hasattr(raw, "rfn_get_deterministic")
    header = open(os.path.join(ROOT, "include", "refign_hip.h")).read()
    assert "#define RFN_ENONDET (-4)" in header and "#define RFN_ABI_VERSION 5" in header
    lib = _lib.load_library()
    assert lib.rfn_get_deterministic() == 0
    try:
        assert lib.rfn_set_deterministic(1) == 0 and lib.rfn_get_deterministic() == 1
        assert lib.rfn_set_deterministic(7) == 0 and lib.rfn_get_deterministic() == 1      # any non-zero value is "on"
    finally:
        assert lib.rfn_set_deterministic(0) == 0
    assert lib.rfn_get_deterministic() == 0
    assert refign_amd.abi_version() == 5


def test_every_deterministic_entry_point_is_bound():
    from refign_amd import _lib
    lib = _lib.load_library()
    for name in ("rfn_bn_stats_fwd_det", "rfn_bn_stats_bwd_det", "rfn_bn_stats_det_workspace_bytes",
                 "rfn_dwconv3x3_nhwc_fwd_stats_det", "rfn_dwconv3x3_nhwc_stats_det", "rfn_dwconv3x3_stats_det_workspace_bytes",
                 "rfn_attn_bwd_dkv_det", "rfn_dacs_mix_jitter_det", "rfn_dacs_mix_jitter_det_workspace_bytes",
                 "rfn_upsample_ce_det", "rfn_upsample_ce_det_workspace_bytes", "rfn_upsample_bilinear2d_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the workspace sizes are host arithmetic: partial rows x 2 C sums (statistics), tiles x (loss + C x 10 x 10 footprint)
    assert lib.rfn_bn_stats_det_workspace_bytes(1 << 20, 256) == 512 * 2 * 256 * 8           # 512 workgroup rows, one channel block
    assert lib.rfn_bn_stats_det_workspace_bytes(1 << 20, 1024) == 256 * 2 * 1024 * 8         # two channel blocks of 512
    assert lib.rfn_bn_stats_det_workspace_bytes(64, 64) == 1 * 2 * 64 * 8
    assert lib.rfn_bn_stats_det_workspace_bytes(0, 64) == 0 and lib.rfn_bn_stats_det_workspace_bytes(64, 12) == 0
    tiles = 2 * (512 // 16) * (1024 // 16)
    assert lib.rfn_upsample_ce_det_workspace_bytes(2, 19, 512, 1024) == tiles * 8 + tiles * 19 * 100 * 4
    assert lib.rfn_dacs_mix_jitter_det_workspace_bytes(128, 128) == 8 * 8 * (1 + 16)


def test_refusal_code_reaches_python_as_runtime_error():
    """An atomic-form launcher refuses before it touches its (here: bogus but non-null) pointers or the device."""
    from refign_amd import _lib, determinism
    lib = _lib.load_library()
    one = ctypes.c_void_p(16)
    with determinism.deterministic():
        rc = lib.rfn_bn_stats_fwd(one, one, 64, 64, 1, None)
        assert rc == -4
        with pytest.raises(RuntimeError, match="rfn_bn_stats_fwd refused in deterministic mode.*bn_stats_kernel"):
            _lib.check(rc, "bn_stats_fwd")
        assert lib.rfn_warp_bwd_f32(one, one, one, one, one, 1, 1, 4, 4, None) == -4
        assert lib.rfn_upsample_ce(one, one, None, one, one, 1, 19, 4, 4, 8, 8, 255, 0, 0, None) == -4
        # accumulate = 1 (atomics) refuses, an unknown value is a plain argument error
        assert lib.rfn_gemm_tn(one, one, one, 64, 64, 64, 64, 64, 32, 1, None, None, 0, 1, None) == -4
        assert lib.rfn_gemm_tn(one, one, one, 64, 64, 64, 64, 64, 32, 3, None, None, 0, 1, None) == -1
    assert lib.rfn_get_deterministic() == 0


def test_context_manager_nests_and_restores():
    from refign_amd import _lib, determinism
    lib = _lib.load_library()
    assert not determinism.enabled()
    with determinism.deterministic():
        assert determinism.enabled() and lib.rfn_get_deterministic() == 1
        with determinism.deterministic(False):
            assert not determinism.enabled() and lib.rfn_get_deterministic() == 0
            with determinism.deterministic():
                assert determinism.enabled()
            assert not determinism.enabled()
        assert determinism.enabled() and lib.rfn_get_deterministic() == 1
    assert not determinism.enabled() and lib.rfn_get_deterministic() == 0
    with pytest.raises(KeyError):
        with determinism.deterministic():
            raise KeyError("x")
    assert not determinism.enabled() and lib.rfn_get_deterministic() == 0
    # holders (trainers): on until the last one lets go
    determinism.acquire()
    determinism.acquire()
    determinism.release()
    assert determinism.enabled() and lib.rfn_get_deterministic() == 1
    determinism.release()
    assert not determinism.enabled() and lib.rfn_get_deterministic() == 0
    # a holder that lets go inside a block leaves the block's mode alone; a block can switch a holder's mode off
    with determinism.deterministic():
        determinism.acquire()
        determinism.release()
        assert determinism.enabled() and lib.rfn_get_deterministic() == 1
    assert not determinism.enabled()
    determinism.acquire()
    with determinism.deterministic(False):
        assert not determinism.enabled() and lib.rfn_get_deterministic() == 0
    assert determinism.enabled() and lib.rfn_get_deterministic() == 1
    determinism.release()
    assert not determinism.enabled() and lib.rfn_get_deterministic() == 0


def test_torch_side_is_set_for_the_span_and_restored():
    from refign_amd import determinism
    before = (torch.are_deterministic_algorithms_enabled(), torch.backends.cudnn.deterministic,
              torch.utils.deterministic.fill_uninitialized_memory)
    with determinism.torch_deterministic(True):
        assert torch.are_deterministic_algorithms_enabled() and torch.backends.cudnn.deterministic
        assert torch.utils.deterministic.fill_uninitialized_memory is False
    assert (torch.are_deterministic_algorithms_enabled(), torch.backends.cudnn.deterministic,
            torch.utils.deterministic.fill_uninitialized_memory) == before
    with determinism.torch_deterministic(False):
        assert torch.are_deterministic_algorithms_enabled() == before[0]
    with determinism.torch_deterministic(True):
        with determinism.torch_switch_suspended():
            assert not torch.are_deterministic_algorithms_enabled()
        assert torch.are_deterministic_algorithms_enabled()
    with determinism.torch_switch_suspended():
        assert not torch.are_deterministic_algorithms_enabled()
    assert torch.are_deterministic_algorithms_enabled() == before[0]


def test_yaml_helper_and_trainer_kwargs_keep_apart():
    from refign_amd import config
    cfg = yaml.safe_load("seed_everything: 0\ntrainer:\n  max_steps: 100\n  deterministic: true\n  precision: 16\n")
    assert config.trainer_deterministic(cfg) is True
    assert config.trainer_deterministic(yaml.safe_load("trainer:\n  deterministic: warn\n")) is True
    assert config.trainer_deterministic(yaml.safe_load("trainer:\n  deterministic: false\n")) is False
    assert config.trainer_deterministic(yaml.safe_load("trainer:\n  max_steps: 1\n")) is False
    assert config.trainer_deterministic({}) is False and config.trainer_deterministic(None) is False
    assert config.trainer_kwargs(cfg) == {"max_steps": 100, "val_every_n_steps": None, "save_last": False,
                                          "sync_batchnorm": False, "precision": 16}


def test_trainer_refuses_precision_32_and_releases_the_flag():
    from test_resume_cpu import _trainer
    from refign_amd import _lib, determinism
    lib = _lib.load_library()
    with pytest.raises(ValueError, match="deterministic=True is not available with precision=32"):
        _trainer(32, deterministic=True)
    assert lib.rfn_get_deterministic() == 0
    a = _trainer(None, deterministic=True)
    assert a.deterministic and determinism.enabled() and lib.rfn_get_deterministic() == 1
    b = _trainer("bf16", deterministic=True)
    a.close()
    assert lib.rfn_get_deterministic() == 1, "a second deterministic trainer is still open"
    a.close()                                                    # closing twice releases once
    assert lib.rfn_get_deterministic() == 1
    b.close()
    assert not determinism.enabled() and lib.rfn_get_deterministic() == 0
    c = _trainer()
    assert not c.deterministic and lib.rfn_get_deterministic() == 0
    c.close()

"""CPU: the host half of the matcher's warp supervision (refign_amd/flowsynth.py, refign_amd/config.py).  Under the fixtures'
seeds draw_composite reproduces what the reference's CompositeFlow drew (tests/golden/flowsynth_*.npz, recorded by
tests/golden/make_golden_flowsynth.py at the reference's own calls): integers and the tails of both random streams exactly,
floats within 1 ulp of fp32; config.warp_supervision_plan on the reference's two MegaDepth configs; the library's new entry
points."""
import os
import random

import numpy as np
import pytest
import torch
from conftest import golden
from make_golden_flowsynth import AMPLITUDES, BATCH_INCLUDE, CASES, CROP, H, KINDS, W, crop_origin

REF_CONFIGS = "/root/reference/configs"
needs_reference = pytest.mark.skipif(not os.path.isdir(REF_CONFIGS), reason="the reference checkout is absent")


def ulp_close(got, want):
    """|got - want| <= 1 ulp of fp32 at `want`, element by element"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert got.shape == want.shape and (np.abs(got - want) <= ulp).all(), (got, want)


def check_sample(p, z, prefix=""):
    g = lambda k: z[prefix + k]  # noqa: E731
    assert p.transform_index == int(g("transform")) and KINDS.index(p.kind) == int(g("kind"))
    ulp_close(p.theta39.numpy(), g("theta39"))
    if prefix + "field" in z:
        e = p.elastic
        assert e["n_perturbations"] == int(g("n_perturbations"))
        np.testing.assert_array_equal(np.array(e["drawn"], np.int64).reshape(-1, 3), g("drawn"))
        ulp_close(e["sigma"], g("sigma"))
        ulp_close(e["alpha"], g("alpha"))
        ulp_close(np.array(e["bumps"], np.float64).reshape(-1, 4), g("bumps"))
        assert tuple(e["noise"].shape) == (2, H, W) and e["noise"].dtype == torch.float32
    else:
        assert p.elastic is None


def check_tails(z):
    np.testing.assert_array_equal(np.array([random.random() for _ in range(4)]), z["random_tail"])
    np.testing.assert_array_equal(torch.rand(4).numpy(), z["torch_tail"])


@pytest.mark.parametrize("case", list(CASES))
def test_draw_composite_reproduces_the_reference(case):
    from refign_amd import flowsynth
    z = golden("flowsynth_" + case)
    include, add_elastic = CASES[case]
    assert [str(v) for v in z["include"]] == include and bool(z["add_elastic"]) == add_elastic
    random.seed(int(z["seed"]))
    torch.manual_seed(int(z["seed"]))
    p = flowsynth.draw_composite(H, W, include_transforms=include, add_elastic=add_elastic, **AMPLITUDES)
    check_sample(p, z)
    check_tails(z)


def test_draw_composite_two_samples_in_a_row():
    from refign_amd import flowsynth
    z = golden("flowsynth_batch")
    random.seed(int(z["seed"]))
    torch.manual_seed(int(z["seed"]))
    ps = [flowsynth.draw_composite(H, W, include_transforms=BATCH_INCLUDE, **AMPLITUDES) for _ in range(2)]
    assert {p.kind for p in ps} == {"hom", "afftps"}
    for i, p in enumerate(ps):
        check_sample(p, z, f"s{i}_")
    check_tails(z)


def test_arguments():
    from refign_amd import flowsynth
    with pytest.raises(ValueError, match="parameterize_with_gaussian"):
        flowsynth.draw_composite(H, W, parameterize_with_gaussian=True)
    with pytest.raises(ValueError, match="rotate"):
        flowsynth.draw_composite(H, W, include_transforms=["rotate"])
    with pytest.raises(ValueError, match="theta"):
        flowsynth.params_from("afftps", H, W, theta_aff=[[1, 0, 0], [0, 1, 0]])
    p = flowsynth.params_from("affine", H, W, theta_aff=[[1, 0, 0.5], [0, 1, 0]], field=np.zeros((2, H, W), np.float32),
                              bumps=[(100.0, 120.0, 20.0, 250.0)])
    assert p.theta39[33:].tolist() == [1, 0, 0.5, 0, 1, 0] and p.elastic["bumps"] == [(100.0, 120.0, 20.0, 250.0)]
    # Python's rounding at the half: (248 - 203) / 2 = 22.5 -> 22
    assert flowsynth.crop_origin(H, W, *CROP) == crop_origin() == (22, 24)
    taps = flowsynth.gaussian_taps(9.0)
    assert taps.size == 73 and taps.dtype == np.float32 and abs(float(taps.astype(np.float64).sum()) - 1.0) < 1e-6
    assert flowsynth.gaussian_taps(135.0).size == 1081


def test_bump_scale_keeps_the_quirk():
    """x is drawn against the width and applied to the rows: a bump whose x lies far below the frame's last row peaks outside
    it, its maximum drops, the scale grows -- and below 1e-6 the reference skips it"""
    from refign_amd import flowsynth
    inside = flowsynth.bump_scale(100, 400, 50, 200, 10)
    outside = flowsynth.bump_scale(100, 400, 130, 200, 10)
    assert inside is not None and outside is not None and outside > 50 * inside
    assert flowsynth.bump_scale(100, 400, 370, 200, 10) is None


@needs_reference
@pytest.mark.parametrize("stage,t_hom,t_afftps,elastic", [("stage1", 0.333, 0.08, False), ("stage2", 0.4, 0.26, True)])
def test_warp_supervision_plan_reads_the_megadepth_configs(stage, t_hom, t_afftps, elastic):
    from refign_amd import config
    cfg = config.load_config(os.path.join(REF_CONFIGS, "megadepth", f"uawarpc_{stage}.yaml"))
    plan = config.warp_supervision_plan(cfg)
    assert plan == {"composite": {"include_transforms": ["hom", "tps", "afftps"], "random_alpha": 0.26, "random_s": 0.45,
                                  "random_tx": 0.25, "random_ty": 0.25, "random_t_hom": t_hom, "random_t_tps": t_hom,
                                  "random_t_tps_for_afftps": t_afftps, "add_elastic": elastic,
                                  "parameterize_with_gaussian": False},
                    "crop": (520, 520), "min_fraction_valid_corr": 0.1}
    if stage == "stage2":
        assert {k: plan["composite"][k] for k in AMPLITUDES} == AMPLITUDES
    with pytest.raises(config.OutOfScopeError):                   # the ingest plan keeps refusing this section
        config.ingest_plan(cfg, "train", "MegaDepth")


def test_warp_supervision_plan_refuses_what_it_cannot_carry():
    from refign_amd import config
    T = "data_modules.transforms."

    def cfg(transforms):
        return {"data": {"init_args": {"load_config": {"train": {"MegaDepth": {"transforms": transforms}}}}}}
    ok = {"class_path": T + "CompositeFlow", "init_args": {"apply_keys": ["image_prime"], "include_transforms": ["hom"]}}
    plan = config.warp_supervision_plan(cfg([ok]))
    assert plan["crop"] is None and plan["composite"]["include_transforms"] == ["hom"] and plan["composite"]["random_s"] == 0.6
    with pytest.raises(config.OutOfScopeError, match="CompositeFlow"):
        config.warp_supervision_plan(cfg([{"class_path": T + "ToTensor"}]))
    with pytest.raises(config.OutOfScopeError, match="parameterize_with_gaussian"):
        config.warp_supervision_plan(cfg([{**ok, "init_args": {**ok["init_args"], "parameterize_with_gaussian": True}}]))
    with pytest.raises(config.OutOfScopeError, match="apply_keys"):
        config.warp_supervision_plan(cfg([{**ok, "init_args": {"apply_keys": "all"}}]))
    with pytest.raises(config.OutOfScopeError, match="rotate"):
        config.warp_supervision_plan(cfg([{**ok, "init_args": {**ok["init_args"], "include_transforms": ["rotate"]}}]))
    with pytest.raises(config.OutOfScopeError, match="CenterCrop"):
        config.warp_supervision_plan(cfg([{"class_path": T + "CenterCrop", "init_args": {"size": [8, 8]}}, ok]))
    with pytest.raises(KeyError):
        config.warp_supervision_plan(cfg([ok]), "val")


def test_header_declares_the_entry_points():
    from refign_amd import _lib
    c = _lib.c_void_p
    import ctypes
    i, d = ctypes.c_int, ctypes.c_double
    assert _lib.ABI_VERSION == 5
    assert _lib.SIGNATURES["rfn_flowsynth_flow_f32"] == (i, [c, i, c, i, c, i, i, c, c, c])
    assert _lib.SIGNATURES["rfn_flowsynth_warp_f32"] == (i, [c, c, c, i, i, i, i, i, i, d, c, c, c, c])
    assert _lib.SIGNATURES["rfn_gaussian_blur_f32"] == (i, [c, c, i, i, i, i, c, c, c])
    lib = os.path.join(os.path.dirname(_lib.__file__), "lib", "librefign_hip.so")
    if os.path.exists(lib):                                       # built: the library exports what the header declares
        with open(lib, "rb") as f:
            blob = f.read()
        for name in ("rfn_flowsynth_flow_f32", "rfn_flowsynth_warp_f32", "rfn_gaussian_blur_f32"):
            assert name.encode() in blob

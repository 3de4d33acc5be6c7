"""CPU: the host half of the photometric chain on image_prime (refign_amd/photometric.py, config.photometric_plan).
photometric.draw makes the pipeline's draws -- ColorJitter, ChannelShuffle, RandomGaussianBlur -- with the calls and in the
order of the reference, so both random streams stand afterwards where the reference leaves them: checked against the calls made
by hand, and against tests/golden/photometric_draws.npz (recorded by tests/golden/make_golden_photometric.py from the
reference's own classes over stand-in torchvision bases); config.photometric_plan on the reference's two MegaDepth sections
(embedded, and from the YAML where the checkout exists) and every refusal it documents; the header's new entry points."""
import copy
import ctypes
import os
import random

import numpy as np
import pytest
import torch
from conftest import golden

REF_CONFIGS = "/root/reference/configs"
needs_reference = pytest.mark.skipif(not os.path.isdir(REF_CONFIGS), reason="the reference checkout is absent")
T = "data_modules.transforms."
IMNET = {"mean": (0.485, 0.456, 0.406), "std": (0.229, 0.224, 0.225)}


def f32_bits(v):
    return np.float32(v).view(np.int32).item()


def plan_of(brightness=(0.4, 1.6), contrast=(0.4, 1.6), saturation=(0.4, 1.6), p=0.2, shuffle=True):
    blur = None if p is None else {"p": p, "kernel_size": 7, "sigma": (0.2, 2.0)}
    return {"brightness": brightness, "contrast": contrast, "saturation": saturation, "shuffle": shuffle, "blur": blur, **IMNET}


def by_hand(plan):
    """the listed torch / random calls of one sample"""
    order = torch.randperm(4).tolist()
    factors = []
    for k in ("brightness", "contrast", "saturation"):
        factors.append(None if plan[k] is None else float(torch.empty(1).uniform_(plan[k][0], plan[k][1])))
    perm = [0, 1, 2]
    random.shuffle(perm)
    coin = random.random()
    sigma = torch.empty(1).uniform_(*plan["blur"]["sigma"]).item() if coin < plan["blur"]["p"] else None
    return order, factors, perm, coin, sigma


@pytest.mark.parametrize("name,plan", [("blur certain", plan_of(p=1.0)), ("blur never", plan_of(p=0.0)),
                                       ("no contrast", plan_of(contrast=None, p=0.5))])
@pytest.mark.parametrize("seed", [0, 11])
def test_draw_makes_the_reference_calls_in_order(name, plan, seed):
    from refign_amd import photometric
    random.seed(seed)
    torch.manual_seed(seed)
    got = [photometric.draw(plan) for _ in range(3)]
    tails = (torch.rand(1).item(), random.random())
    random.seed(seed)
    torch.manual_seed(seed)
    want = [by_hand(plan) for _ in range(3)]
    assert tails == (torch.rand(1).item(), random.random())
    for p, (order, factors, perm, coin, sigma) in zip(got, want):
        assert p.order == order and p.perm == perm and p.coin == coin
        assert [None if f is None else f32_bits(f) for f in p.factors] == [None if f is None else f32_bits(f) for f in factors]
        assert p.sigma == sigma and (p.kernel is None) == (sigma is None)
        if name == "blur certain":
            assert p.sigma is not None and 0.2 <= p.sigma <= 2.0
        if name == "blur never":
            assert p.sigma is None
        if name == "no contrast":
            assert p.contrast is None and p.record()[5] == 0


def test_draw_reproduces_the_reference_classes():
    """the golden: the reference's ColorJitter -> ChannelShuffle -> RandomGaussianBlur, two samples in a row per seed"""
    from refign_amd import photometric
    z = golden("photometric_draws")
    rng = lambda v: (max(0.0, 1.0 - float(v)), 1.0 + float(v))  # noqa: E731
    plan = {"brightness": rng(z["brightness"]), "contrast": rng(z["contrast"]), "saturation": rng(z["saturation"]),
            "shuffle": True, "blur": {"p": float(z["p"]), "kernel_size": int(z["kernel_size"]),
                                      "sigma": tuple(float(v) for v in z["sigma_range"])}, **IMNET}
    ramp = np.arange(12, dtype=np.uint8).reshape(3, 2, 2)
    blurred = 0
    for i, seed in enumerate(z["seeds"].tolist()):
        random.seed(seed)
        torch.manual_seed(seed)
        for j in range(z["order"].shape[1]):
            p = photometric.draw(plan)
            assert p.order == z["order"][i, j].tolist()
            assert [f32_bits(f) for f in p.factors] == [f32_bits(f) for f in z["factors"][i, j]]
            np.testing.assert_array_equal(ramp[p.perm], z["shuffled"][i, j])
            assert p.coin == float(z["coin"][i, j])
            if np.isnan(z["sigma"][i, j]):
                assert p.sigma is None and not p.coin < plan["blur"]["p"]
            else:
                assert p.sigma == float(z["sigma"][i, j])
                blurred += 1
        np.testing.assert_array_equal(np.array([random.random() for _ in range(4)]), z["random_tail"][i])
        np.testing.assert_array_equal(torch.rand(4).numpy(), z["torch_tail"][i])
    assert 0 < blurred < z["coin"].size


def test_record_and_kernel():
    from refign_amd import photometric
    p = photometric.params_from([2, 0, 3, 1], 0.4, None, 1.6, [2, 0, 1], 0.7, mean=(0.1, 0.2, 0.3), std=(1.0, 2.0, 4.0))
    rec = p.record()
    flt = rec.view(np.float32)
    assert rec.dtype == np.int32 and rec.size == photometric.RECORD_WORDS == 80
    assert rec[0:4].tolist() == [2, 0, 3, 1] and rec[4:8].tolist() == [1, 0, 1, 0]
    assert flt[8] == np.float32(0.4) and flt[11] == np.float32(1.0 - 0.4) and flt[10] == np.float32(1.6)
    assert flt[13] == np.float32(1.0 - 1.6) and flt[9] == 0 and flt[12] == 0
    assert rec[14:17].tolist() == [2, 0, 1] and rec[17] == 1 and rec[73:].tolist() == [0] * 7
    assert flt[18:24].tolist() == [np.float32(v) for v in (0.1, 0.2, 0.3, 1.0, 2.0, 4.0)]
    # the weights: the formula of the kernel construction, each call fp32 on the CPU
    k1 = torch.exp(-0.5 * (torch.linspace(-3, 3, 7) / 0.7) ** 2)
    k1 = k1 / k1.sum()
    K = k1[:, None] @ k1[None, :]
    assert torch.equal(torch.from_numpy(flt[24:73].copy()).reshape(7, 7), K) and abs(float(K.double().sum()) - 1.0) < 1e-6
    # a smaller kernel sits centred in zeros
    k3 = photometric.blur_kernel(1.0, 3)
    assert float(k3[2:5, 2:5].double().sum()) == pytest.approx(1.0, abs=1e-6) and int((k3 != 0).sum()) == 9
    assert photometric.params_from([0, 1, 2, 3], None, None, None, [0, 1, 2], None).record()[17] == 0
    for bad in (dict(order=[0, 1, 2, 2]), dict(perm=[0, 0, 1]), dict(kernel_size=4), dict(kernel_size=9), dict(sigma=0.0)):
        kw = dict(order=[0, 1, 2, 3], brightness=1.0, contrast=1.0, saturation=1.0, perm=[0, 1, 2], sigma=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            photometric.params_from(**kw)


def test_apply_refuses_a_cpu_tensor():
    from refign_amd import photometric
    p = photometric.params_from([0, 1, 2, 3], 1.0, 1.0, 1.0, [0, 1, 2], None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        photometric.apply(torch.zeros(3, 8, 8, dtype=torch.uint8), p)


# ---- config.photometric_plan --------------------------------------------------------------------------------------------------
def chain(p=0.2, sigma=(0.2, 2.0)):
    keys = {"apply_keys": ["image_prime"]}
    return [{"class_path": T + "ToTensor"},
            {"class_path": T + "ColorJitter", "init_args": {**keys, "brightness": 0.6, "contrast": 0.6, "saturation": 0.6, "hue": 0}},
            {"class_path": T + "ChannelShuffle", "init_args": dict(keys)},
            {"class_path": T + "RandomGaussianBlur", "init_args": {**keys, "p": p, "kernel_size": 7, "sigma": list(sigma)}},
            {"class_path": T + "ConvertImageDtype"}, {"class_path": T + "Normalize"},
            {"class_path": T + "CompositeFlow", "init_args": {**keys, "include_transforms": ["hom", "tps", "afftps"]}},
            {"class_path": T + "CenterCrop", "init_args": {"size": [520, 520]}}]


def cfg_of(transforms, dataset="MegaDepth"):
    return {"data": {"init_args": {"load_config": {"train": {dataset: {"dims": [750, 750], "transforms": transforms}}}}}}


STAGE_PLAN = {"brightness": (1.0 - 0.6, 1.6), "contrast": (1.0 - 0.6, 1.6), "saturation": (1.0 - 0.6, 1.6), "shuffle": True,
              "blur": {"p": 0.2, "kernel_size": 7, "sigma": (0.2, 2.0)}, **IMNET}


def test_photometric_plan_of_the_stage_sections():
    """both stages' sections carry the same chain (they differ in CompositeFlow's amplitudes)"""
    from refign_amd import config
    cfg = cfg_of(chain())
    assert config.photometric_plan(cfg) == STAGE_PLAN
    assert config.photometric_plan(cfg, "train", "MegaDepth") == STAGE_PLAN
    with pytest.raises(config.OutOfScopeError, match="ColorJitter"):      # the ingest plan keeps refusing the section
        config.ingest_plan(cfg, "train", "MegaDepth")
    assert config.warp_supervision_plan(cfg)["crop"] == (520, 520)        # and the geometric half reads it as before
    with pytest.raises(KeyError):
        config.photometric_plan(cfg, "val")


@needs_reference
@pytest.mark.parametrize("stage", ["stage1", "stage2"])
def test_photometric_plan_reads_the_megadepth_configs(stage):
    from refign_amd import config
    cfg = config.load_config(os.path.join(REF_CONFIGS, "megadepth", f"uawarpc_{stage}.yaml"))
    assert config.photometric_plan(cfg) == STAGE_PLAN
    with pytest.raises(config.OutOfScopeError, match="ColorJitter"):
        config.ingest_plan(cfg, "train", "MegaDepth")
    with pytest.raises(config.OutOfScopeError, match="ColorJitter"):      # the val section has no chain
        config.photometric_plan(cfg, "val")


ROBOTCAR = [{"class_path": T + "RandomRotation", "init_args": {"degrees": 10}}, {"class_path": T + "ToTensor"},
            {"class_path": T + "RandomCrop", "init_args": {"size": [512, 512]}, "cat_max_ratio": 0.75},     # (as the file indents it)
            {"class_path": T + "ColorJitter", "init_args": {"brightness": 0.25, "contrast": 0.25, "saturation": 0.25, "hue": 0.1}},
            {"class_path": T + "RandomHorizontalFlip"}, {"class_path": T + "ConvertImageDtype"}, {"class_path": T + "Normalize"}]


def test_photometric_plan_refuses_the_robotcar_hue():
    from refign_amd import config
    with pytest.raises(config.OutOfScopeError, match="hue"):
        config.photometric_plan(cfg_of(ROBOTCAR, "RobotCar"), "train", "RobotCar")
    path = os.path.join(REF_CONFIGS, "cityscapes_robotcar", "refign_daformer.yaml")
    if os.path.exists(path):
        cfg = config.load_config(path)
        sections = cfg["data"]["init_args"]["load_config"]["train"]["RobotCar"]
        assert sections[0]["transforms"] == ROBOTCAR
        with pytest.raises(config.OutOfScopeError, match="list of sections"):
            config.photometric_plan(cfg, "train", "RobotCar")
        with pytest.raises(config.OutOfScopeError, match="hue"):
            config.photometric_plan(cfg_of(sections[0]["transforms"], "RobotCar"), "train", "RobotCar")


def test_photometric_plan_refuses_what_it_cannot_carry():
    from refign_amd import config

    def changed(index, **args):
        t = copy.deepcopy(chain())
        t[index]["init_args"].update(args)
        return cfg_of(t)
    with pytest.raises(config.OutOfScopeError, match="hue"):
        config.photometric_plan(changed(1, hue=0.1))
    with pytest.raises(config.OutOfScopeError, match="hue"):
        config.photometric_plan(changed(1, hue=[-0.1, 0.1]))
    for index in (1, 2, 3):
        with pytest.raises(config.OutOfScopeError, match="apply_keys"):
            config.photometric_plan(changed(index, apply_keys=["image", "image_prime"]))
        with pytest.raises(config.OutOfScopeError, match="apply_keys"):
            config.photometric_plan(changed(index, apply_keys="all"))
    for ksize in (6, 9, [7, 5]):
        with pytest.raises(config.OutOfScopeError, match="kernel_size"):
            config.photometric_plan(changed(3, kernel_size=ksize))
    with pytest.raises(config.OutOfScopeError, match="order"):
        t = chain()
        config.photometric_plan(cfg_of([t[0], t[2], t[1]] + t[3:]))
    with pytest.raises(config.OutOfScopeError, match="order"):
        t = chain()
        config.photometric_plan(cfg_of([t[0], t[1], t[3], t[2]] + t[4:]))
    for index in (1, 2, 3):
        with pytest.raises(config.OutOfScopeError, match="ConvertImageDtype"):
            t = chain()
            moved = t.pop(index)
            t.insert(4, moved)                                   # now right behind ConvertImageDtype
            config.photometric_plan(cfg_of(t))
    with pytest.raises(config.OutOfScopeError, match="second"):
        t = chain()
        config.photometric_plan(cfg_of(t[:2] + [t[1]] + t[2:]))
    with pytest.raises(config.OutOfScopeError, match="ColorJitter"):
        t = chain()
        config.photometric_plan(cfg_of(t[:1] + t[2:]))
    with pytest.raises(config.OutOfScopeError, match="gamma"):
        config.photometric_plan(changed(1, gamma=0.5))
    # what it does carry: a smaller kernel, a section without shuffle or blur, a disabled step, explicit statistics
    assert config.photometric_plan(changed(3, kernel_size=3))["blur"]["kernel_size"] == 3
    t = chain()
    plan = config.photometric_plan(cfg_of(t[:2] + t[4:]))
    assert plan["shuffle"] is False and plan["blur"] is None and plan["brightness"] == STAGE_PLAN["brightness"]
    assert config.photometric_plan(changed(1, contrast=0))["contrast"] is None
    assert config.photometric_plan(changed(1, contrast=[0.5, 1.5]))["contrast"] == (0.5, 1.5)
    t = chain()
    t[5] = {"class_path": T + "Normalize", "init_args": {"mean": [0.5, 0.5, 0.5], "std": [0.25, 0.25, 0.25]}}
    plan = config.photometric_plan(cfg_of(t))
    assert plan["mean"] == (0.5, 0.5, 0.5) and plan["std"] == (0.25, 0.25, 0.25)


def test_header_declares_the_entry_points():
    from refign_amd import _lib
    c, i = _lib.c_void_p, ctypes.c_int
    assert _lib.ABI_VERSION == 5
    assert _lib.SIGNATURES["rfn_photometric_record_words"] == (i, [])
    assert _lib.SIGNATURES["rfn_photometric_gray_sums_u8"] == (i, [c, c, i, i, i, c, c])
    assert _lib.SIGNATURES["rfn_photometric_apply_u8"] == (i, [c, c, c, i, i, i, c, c])
    lib = os.path.join(os.path.dirname(_lib.__file__), "lib", "librefign_hip.so")
    if os.path.exists(lib):                                       # built: the library exports what the header declares
        with open(lib, "rb") as f:
            blob = f.read()
        for name in ("rfn_photometric_record_words", "rfn_photometric_gray_sums_u8", "rfn_photometric_apply_u8"):
            assert name.encode() in blob

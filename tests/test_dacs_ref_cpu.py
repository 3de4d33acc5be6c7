"""CPU: the fp64 reference of the DACS data step, the fp32 model of the kernels and the bound built on them (tests/dacs_ref.py).

test_dacs_gpu.py holds csrc/dacs.hip to `min(M E + 2^-23, 1e-5)`, E being the error of the fp32 model on the very input.  Before
anyone trusts that bound, this file shows that it has teeth: each defect such a kernel typically has (dacs_ref.FAULTS), injected
into the model, lands 10 x or more outside the bound on its designated cases.  It also runs the torch fallback of the data step
(uda.strong_transform / uda._gaussian_blur) with the same draws against the same reference within the same bound, so that both
routes through get_dacs_mix are pinned to one statement of the operators.  Every test prints its figures before it asserts."""
import itertools
import math

import numpy as np
import pytest
import torch

import dacs_ref as dr


def test_case_table():
    """The table holds what it is about: all 24 orders at both jitter shapes, factors and angles on both ends of their range,
    contrast at each position, the four blur windows, mixed switches, a full batch, and every fault's cases exist."""
    assert set(dr.ORDERS) == set(itertools.permutations(range(4))) and len(dr.ORDERS) == 24
    for h, w in dr.JITTER_SHAPES:
        seen, factors = set(), set()
        for third in range(3):
            c = dr.case(f"jitter-{h}x{w}-{third}")
            assert c.shape == (dr.MAX_BATCH, h, w) and (h * w) % 4 == 0
            for order, factor, hue in c.jitter:
                seen.add(tuple(order))
                factors.update(factor)
            even = dr.case(f"jitter-{h}x{w}-{third}-even")
            assert [j is None for j in even.jitter] == [n % 2 == 1 for n in range(8)]
            assert all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) for a, b in zip(even.jitter[::2], c.jitter[::2]))
            assert np.array_equal(even.src, c.src) and np.array_equal(even.gt, c.gt) and even.bits == c.bits
        assert seen == set(dr.ORDERS)
        assert min(factors) == float(np.float32(1 - dr.S)) and max(factors) == float(np.float32(1 + dr.S))
        assert any(min(factors) < f < max(factors) for f in factors)
    assert (18 * 22) % 4 == 0 and 22 % 4 != 0 and (40 * 72 // 4) % 256 != 0 and 40 * 72 // 4 > 512
    assert sorted(o.index(1) for o in dr.CONTRAST_ORDERS) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert all(o[0] == 0 or o[:2] == (1, 0) for o in dr.CONTRAST_ORDERS)
    assert [(dr.window(h), dr.window(w)) for h, w in dr.BLUR_SHAPES] == [(1, 1), (3, 7), (35, 3), (3, 69)]
    assert min(min(s) for s in dr.BLUR_SHAPES) == dr.BLUR_R + 1 and 35 > 2 * dr.BLUR_R + 1
    both = dr.case("both-40x72")
    assert {(j is not None, s is not None) for j, s in zip(both.jitter, both.sigma)} == {(a, b) for a in (0, 1) for b in (0, 1)}
    m = dr.case("mask-40x72")
    assert {(b >> 30) & 1 for b in m.bits} == {0, 1} and {(b >> 31) & 1 for b in m.bits} == {0, 1}
    assert set(np.unique(m.gt)) == set(dr.EDGE_LABELS)
    assert set(dr.FAULTS) == set(dr.FAULT_NAMES)
    for cases in dr.FAULTS.values():
        assert cases and all(c in dr.CASES for c in cases)
    assert 1.0 <= dr.M and math.log2(dr.M) == int(math.log2(dr.M))


def test_hue_angles_reach_both_ends():
    angles = set()
    for i in range(24):
        (order, factor, hue), draws = dr.order_jitter(i)
        angles.add(draws[list(order).index(3) + 1])
        # the matrix is the rotation it claims to be: luma row kept, angle 0 -> identity
        assert np.allclose(np.array([0.299, 0.587, 0.114]) @ hue.astype(np.float64), [0.299, 0.587, 0.114], atol=1e-6)
    assert {0.0, 1.0} < angles
    assert np.allclose(dr.make_jitter((0, 1, 2, 3), [0.5] * 4, 0.5)[0][2], np.eye(3), atol=1e-7)


def test_reference_blur_is_a_convolution_with_reflected_border():
    """reference()'s blur against fp64 torch conv2d on a reflect-padded image, window from the rule, taps over the whole window."""
    c = dr.case("blur-344x24-random")
    want = dr.case_reference("blur-344x24-random")[0]
    x = torch.from_numpy(dr.plain_mix(c)).double()
    H, W = c.shape[1:]
    for n, sigma in enumerate(c.sigma):
        if sigma is None:
            assert np.array_equal(want[n], x[n].numpy())
            continue
        ky, kx = (torch.from_numpy(dr.taps(dr.window(d), sigma, False)) for d in (H, W))
        assert len(ky) == 35 and len(kx) == 3 and abs(float(ky.sum()) - 1) < 1e-15
        y = torch.nn.functional.pad(x[n:n + 1], (len(kx) // 2, len(kx) // 2, len(ky) // 2, len(ky) // 2), mode="reflect")
        y = torch.nn.functional.conv2d(y, (ky[:, None] * kx[None, :]).expand(3, 1, -1, -1).contiguous(), groups=3)
        assert float((y[0] - torch.from_numpy(want[n])).abs().max()) <= 1e-14 * float(y.abs().max())


def test_builders():
    """Each builder has the property it is named for."""
    B, H, W = 3, 24, 28
    src, trg, gt, pseudo, pw, bits = dr.build_saturating(1, B, H, W)
    v01 = src * dr.STD32.reshape(3, 1, 1) + dr.MEAN32.reshape(3, 1, 1)
    assert 0.3 < float(((v01 + 0.2 >= 1) | (v01 + 0.2 <= 0)).mean()) < 0.5
    src, trg, *_ = dr.build_impulses(1, B, H, W)
    assert all(int((a != 0).sum()) == 9 * B for a in (src, trg))
    assert src[0, 0, 0, 0] != 0 and src[0, 0, H - 1, W - 1] != 0 and src[0, 0, 1, W - 2] != 0
    src, trg, *_ = dr.build_constant(1, B, H, W)
    assert np.array_equal(src, trg) and float((src.max((2, 3)) - src.min((2, 3))).max()) == 0
    c = dr.case("jitter-40x72-0")
    got = dr.case_reference("jitter-40x72-0")[0]
    r01 = got * dr.STD32.reshape(3, 1, 1) + dr.MEAN32.reshape(3, 1, 1)
    sat = float(((r01 < 1e-9) | (r01 > 1 - 1e-9)).mean())
    print(f"DACS_SAT jitter-40x72-0 share of outputs on a clamp {sat:.3f}")
    assert 0.0 < sat <= 0.2 and c.src.dtype == np.float32


@pytest.mark.parametrize("name", list(dr.CASES))
def test_model_is_rounding_noise(name):
    """model32 is a few float32 roundings from the reference: 4 E stays under the cap of 1e-5 (so the cap never is what binds),
    labels and weights are the reference's, and where nothing but the mix happens the model is the plain mix bit for bit."""
    c, ref, mod = dr.case(name), dr.case_reference(name), dr.case_model(name)
    E = dr.case_E(name)
    print(f"DACS_MODEL {name} E {E:.3e} bound {dr.bound(E):.3e} max|want| {float(np.abs(ref[0]).max()):.3f}")
    assert mod[0].dtype == np.float32 and ref[0].dtype == np.float64
    assert np.array_equal(mod[1], ref[1]) and np.array_equal(mod[2], ref[2]) and ref[2].dtype == np.float32
    assert dr.M * E <= dr.CAP
    plain = dr.plain_mix(c)
    for n in range(c.shape[0]):
        if c.jitter[n] is None and (c.sigma[n] is None or name.startswith("blur-17x20")):
            assert np.array_equal(mod[0][n], plain[n]) and np.array_equal(ref[0][n], plain[n].astype(np.float64))
    if name.endswith("constant"):
        assert dr.rel_err(ref[0], plain) <= 1e-15


def _fault_params():
    for fault, cases in dr.FAULTS.items():
        for name in cases:
            yield pytest.param(fault, name, id=f"{fault}-{name}")


@pytest.mark.parametrize("fault,name", list(_fault_params()))
def test_fault_is_outside_the_bound(fault, name):
    """A kernel with this defect fails the GPU test on this case: its error is 10 x the bound or more; a label fault also
    changes at least one label and one weight."""
    ref, bad = dr.case_reference(name), dr.case_model(name, fault)
    E = dr.case_E(name)
    err = dr.rel_err(bad[0], ref[0])
    print(f"DACS_FAULT {fault} {name} error {err:.3e} bound {dr.bound(E):.3e} factor {err / dr.bound(E):.1f}")
    assert err >= 10 * dr.bound(E)
    if fault in dr.LABEL_FAULTS:
        assert not np.array_equal(bad[1], ref[1]) and not np.array_equal(bad[2], ref[2])
    else:
        assert np.array_equal(bad[1], ref[1])


def test_label_30_and_255_are_what_the_label_faults_touch():
    m = dr.case("mask-40x72")
    good = dr.class_mask(m.gt, m.bits)
    for fault, label in (("mask_ignores_255", 255), ("class30_out_of_range", 30)):
        diff = good != dr.class_mask(m.gt, m.bits, fault)
        assert diff.any() and set(np.unique(m.gt[diff])) == {label}
    # labels outside the set are never taken, whatever the bits
    every = dr.class_mask(m.gt, (0xFFFFFFFF,) * 8)
    assert not every[np.isin(m.gt, (31, 40, 254, -1))].any() and every[np.isin(m.gt, (0, 5, 18, 30, 255))].all()


# ---------------------------------------------------------------------------------------------------------------------
# the torch fallback of the data step (refign_amd/uda.py) with the same draws
# ---------------------------------------------------------------------------------------------------------------------
UDA_CASES = dr.JITTER_CASES + ("contrast-40x72", "mask-40x72", "both-40x72") + dr.BLUR_CASES


def _uda_data_step(monkeypatch, c):
    from refign_amd import uda
    B, H, W = c.shape
    mask = torch.from_numpy(dr.class_mask(c.gt, c.bits)).long()
    src, trg, gt, pseudo, pw = (torch.from_numpy(a) for a in (c.src, c.trg, c.gt, c.pseudo, c.pweight))
    imgs, lbls, wgts = [], [], []
    for n in range(B):
        draws = iter(c.draws[n] or ())
        monkeypatch.setattr(torch, "randperm", lambda k, n=n: torch.tensor(c.jitter[n][0]))
        monkeypatch.setattr(torch, "rand", lambda size, draws=draws: torch.tensor(next(draws), dtype=torch.float64))
        monkeypatch.setattr(np.random, "uniform", lambda lo, hi, n=n: c.sigma[n])
        param = {"mix": mask[n][None, None], "color_jitter": 1.0 if c.jitter[n] is not None else 0.0, "color_jitter_p": 0.5,
                 "color_jitter_s": dr.S, "blur": 1.0 if c.sigma[n] is not None else 0.0}
        img, lbl = uda.strong_transform(param, data=torch.stack((src[n], trg[n])), target=torch.stack((gt[n], pseudo[n]))[:, None])
        _, w = uda.strong_transform(param, target=torch.stack((torch.ones_like(pw[n]), pw[n]))[:, None])
        assert next(draws, None) is None                               # every uniform of the case was asked for, in order
        imgs.append(img[0]), lbls.append(lbl[0, 0]), wgts.append(w[0, 0])
    return torch.stack(imgs).numpy(), torch.stack(lbls).numpy(), torch.stack(wgts).numpy()


@pytest.mark.parametrize("name", UDA_CASES)
def test_torch_fallback_meets_the_same_reference(monkeypatch, name):
    c, ref = dr.case(name), dr.case_reference(name)
    img, lbl, wgt = _uda_data_step(monkeypatch, c)
    E = dr.case_E(name)
    err = dr.rel_err(img, ref[0])
    print(f"DACS_UDA {name} torch {err:.3e} model {E:.3e} ratio {err / E if E > 0 else float('nan'):.2f} bound {dr.bound(E):.3e}")
    assert img.dtype == np.float32 and np.array_equal(lbl, ref[1]) and np.array_equal(wgt, ref[2])
    assert err <= dr.bound(E)

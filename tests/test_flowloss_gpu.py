"""GPU: the fused multi-level flow loss (csrc/flowloss.hip, refign_amd/flowloss.py) behind losses.MultiScaleFlowLoss and
losses.WBipathLoss -- against golden vectors captured from the reference (tests/golden/make_golden_matcher.py), against the
torch formulation on the same device, launch-to-launch repeatability, and no host synchronisation."""
import numpy as np
import pytest
import torch
from conftest import golden

pytestmark = pytest.mark.gpu

WEIGHTS = [0.32, 0.08, 0.02, 0.01]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def T(a, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


def _count_entry(monkeypatch, names):
    from refign_amd import _lib
    lib = _lib.load_library()
    calls = {}
    for name in names:
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    return calls


def _golden_levels(z, dev):
    first = [(T(z[f"in/f{i}"], dev, True), T(z[f"in/uf{i}"], dev, True)) for i in range(4)]
    second = [(T(z[f"in/s{i}"], dev, True), T(z[f"in/us{i}"], dev, True)) for i in range(4)]
    return first, second


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the reference (the bars of test_matcher_gpu.test_wbipath_loss_matches_reference)
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_losses_match_reference(dev, monkeypatch):
    from refign_amd import losses
    assert losses.FUSED_LEVEL_LOSS
    calls = _count_entry(monkeypatch, ["rfn_flowloss_fwd_f32", "rfn_flowloss_bwd_f32"])
    z = golden("matcher_losses_128x160")
    first, second = _golden_levels(z, dev)
    flow, mask = T(z["flow_prime"], dev), T(z["mask_prime"], dev)
    ss = losses.MultiScaleFlowLoss(loss_type='HuberLoss', level_weights=WEIGHTS)
    us = losses.WBipathLoss(objective='multi_scale_flow_loss', loss_type='HuberLoss', visibility_mask=True)
    l_ss = ss(first, flow, mask=mask)
    l_us, masks, cyc, comp = us(first, second, flow, mask_used=mask, return_masks=True)
    assert calls.get("rfn_flowloss_fwd_f32") == 2
    print(f"\nss {float(l_ss)!r} golden {float(z['ss_loss'])!r}; us {float(l_us)!r} golden {float(z['us_loss'])!r}")
    assert abs(float(l_ss) - float(z["ss_loss"])) <= 1e-5 * float(z["ss_loss"])
    assert abs(float(l_us) - float(z["us_loss"])) <= 1e-5 * float(z["us_loss"])
    (l_ss + l_us).backward()
    assert calls.get("rfn_flowloss_bwd_f32") == 2
    for i in range(4):
        assert (masks[i].cpu().numpy() != z[f"mask{i}"]).sum() <= 2
        assert (cyc[i].cpu().numpy() != z[f"cyclic{i}"]).sum() <= 2
        assert np.abs(comp[i][0].detach().cpu().numpy() - z[f"composed{i}"]).max() <= 1e-4
        for nm, x in (("f", first[i][0]), ("uf", first[i][1]), ("s", second[i][0]), ("us", second[i][1])):
            want = z[f"grad/{nm}{i}"]
            err = np.abs(x.grad.cpu().numpy() - want).max()
            assert err <= 1e-4 * max(np.abs(want).max(), 1e-6), (nm, i, err)


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the torch formulation on the same device
# ---------------------------------------------------------------------------------------------------------------------
H, W = 37, 53
SIZES = [(5, 7), (1, 1), (37, 53)]              # non-integer scale, a single pixel, no resize
DELTA = 1.0                                      # HuberLoss's default, what MultiScaleFlowLoss builds


def _case(dev, B, lvc, sizes, hw, seed):
    """Ground truth on a quarter-pixel lattice (so that gt + r - gt == r exactly where nothing is resized), estimates with
    residuals of exactly 0 and exactly +-delta planted on the level that is not resized."""
    g = torch.Generator().manual_seed(seed)
    gt = (torch.randn(B, 2, *hw, generator=g) * 12).round() / 4
    levels = []
    for (h, w) in sizes:
        est = torch.randn(B, 2, h, w, generator=g) * 2
        if (h, w) == tuple(hw):
            est = gt + torch.randn(B, 2, h, w, generator=g) * 1.5
            flat, ref = est.view(-1), gt.view(-1)
            n = flat.numel()
            flat[0:n:7] = ref[0:n:7]                          # residual 0
            flat[1:n:7] = ref[1:n:7] + DELTA                  # residual exactly delta
            flat[2:n:7] = ref[2:n:7] - DELTA
            assert bool(((flat - ref)[1:n:7] == DELTA).all()) and bool(((flat - ref)[0:n:7] == 0).all())
        lv = None if lvc == 0 else torch.randn(B, lvc, h, w, generator=g)
        levels.append((est, lv))
    return gt.to(dev), levels


def _masks(kind, B, sizes, hw, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == "none":
        return None
    if kind == "partial":                                      # one full-resolution mask, resized per level by _level_mask
        return torch.rand(B, *hw, generator=g) > 0.3
    per_level = [torch.rand(B, h, w, generator=g) > 0.4 for (h, w) in sizes]
    per_level[0] = torch.zeros(B, *sizes[0], dtype=torch.bool)  # "empty0": no valid pixel on the first level
    return per_level


def _run(loss_mod, levels, gt, mask, dev):
    ins = [(f.clone().to(dev).requires_grad_(True), None if lv is None else lv.clone().to(dev).requires_grad_(True))
           for f, lv in levels]
    arg = [(f, lv) if lv is not None else f for f, lv in ins]
    if mask is not None:
        mask = [m.to(dev) for m in mask] if isinstance(mask, list) else mask.to(dev)
    loss = loss_mod(arg, gt, mask=mask)
    loss.backward()
    grads = [(f.grad, None if lv is None else lv.grad) for f, lv in ins]
    return loss.detach(), grads


def _compare(got, want, what):
    (l1, g1), (l0, g0) = got, want
    assert torch.isfinite(l1).all()
    assert abs(float(l1) - float(l0)) <= 1e-5 * abs(float(l0)), (what, float(l1), float(l0))
    for i, (a, b) in enumerate(zip(g1, g0)):
        for x, y, nm in ((a[0], b[0], "flow"), (a[1], b[1], "logvar")):
            if x is None:
                assert y is None
                continue
            assert torch.isfinite(x).all(), (what, i, nm)
            y = torch.zeros_like(x) if y is None else y        # (torch: a level without valid pixels is not in the graph)
            err, top = float((x - y).abs().max()), float(y.abs().max())
            assert err <= 1e-4 * max(top, 1e-6), (what, i, nm, err, top)


CASES = [(lt, lvc) for lt in ("L1Loss", "L2Loss", "HuberLoss") for lvc in (0, 1, 2) if not (lt == "L1Loss" and lvc)]


@pytest.mark.parametrize("mask_kind", ["none", "partial", "empty0"])
@pytest.mark.parametrize("loss_type,lvc", CASES)
@pytest.mark.parametrize("B", [1, 3])
def test_fused_matches_torch_formulation(dev, monkeypatch, B, loss_type, lvc, mask_kind):
    from refign_amd import losses
    seed = B * 100 + lvc * 10 + len(loss_type)
    gt, levels = _case(dev, B, lvc, SIZES, (H, W), seed)
    mask = _masks(mask_kind, B, SIZES, (H, W), seed)
    mod = losses.MultiScaleFlowLoss(loss_type=loss_type, level_weights=[0.5, 2.0, 1.0])
    calls = _count_entry(monkeypatch, ["rfn_flowloss_fwd_f32"])
    got = _run(mod, levels, gt, mask, dev)
    assert calls.get("rfn_flowloss_fwd_f32") == 1
    monkeypatch.setattr(losses, "FUSED_LEVEL_LOSS", False)
    want = _run(mod, levels, gt, mask, dev)
    assert calls.get("rfn_flowloss_fwd_f32") == 1
    _compare(got, want, (B, loss_type, lvc, mask_kind))
    if mask_kind == "empty0":
        # the level without a valid pixel contributes exactly 0 and its gradients are exactly 0
        from refign_amd import flowloss
        ms = [losses._level_mask(m.to(dev), f.shape[-2:]) for m, (f, _) in zip(mask, levels)]
        ins = [(f.to(dev), None if lv is None else lv.to(dev)) for f, lv in levels]
        _, per_level = flowloss.multi_level_flow_loss(ins, gt, ms, [0.5, 2.0, 1.0], loss_type, return_levels=True)
        assert float(per_level[0]) == 0.0 and bool(torch.isfinite(per_level).all())
        assert float(got[1][0][0].abs().max()) == 0.0
        assert got[1][0][1] is None or float(got[1][0][1].abs().max()) == 0.0


@pytest.mark.parametrize("lvc", [0, 2])
def test_fused_matches_torch_formulation_several_blocks(dev, monkeypatch, lvc):
    """A level of 130 x 130 at B = 2: 33 800 pixels, more than one workgroup of partials, the last one partly filled."""
    from refign_amd import _lib, losses
    sizes, hw = [(33, 33), (130, 130)], (260, 260)
    assert 2 * 130 * 130 > 4 * _lib.load_library().rfn_flowloss_block_pixels()
    gt, levels = _case(dev, 2, lvc, sizes, hw, 7 + lvc)
    mask = torch.rand(2, *hw, generator=torch.Generator().manual_seed(3)) > 0.2
    mod = losses.MultiScaleFlowLoss(loss_type="HuberLoss", level_weights=[0.25, 1.0])
    got = _run(mod, levels, gt, mask, dev)
    monkeypatch.setattr(losses, "FUSED_LEVEL_LOSS", False)
    _compare(got, _run(mod, levels, gt, mask, dev), ("130x130", lvc))


# ---------------------------------------------------------------------------------------------------------------------
# 3. repeatability
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_loss_is_bit_repeatable(dev):
    from refign_amd import losses
    z = golden("matcher_losses_128x160")
    flow, mask = T(z["flow_prime"], dev), T(z["mask_prime"], dev)
    mod = losses.MultiScaleFlowLoss(loss_type='HuberLoss', level_weights=WEIGHTS)
    runs = []
    for _ in range(2):
        first, _ = _golden_levels(z, dev)
        loss = mod(first, flow, mask=mask)
        loss.backward()
        runs.append([loss.detach()] + [t.grad for pair in first for t in pair])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    gt, levels = _case(dev, 2, 2, [(130, 130)], (260, 260), 11)
    a, b = (_run(losses.MultiScaleFlowLoss(loss_type="L2Loss"), levels, gt, None, dev) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0][0], b[1][0][0]) and torch.equal(a[1][0][1], b[1][0][1])


# ---------------------------------------------------------------------------------------------------------------------
# 4. no host synchronisation
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_losses_do_not_synchronise(dev):
    from refign_amd import losses
    z = golden("matcher_losses_128x160")
    flow, mask = T(z["flow_prime"], dev), T(z["mask_prime"], dev)
    ss = losses.MultiScaleFlowLoss(loss_type='HuberLoss', level_weights=WEIGHTS)
    us = losses.WBipathLoss(objective='multi_scale_flow_loss', loss_type='HuberLoss', visibility_mask=True)

    def once():
        first, second = _golden_levels(z, dev)
        total = ss(first, flow, mask=mask) + us(first, second, flow, mask_used=mask)
        total.backward()
        return total.detach()
    warm = once()                                            # the library, the allocator's blocks
    first, second = _golden_levels(z, dev)                   # (uploads are not part of the loss)
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        total = ss(first, flow, mask=mask) + us(first, second, flow, mask_used=mask)
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert abs(float(total) - float(warm)) <= 1e-5 * abs(float(warm))

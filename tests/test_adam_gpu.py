"""GPU: optim.MultiTensorAdam -- torch.optim.Adam (weight decay as an L2 term of the gradient) of a whole parameter set as
one launch (csrc/reduce.hip: rfn_multi_adam_f32 / rfn_multi_adam_amp_f32) against torch's own non-fused step."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(257, 33), (64,), (3, 3, 16, 16), (70001,), (5,), (128, 128)]
LRS = [1e-3, 3e-4, 1e-2]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _make(params, **kw):
    return torch.optim.Adam([{"params": params[:2], "lr": LRS[0], "weight_decay": 0.01},
                             {"params": params[2:4], "lr": LRS[1], "weight_decay": 0.0},
                             {"params": params[4:], "lr": LRS[2], "weight_decay": 0.1, "betas": (0.8, 0.99)}], **kw)


def _pair(dev, seed=0):
    torch.manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in SHAPES]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    flat = torch.zeros(sum(q.numel() for q in qs), device=dev)      # gradients as persistent views, as in the trainer
    o = 0
    for q in qs:
        q.grad = flat[o:o + q.numel()].view_as(q)
        o += q.numel()
    return ps, qs


def _fill(ps, qs, it):
    for p, q in zip(ps, qs):
        g = torch.randn_like(p) * (0.1 + it)
        p.grad = g.clone()
        q.grad.copy_(g)


def _assert_close(ref, mine, ps, qs):
    for p, q in zip(ps, qs):
        assert float((p - q).abs().max()) <= 2e-6 * float(p.abs().max())
        for k in ("exp_avg", "exp_avg_sq"):
            a, b = ref.state[p][k], mine.state[q][k]
            assert float((a - b).abs().max()) <= 2e-6 * float(a.abs().max()) + 1e-12, k


def test_multi_tensor_adam_matches_torch(dev):
    """6 steps with fresh gradients, 3 parameter groups (one with weight_decay=0), odd sizes, the learning rate changing
    every step: parameters and both moments to 2e-6 relative, step counters equal, 5 launches (torch takes step 1)."""
    from refign_amd.optim import MultiTensorAdam
    ps, qs = _pair(dev)
    ref, mine = _make(ps, foreach=False), _make(qs)
    fast = MultiTensorAdam(mine)
    for it in range(6):
        _fill(ps, qs, it)
        for opt in (ref, mine):
            for gi, grp in enumerate(opt.param_groups):
                grp["lr"] = LRS[gi] * (1.0 - 0.1 * it)
        ref.step()
        fast.step()
    assert fast.launches == 5
    _assert_close(ref, mine, ps, qs)
    sd = mine.state_dict()                                           # looking at the state brings the counters up to date
    assert all(float(s["step"]) == 6.0 for s in sd["state"].values())
    for p, q in zip(ps, qs):
        assert float(ref.state[p]["step"]) == float(mine.state[q]["step"]) == 6.0


def test_multi_tensor_adam_weight_decay_is_l2_not_decoupled(dev):
    """The decay form is the point of the class: with a large weight decay Adam and AdamW part ways in the first digits."""
    from refign_amd.optim import MultiTensorAdam
    ps, qs = _pair(dev, 3)
    ref, mine = _make(ps, foreach=False), _make(qs)
    decoupled = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in ps[4:]], lr=LRS[2], weight_decay=0.1,
                                  betas=(0.8, 0.99))
    fast = MultiTensorAdam(mine)
    for it in range(3):
        _fill(ps, qs, it)
        for r, p in zip(decoupled.param_groups[0]["params"], ps[4:]):
            r.grad = p.grad.clone()
        ref.step(), fast.step(), decoupled.step()
    _assert_close(ref, mine, ps, qs)
    r5, q5 = decoupled.param_groups[0]["params"][1], qs[5]
    assert float((r5 - q5).abs().max()) > 1e-4 * float(q5.abs().max())


def test_multi_tensor_adam_declines_what_is_not_plain_adam(dev):
    from refign_amd.optim import MultiTensorAdam
    for kw in ({"amsgrad": True}, {"maximize": True}):
        opt = torch.optim.Adam([torch.nn.Parameter(torch.randn(8, device=dev))], **kw)
        opt.param_groups[0]["params"][0].grad = torch.ones(8, device=dev)
        f = MultiTensorAdam(opt)
        f.step(), f.step()
        assert f.launches == 0, kw
    w = torch.optim.AdamW([torch.nn.Parameter(torch.randn(8, device=dev))])
    w.param_groups[0]["params"][0].grad = torch.ones(8, device=dev)
    f = MultiTensorAdam(w)
    f.step(), f.step()
    assert f.launches == 0


def test_multi_tensor_adam_follows_load_state_dict(dev):
    """load_state_dict in mid-run replaces every moment tensor and the step counters: the one-launch step continues from
    the LOADED state."""
    from refign_amd.optim import MultiTensorAdam
    ps, qs = _pair(dev, 1)
    ref, mine = _make(ps, foreach=False), _make(qs)
    fast = MultiTensorAdam(mine)
    torch.manual_seed(5)
    grads = [[torch.randn_like(p) for p in ps] for _ in range(7)]

    def run(it):
        for p, q, g in zip(ps, qs, grads[it]):
            p.grad = g.clone()
            q.grad.copy_(g)
        ref.step()
        fast.step()
    for it in range(3):
        run(it)
    saved = (copy.deepcopy(ref.state_dict()), [p.detach().clone() for p in ps], copy.deepcopy(mine.state_dict()))
    for it in range(3, 5):
        run(it)
    ref.load_state_dict(saved[0])
    mine.load_state_dict(saved[2])
    with torch.no_grad():
        for p, q, v in zip(ps, qs, saved[1]):
            p.copy_(v)
            q.copy_(v)
    for it in range(5, 7):
        run(it)
    _assert_close(ref, mine, ps, qs)
    mine.state_dict()
    for p, q in zip(ps, qs):
        assert float(ref.state[p]["step"]) == float(mine.state[q]["step"]) == 5.0


def test_multi_tensor_adam_amp_step_skips_on_found_inf(dev):
    """step_amp: the update of step t = device_step + 1 when found_inf is 0 (against torch), and nothing at all -- parameters
    and both moments bit-equal -- when it is set."""
    from refign_amd.optim import MultiTensorAdam
    ps, qs = _pair(dev, 2)
    ref, mine = _make(ps, foreach=False), _make(qs)
    fast = MultiTensorAdam(mine)
    found = torch.zeros(1, device=dev)
    _fill(ps, qs, 0)
    ref.step()
    assert fast.step_amp(found) is False                              # no state yet: the caller steps torch's optimizer
    mine.step()
    for it in range(1, 3):
        _fill(ps, qs, it)
        ref.step()
        assert fast.step_amp(found) is True
        fast.device_step.add_(1.0)                                    # what LossScaler.update does when the step was taken
    _assert_close(ref, mine, ps, qs)
    before = [(q.detach().clone(), mine.state[q]["exp_avg"].clone(), mine.state[q]["exp_avg_sq"].clone()) for q in qs]
    _fill(ps, qs, 3)
    found.fill_(1.0)
    assert fast.step_amp(found) is True
    for q, (p0, m0, v0) in zip(qs, before):
        assert torch.equal(q, p0) and torch.equal(mine.state[q]["exp_avg"], m0) and torch.equal(mine.state[q]["exp_avg_sq"], v0)
    assert float(fast.device_step) == 3.0

"""GPU: the decode heads without their extra passes (refign_amd/bn.py, seg.py, upcat.py; csrc/bn.hip, csrc/upcat.hip):
  * Dropout2d folded into the BatchNorm passes (bn_act_train(drop=...)): bit for bit the chain `bn_act_train` then `y * noise`
    on the same kernels, forward and backward, and the same consumption of the generator by a whole DAFormerHead;
  * the backward passes on a grad_y read in place from a channel slice (the `_ld` entry points), inside a guard-band arena;
  * the student's ASPP with its branches written into the concatenation under autograd (seg._ASPP_NOCAT_GRAD);
  * the gradients of the ASPP input summed inside the gather backward of upsample_concat (seg._UPCAT_FANIN)."""
import copy

import pytest
import torch

from guardband import FILLS, GuardArena

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bn(C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.rand(C, generator=g) - 0.5)
    return bn


def _case(B, C, H, W, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3).to(dev).to(dtype).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(B, C, H, W, generator=g).to(dev).to(dtype).contiguous(memory_format=torch.channels_last)
    noise = torch.empty(B, C, 1, 1).bernoulli_(0.5, generator=g).div_(0.5).to(dev).to(dtype)
    assert bool((noise == 0).any()) and bool((noise == 2).any())           # dropped and kept channels both occur
    return x, gy, noise


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C", [64, 72])
def test_dropout_in_the_batchnorm_passes_equals_the_multiply_after_them(dev, C, dtype, relu):
    """B = 3 samples of 7 x 9 = 63 rows: with 32 row lanes and 2 workgroup rows a thread's stride is 64 rows, so consecutive rows
    of a thread lie in different samples, also inside the four-row loop of the statistics; C = 72: nine channel vectors, the
    second block of eight masked.  The fused passes give the bits of the chain (same kernels, multiply by ATen): y, and under
    deterministic mode the backward sums, grad_x and the parameter gradients; the apply pass alone on given sums too.  The
    atomic backward sums against an fp64 sum: the bound of test_syncbn_gpu.test_split_phase_kernels_with_added_buffers_equal_
    full_batch for those sums (2 % of their largest + 1e-3)."""
    from refign_amd import bn as bnk
    from refign_amd import determinism
    B, H, W = 3, 7, 9
    x, gy, noise = _case(B, C, H, W, dtype, dev, 11 * C + int(relu))
    bn0 = _bn(C, dev, C)

    def chain():
        bn, xx = copy.deepcopy(bn0), x.clone().requires_grad_(True)
        y = bnk.bn_act_train(xx, bn, relu, dtype) * noise
        y.backward(gy)
        return y.detach(), xx.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var, bn.num_batches_tracked

    def fused():
        bn, xx = copy.deepcopy(bn0), x.clone().requires_grad_(True)
        y = bnk.bn_act_train(xx, bn, relu, dtype, drop=noise)
        y.backward(gy)
        return y.detach(), xx.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var, bn.num_batches_tracked

    with determinism.deterministic():
        want, got = chain(), fused()
    for name, a, b in zip(("y", "grad_x", "grad_weight", "grad_bias", "running_mean", "running_var", "batches"), got, want):
        assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))
    assert torch.equal(fused()[0], want[0])                                # (the forward does not depend on the mode)

    # the passes themselves
    xh, gh, drop = x.permute(0, 2, 3, 1), gy.permute(0, 2, 3, 1), noise.view(B, C)
    gmul = (gy * noise).permute(0, 2, 3, 1)                                # what the multiply's backward hands to BatchNorm
    assert xh.is_contiguous() and gh.is_contiguous() and gmul.is_contiguous()
    w, b = bn0.weight.detach(), bn0.bias.detach()
    sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
    bnk._stats_fwd(xh, sums)
    det = []
    with determinism.deterministic():
        for g_, kw in ((gmul, {}), (gh, {"drop": drop})):
            bs = torch.empty((2, C), dtype=torch.float32, device=dev)
            bnk._stats_bwd(xh, g_, sums, w, b, bs, 1e-5, int(relu), **kw)
            det.append(bs)
    assert torch.equal(det[0], det[1])
    gxs = []
    for g_, kw in ((gmul, {}), (gh, {"drop": drop})):
        gx = torch.empty_like(xh)
        bnk._apply_bwd(xh, g_, sums, det[0], w, b, gx, 1e-5, int(relu), **kw)
        gxs.append(gx)
    assert torch.equal(gxs[0], gxs[1])
    atomic = torch.empty((2, C), dtype=torch.float32, device=dev)
    bnk._stats_bwd(xh, gh, sums, w, b, atomic, 1e-5, int(relu), drop=drop)
    xd = xh.double().reshape(-1, C)
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    xhat = (xd - mean) * torch.rsqrt(var + 1e-5)
    gd = gmul.double().reshape(-1, C)
    if relu:
        gd = gd * ((xhat * w.double() + b.double()) > 0)
    ref = torch.stack((gd.sum(0), (gd * xhat).sum(0)))
    for i in (0, 1):
        err, bound = float((atomic[i].double() - ref[i]).abs().max()), 0.02 * float(ref[i].abs().max()) + 1e-3
        print(f"atomic backward sums[{i}]: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def _head_inputs(dev, requires_grad):
    g = torch.Generator().manual_seed(21)
    sizes = [(20, 28), (10, 14), (5, 7), (3, 4)]
    return [torch.randn(2, c, h, w, generator=g).to(dev).requires_grad_(requires_grad)
            for c, (h, w) in zip([32, 64, 160, 256], sizes)]


@pytest.mark.parametrize("mode", ["teacher", "autograd"])
@pytest.mark.parametrize("head_type", ["DAFormerHead", "SegFormerHead"])
def test_fused_dropout_draws_from_the_generator_like_the_module(dev, head_type, mode, monkeypatch):
    """One seed, a head in training mode with Dropout2d(0.1), the multiply inside the BatchNorm pass and as the module: the same
    logits and the same generator state afterwards -- gradient-free (the EMA teacher) and under autograd (there, in deterministic
    mode, the same input and parameter gradients too)."""
    import contextlib
    from refign_amd import determinism, seg
    torch.manual_seed(2)
    if head_type == "DAFormerHead":
        head0 = seg.DAFormerHead([32, 64, 160, 256], [0, 1, 2, 3], 19, 'multiple_select', channels=64, embed_dims=64)
    else:
        head0 = seg.SegFormerHead([32, 64, 160, 256], [0, 1, 2, 3], 19, 'multiple_select', channels=64)
    head0 = head0.to(dev).train()
    calls, res = [], {}
    for fused in (True, False):
        monkeypatch.setattr(seg, "_DROPOUT_FUSED", fused)
        head = copy.deepcopy(head0)
        xs = _head_inputs(dev, mode == "autograd")
        torch.manual_seed(7)
        grad = contextlib.nullcontext() if mode == "autograd" else torch.no_grad()
        with grad, determinism.deterministic(mode == "autograd"), torch.autocast("cuda", dtype=torch.bfloat16):
            mults = []
            hook = head.dropout.register_forward_hook(lambda m, i, o: mults.append(1))
            y = head(xs)
            hook.remove()
            calls.append(len(mults))
            grads = []
            if mode == "autograd":
                y.float().square().mean().backward()
                grads = [t.grad for t in xs] + [p.grad for p in head.parameters()]
        res[fused] = (y.detach(), torch.cuda.get_rng_state(dev), grads)
    assert calls == [0, 1]                                                  # the module's multiply ran only with the fusion off
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
    assert len(res[True][2]) == len(res[False][2])
    for a, b in zip(res[True][2], res[False][2]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    monkeypatch.setattr(seg, "_DROPOUT_FUSED", True)
    torch.manual_seed(8)                                                    # another seed, other logits: the noise is in them
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert not torch.equal(copy.deepcopy(head0)(_head_inputs(dev, False)), res[True][0])


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("C,off,wide", [(64, 64, 256), (64, 192, 256), (72, 136, 208)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_backward_passes_read_grad_y_in_place_from_a_channel_slice(dev, dtype, C, off, wide, fill):
    """grad_y as a channel slice of a wider channels-last tensor, by row pitch (rfn_bn_stats_bwd_det_ld / rfn_bn_stats_bwd_ld /
    rfn_bn_apply_bwd_ld): the bits of the dense entry points on a contiguous copy of the slice (the sums in their deterministic
    form).  The wide tensor and everything the passes allocate live in a guard-band arena: nothing outside the results is written,
    and the wide tensor itself is unchanged."""
    from refign_amd import bn as bnk
    from refign_amd import determinism
    B, H, W = 3, 7, 9
    g = torch.Generator().manual_seed(C + off)
    xh = (torch.randn(B, H, W, C, generator=g) * 1.5 + 0.3).to(dev).to(dtype)
    wide_g = torch.randn(B, H, W, wide, generator=g).to(dev).to(dtype)
    bn = _bn(C, dev, off)
    w, b = bn.weight.detach(), bn.bias.detach()
    sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
    bnk._stats_fwd(xh, sums)

    def passes(gy):
        with determinism.deterministic():
            bs = torch.empty((2, C), dtype=torch.float32, device=dev)
            bnk._stats_bwd(xh, gy, sums, w, b, bs, 1e-5, 1)
        gx = torch.empty_like(xh)
        bnk._apply_bwd(xh, gy, sums, bs, w, b, gx, 1e-5, 1)
        atomic = torch.empty((2, C), dtype=torch.float32, device=dev)
        bnk._stats_bwd(xh, gy, sums, w, b, atomic, 1e-5, 1)
        return bs, gx, atomic

    dense = wide_g[..., off:off + C].contiguous()
    want = passes(dense)                                                    # (also sizes the cached workspace outside the arena)
    arena = GuardArena(dev, fill, 4 << 20)
    placed = arena.place(wide_g)
    sl = placed[..., off:off + C]
    assert not sl.is_contiguous() and sl.stride(-2) == wide
    with arena.allocations():
        got = passes(sl)
    arena.check()
    assert torch.equal(placed, wide_g)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the atomic form: the same sums up to the order of fp32 additions (bound: as in the test above, from test_syncbn_gpu)
    for i in (0, 1):
        assert float((got[2][i] - want[0][i]).abs().max()) <= 0.02 * float(want[0][i].abs().max()) + 1e-3


def _aspp_run(aspp0, x0, seg, monkeypatch, nocat, deterministic):
    from refign_amd import determinism
    monkeypatch.setattr(seg, "_ASPP_NOCAT_GRAD", nocat)
    aspp, x = copy.deepcopy(aspp0), x0.clone().requires_grad_(True)
    cats, real = [], torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **k: (cats.append(1), real(*a, **k))[1])
    with determinism.deterministic(deterministic), torch.autocast("cuda", dtype=torch.bfloat16):
        y = aspp(x)
        y.float().square().mean().backward()
    monkeypatch.setattr(torch, "cat", real)
    return (y.detach(), x.grad, {n: p.grad for n, p in aspp.named_parameters()}, {n: v.clone() for n, v in aspp.named_buffers()},
            len(cats))


def test_student_aspp_writes_its_branches_into_the_concatenation(dev, monkeypatch):
    """ASPP under autograd (the student's decode head): the branches' BatchNorm + ReLU passes write into the concatenation and
    their backward passes read its gradient by row pitch (bn._BNActCat) == the torch.cat formulation on the same kernels: output,
    running statistics and num_batches_tracked; under deterministic mode the input gradient and every parameter gradient."""
    from refign_amd import seg
    torch.manual_seed(4)
    aspp0 = seg.ASPPWrapper(128, 64, True, (1, 6, 12, 18), False, torch.nn.BatchNorm2d, torch.nn.ReLU).to(dev).train()
    x0 = torch.randn(3, 128, 20, 28, device=dev)
    new, old = _aspp_run(aspp0, x0, seg, monkeypatch, True, False), _aspp_run(aspp0, x0, seg, monkeypatch, False, False)
    assert torch.equal(new[0], old[0])
    assert len(new[3]) == len(old[3]) == 3 * 8 and all(torch.equal(new[3][n], old[3][n]) for n in old[3])
    new, old = _aspp_run(aspp0, x0, seg, monkeypatch, True, True), _aspp_run(aspp0, x0, seg, monkeypatch, False, True)
    assert new[4] == old[4] - 1                                             # the concatenation is gone
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])
    assert all(g is not None for g in old[2].values()) and len(old[2]) == len(new[2])
    for n in old[2]:
        assert torch.equal(new[2][n], old[2][n]), n


@pytest.mark.parametrize("handles,used", [(1, (0,)), (2, (0, 1)), (4, (0, 1, 2, 3)), (4, (0, 2, 3))])
def test_gradients_of_several_consumers_are_added_inside_the_gather(dev, handles, used):
    """upsample_concat(handles=...): the gradients arriving through the handles are added in fp32 inside the backward's gather
    kernel (rfn_upsample_concat_nhwc_bwd_sum) and rounded once; a handle nobody used is skipped.  Shapes of test_seg_gpu.
    test_upsample_concat_fused_matches_interpolate_cat.  Reference: the fp64 sum of the operands through the fp64 bilinear
    backward.  The fused result is no further from it than the chain it replaces (16-bit additions by ATen, then the
    single-operand entry point), and element by element within that test's tolerance for the single-operand kernel."""
    import torch.nn.functional as F
    from refign_amd.upcat import upsample_concat
    sizes, chans, n, dt = [(34, 60), (17, 30), (9, 15), (5, 8)], [32, 32, 32, 32], 2, torch.bfloat16
    H, W = 34, 60
    g = torch.Generator().manual_seed(handles * 10 + len(used))
    toks = [torch.randn(n, h * w, c, generator=g).to(dev).to(dt) for (h, w), c in zip(sizes, chans)]
    gos = [torch.randn(n, sum(chans), H, W, generator=g).to(dev).to(dt).contiguous(memory_format=torch.channels_last) for _ in used]

    def run(k, grads):
        leaves = [t.clone().requires_grad_() for t in toks]
        out = upsample_concat(leaves, sizes, (H, W), handles=k)
        outs = [out] if k == 1 else list(out)
        assert len(outs) == k and all(torch.equal(o, outs[0]) for o in outs)
        torch.autograd.backward([outs[i] for i in (used if k > 1 else (0,))], grads)
        return [t.grad for t in leaves]

    got = run(handles, gos)
    chain_g = gos[0]
    for t in gos[1:]:
        chain_g = chain_g + t                                              # what the autograd engine did: a 16-bit rounding each
    chain = run(1, [chain_g])
    leaves = [t.double().requires_grad_() for t in toks]
    parts = []
    for t, (h, w), c in zip(leaves, sizes, chans):
        m = t.transpose(1, 2).reshape(n, c, h, w)
        parts.append(m if (h, w) == (H, W) else F.interpolate(m, size=(H, W), mode='bilinear', align_corners=False))
    torch.cat(parts, 1).backward(sum(t.double() for t in gos))
    err_fused = max(float((a.double() - r.grad).abs().max()) for a, r in zip(got, leaves))
    err_chain = max(float((a.double() - r.grad).abs().max()) for a, r in zip(chain, leaves))
    print(f"handles {handles}, used {used}: max error fused {err_fused:.4e}, chain {err_chain:.4e}")
    assert err_fused <= err_chain
    for a, r in zip(got, leaves):
        assert torch.allclose(a.float(), r.grad.float(), rtol=2e-2, atol=2e-2)
    if len(used) == 1:
        assert all(torch.equal(a, b) for a, b in zip(got, chain))

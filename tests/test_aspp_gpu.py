"""GPU: DeepLabV2Head's tap-GEMM path (csrc/aspp.hip: rfn_aspp_tapsum / rfn_aspp_tapsum_bwd around the existing GEMM kernels)
against an fp64 torch reference of the four dilated convolutions, and against the per-branch path (four conv.Conv2d on the
implicit-GEMM kernels, resnet.ASPP_FUSED = False) on the same inputs.

The bound is relative to the per-branch path: with e_pb = max |per-branch - fp64| of a tensor, the fused path is held to
2 e_pb + 1 ulp of that tensor's dtype (ulp: the dtype's spacing at the reference's largest magnitude, finfo.eps * max |ref|).
Inputs, weights and the incoming gradient are representable in the 16-bit dtype, so the fp64 reference sees exactly the values
the kernels see.  tools/deeplabv2_parity.py writes both errors per shape into profiles/deeplabv2_parity.txt.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DILATIONS = (6, 12, 18, 24)
# (B, C, H, W, classes): 12 live taps; 24; all 36, ragged against any tile; centre taps only; the configs' channel count
CASES = [(2, 64, 7, 9, 19), (1, 128, 25, 13, 19), (2, 64, 33, 41, 19), (1, 64, 5, 5, 19), (1, 2048, 9, 11, 19), (2, 64, 7, 9, 5)]
DTYPES = [torch.bfloat16, torch.float16]
TENSORS = ("out", "dx", "dw", "db")
_REF = {}


def _inputs(case, dtype):
    """x, gy (both exactly representable in dtype), and the head's parameters rounded to dtype, on the CPU in fp32"""
    B, C, H, W, K = case
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W + K)
    r = lambda t: t.to(dtype).float()  # noqa: E731
    x = r(torch.randn(B, C, H, W, generator=g))
    gy = r(torch.randn(B, K, H, W, generator=g))
    ws = [r(torch.randn(K, C, 3, 3, generator=g) * (9 * C) ** -0.5) for _ in DILATIONS]
    bs = [r(torch.randn(K, generator=g) * 0.1) for _ in DILATIONS]
    return x, gy, ws, bs


def reference(case, dtype):
    """fp64 forward and gradients of sum_r conv_r on the CPU, computed once per (case, dtype) and shared"""
    key = (case, dtype)
    if key not in _REF:
        x, gy, ws, bs = _inputs(case, dtype)
        x64 = x.double().requires_grad_()
        ws64 = [w.double().requires_grad_() for w in ws]
        bs64 = [b.double().requires_grad_() for b in bs]
        with torch.enable_grad():
            y = sum(torch.nn.functional.conv2d(x64, w, b, 1, d, d) for w, b, d in zip(ws64, bs64, DILATIONS))
            grads = torch.autograd.grad(y, [x64] + ws64 + bs64, gy.double())
        n = len(DILATIONS)
        _REF[key] = {"out": y.detach(), "dx": grads[0], "dw": torch.stack(grads[1:1 + n]), "db": torch.stack(grads[1 + n:])}
    return _REF[key]


def make_head(case, dtype, dev, dilations=DILATIONS, paddings=None):
    from refign_amd import resnet
    B, C, H, W, K = case
    _, _, ws, bs = _inputs(case, dtype)
    head = resnet.DeepLabV2Head(C, 0, K, dilation_series=list(dilations), padding_series=list(paddings or dilations))
    with torch.no_grad():
        for conv, w, b in zip(head.conv2d_list, ws, bs):
            conv.weight.copy_(w)
            conv.bias.copy_(b)
    return head.to(dev).train()


def run_head(head, case, dtype, dev, fused, reset_grads=True):
    """forward + backward under autocast -> {out, dx, dw, db} in fp64 on the CPU, and the dtypes the tensors came in"""
    from refign_amd import resnet
    x, gy, _, _ = _inputs(case, dtype)
    x = x.to(dev).to(dtype).requires_grad_()           # a 16-bit leaf: what the backbone hands the head under autocast
    saved, resnet.ASPP_FUSED = resnet.ASPP_FUSED, fused
    try:
        assert head.fused_ok(x.detach()) == fused
        if reset_grads:
            for p in head.parameters():
                p.grad = None
        with torch.autocast("cuda", dtype=dtype):
            y = head([x])
        y.backward(gy.to(dev).to(y.dtype))
    finally:
        resnet.ASPP_FUSED = saved
    torch.cuda.synchronize()
    got = {"out": y.detach(), "dx": x.grad, "dw": torch.stack([c.weight.grad for c in head.conv2d_list]),
           "db": torch.stack([c.bias.grad for c in head.conv2d_list])}
    dts = {k: v.dtype for k, v in got.items()}
    return {k: v.double().cpu() for k, v in got.items()}, dts


def measure(case, dtype, dev):
    """-> {tensor: (fused error, per-branch error, bound, fused-vs-per-branch difference)}"""
    ref = reference(case, dtype)
    head = make_head(case, dtype, dev)
    pb, dts = run_head(head, case, dtype, dev, fused=False)
    fu, dts_f = run_head(head, case, dtype, dev, fused=True)
    out = {}
    for k in TENSORS:
        assert fu[k].shape == ref[k].shape == pb[k].shape and dts_f[k] == dts[k], k
        e_pb = float((pb[k] - ref[k]).abs().max())
        e_fu = float((fu[k] - ref[k]).abs().max())
        ulp = float(torch.finfo(dts[k]).eps) * float(ref[k].abs().max())
        out[k] = (e_fu, e_pb, 2 * e_pb + ulp, float((fu[k] - pb[k]).abs().max()))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_fused_head_matches_fp64_within_twice_the_per_branch_error(dev, case, dtype):
    res = measure(case, dtype, dev)
    for k, (e_fu, e_pb, bound, diff) in res.items():
        print(f"{case} {dtype} {k}: fused {e_fu:.3e} per-branch {e_pb:.3e} bound {bound:.3e} fused-vs-per-branch {diff:.3e}")
    for k, (e_fu, e_pb, bound, diff) in res.items():
        assert e_fu <= bound, f"{k}: fused error {e_fu:.3e} > 2 x per-branch error {e_pb:.3e} + 1 ulp = {bound:.3e}"
        assert diff <= bound, f"{k}: fused and per-branch differ by {diff:.3e} > {bound:.3e}"


def test_padding_other_than_dilation_takes_the_per_branch_path(dev, monkeypatch):
    from refign_amd import resnet
    case = (1, 64, 9, 11, 19)
    head = make_head(case, torch.bfloat16, dev, dilations=(2,), paddings=(3,))
    x, _, ws, bs = _inputs(case, torch.bfloat16)
    assert not head.fused_ok(x.to(dev).bfloat16())

    def refuse(*a, **k):
        raise AssertionError("the fused path ran")
    monkeypatch.setattr(resnet, "_tapsum", refuse)
    with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
        y = head([x.to(dev)])
    want = torch.nn.functional.conv2d(x.double(), ws[0].double(), bs[0].double(), 1, 3, 2)
    assert y.shape == want.shape == (1, 19, 11, 13)
    assert float((y.double().cpu() - want).abs().max()) <= 2 ** -7 * float(want.abs().max())
    # and the switch: with ASPP_FUSED off an in-domain head does not reach the kernel either
    head = make_head(case, torch.bfloat16, dev)
    assert head.fused_ok(x.to(dev).bfloat16())
    monkeypatch.setattr(resnet, "ASPP_FUSED", False)
    assert not head.fused_ok(x.to(dev).bfloat16())
    with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
        head([x.to(dev)])


@pytest.mark.parametrize("sink", [False, True], ids=["autograd", "grad_sink"])
def test_dead_taps_get_exactly_zero_weight_gradient(dev, sink):
    """7 x 9: branch 0 (d = 6) has all nine taps live, branches 1-3 their centre tap only."""
    from refign_amd import params
    case = CASES[0]
    head = make_head(case, torch.bfloat16, dev)
    if sink:                                      # the trainer's flat gradient buffer: kernels add into p.grad themselves
        for p in head.parameters():
            p.grad = torch.zeros_like(p)
            params.mark_grad_sink(p)
    got, _ = run_head(head, case, torch.bfloat16, dev, fused=True, reset_grads=not sink)
    dw = got["dw"]
    assert float(dw[0].abs().min()) > 0.0
    for r in range(1, 4):
        dead = torch.ones(3, 3, dtype=torch.bool)
        dead[1, 1] = False
        assert float(dw[r][:, :, dead].abs().max()) == 0.0
        assert float(dw[r][:, :, 1, 1].abs().min()) > 0.0
    ref = reference(case, torch.bfloat16)
    assert float((dw - ref["dw"]).abs().max()) <= 1e-3 * float(ref["dw"].abs().max())
    assert float((got["db"] - ref["db"]).abs().max()) <= 1e-3 * float(ref["db"].abs().max())


def test_two_deterministic_runs_have_equal_bits(dev):
    from refign_amd import determinism
    case = CASES[2]
    head = make_head(case, torch.float16, dev)
    with determinism.deterministic():
        assert determinism.enabled()
        a, _ = run_head(head, case, torch.float16, dev, fused=True)          # (an RFN_ENONDET refusal would raise here)
        b, _ = run_head(head, case, torch.float16, dev, fused=True)
    for k in TENSORS:
        assert torch.equal(a[k], b[k]), k
    c, _ = run_head(head, case, torch.float16, dev, fused=True)              # no atomics either way: the same bits outside the mode
    for k in TENSORS:
        assert torch.equal(a[k], c[k]), k


def test_forward_and_backward_capture_into_a_graph_and_follow_refreshed_weights(dev):
    from refign_amd import params
    case = CASES[1]
    dtype = torch.bfloat16
    head = make_head(case, dtype, dev)
    x, gy, _, _ = _inputs(case, dtype)
    x, gy = x.to(dev).requires_grad_(), gy.to(dev).to(dtype)
    plist = list(head.parameters())

    def step():
        with torch.autocast("cuda", dtype=dtype):
            y = head([x])
        return (y,) + torch.autograd.grad(y, [x] + plist, gy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                    # (makes the cached weight copies: nothing is created under capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, step()):
        assert torch.equal(a, b)
    with torch.no_grad():                         # an optimizer / EMA update: in place, then the refresh of the cached copies
        for p in plist:
            p.mul_(1.25).add_(0.01)
    params.refresh(plist)
    g.replay()
    torch.cuda.synchronize()
    fresh = step()
    assert not torch.equal(outs[0], torch.zeros_like(outs[0]))
    for a, b in zip(outs, fresh):
        assert torch.equal(a, b)


def test_entry_points_refuse_bad_arguments(dev):
    from refign_amd import _lib
    from refign_amd._tensor import ptr
    z = torch.zeros(4 * 24, dtype=torch.bfloat16, device=dev)
    import ctypes
    taps = ctypes.cast((ctypes.c_int * 2)(0, 0), ctypes.c_void_p)
    with pytest.raises(RuntimeError, match="ldz"):            # ldz < T Np
        _lib.call("rfn_aspp_tapsum", dev, ptr(z), 16, None, 0, taps, 1, ptr(z), 1, 2, 2, 24, 1)
    with pytest.raises(RuntimeError, match="taps"):           # T outside 1 .. 64
        _lib.call("rfn_aspp_tapsum_bwd", dev, ptr(z), taps, 65, ptr(z[8:]), 65 * 24, 1, 1, 1, 24, 1)
    with pytest.raises(RuntimeError, match="dtype"):
        _lib.call("rfn_aspp_tapsum", dev, ptr(z), 24, None, 0, taps, 1, ptr(z), 1, 2, 2, 24, 0)


def test_parity_figures_are_recorded():
    """profiles/deeplabv2_parity.txt carries the measured errors of both paths for every case of this file"""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "deeplabv2_parity.txt")
    text = open(path).read()
    for case in CASES:
        assert "x".join(map(str, case)) in text
    assert np.all([w in text for w in ("per-branch", "fused", "bf16", "f16")])

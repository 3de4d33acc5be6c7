"""GPU: the fused key / value path of the gradient-free MiT passes (csrc/kvpath.hip, mfma.kv_packs): spatial-reduction Linear read
in place, LayerNorm, kv Linear and the attention kernel's K / V packs in one launch, against the five-launch chain it stands for
(conv.patch_conv_tokens -> layernorm.LayerNorm -> linear.Linear -> rfn_attn_pack).

Reference semantics: Attention.forward of models/backbones/mix_transformer.py:137-164.  The kernel uses the NT GEMM's MFMA shape
and ascending K order and the LayerNorm kernel's lane arithmetic, so its plain kv output is expected BIT-EQUAL to the chain's."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guardband import GuardArena  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
B = 2
# (C, heads, r, H, W): reduced tokens per image -> what the shape exercises
CASES = [
    (64, 1, 8, 19, 27),      # 2 x 3 = 6: ragged border dropped; one partial block padded to two
    (128, 2, 4, 19, 27),     # 4 x 6 = 24: ragged border dropped
    (320, 5, 2, 24, 40),     # 240: 7.5 blocks, padded to 8; several tiles
    (320, 5, 2, 34, 30),     # 17 x 15 = 255: 8 blocks per image, the tile of blocks 6-8 spans the two images
    (512, 8, 1, 7, 10),      # 70 rows, sr_ratio == 1: 3 blocks padded to 4; the last tile is partial
]
PARAMS = [(c, torch.bfloat16) for c in CASES] + [(CASES[i], torch.float16) for i in (0, 1, 3, 4)]
IDS = [f"C{c[0]}r{c[2]}-{c[3]}x{c[4]}-{str(dt).split('.')[-1]}" for c, dt in PARAMS]
_CACHE = {}


def _setup(dev, case, dtype):
    """(module, x, today's chain's kv, the fused call's result with three pack blocks per workgroup -- the teacher's form; these
    small launches would take one), made once per case and left unchanged."""
    key = (case, dtype)
    if key not in _CACHE:
        from refign_amd import mfma
        from refign_amd.conv import patch_conv_tokens
        from refign_amd.seg import Attention
        C, heads, r, H, W = case
        torch.manual_seed(1000 + C + H)
        m = Attention(C, num_heads=heads, qkv_bias=True, sr_ratio=r).to(dev).eval()
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("bias"):
                    p.copy_(torch.randn_like(p) * 0.3)
            if r > 1:
                m.norm.weight.copy_(1.0 + 0.3 * torch.randn_like(m.norm.weight))
            x = (torch.randn(B, H * W, C, device=dev) * 1.5).to(dtype)
            n = m.norm(patch_conv_tokens(x, H, W, m.sr)) if r > 1 else x
            kv_chain = m.kv(n)
            fused = mfma.kv_packs(x, H, W, m.sr if r > 1 else None, m.norm if r > 1 else None, m.kv, want_kv=True, blocks_per_wg=3)
        assert fused is not None and kv_chain.dtype == dtype
        _CACHE[key] = (m, x, kv_chain, fused)
    return _CACHE[key]


def _fused(m, x, case, want_kv=True, blocks=0):
    from refign_amd import mfma
    C, heads, r, H, W = case
    with torch.no_grad():
        return mfma.kv_packs(x, H, W, m.sr if r > 1 else None, m.norm if r > 1 else None, m.kv, want_kv=want_kv,
                             blocks_per_wg=blocks)


def _written(kvr, kvt, heads):
    """The blocks the kernel owns: K's of the R-pack image, V's of the T-pack image, each (B, heads, nkblk * 4096) bytes."""
    return kvr.view(B, 2 * heads, -1)[:, :heads], kvt.view(B, 2 * heads, -1)[:, heads:]


def _fp64_chain(m, x, case):
    """The chain in fp64 on the same 16-bit inputs and 16-bit weights, no intermediate rounding."""
    C, heads, r, H, W = case
    dt = x.dtype
    w16 = lambda p: p.detach().to(dt).double()  # noqa: E731
    n = x.double()
    if r > 1:
        Hr, Wr = H // r, W // r
        pt = n.view(B, H, W, C)[:, :Hr * r, :Wr * r].reshape(B, Hr, r, Wr, r, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hr * Wr, r * r * C)
        y = pt @ w16(m.sr.weight).permute(0, 2, 3, 1).reshape(C, -1).t() + w16(m.sr.bias)
        n = F.layer_norm(y, (C,), m.norm.weight.detach().double(), m.norm.bias.detach().double(), m.norm.eps)
    return n @ w16(m.kv.weight).t() + w16(m.kv.bias)


@pytest.mark.parametrize("blocks", [3, 1, 0])
@pytest.mark.parametrize("case,dtype", PARAMS, ids=IDS)
def test_packs_equal_attn_pack_of_the_plain_output(dev, case, dtype, blocks):
    """Pack layout, exact: K's R-pack and V's T-pack equal rfn_attn_pack of the kernel's own plain kv output bit for bit, in pack
    buffers that held 0xFF before the call; the rows past Nkv and the block that makes nkblk even come out zero.  `blocks`: pack
    blocks per workgroup, 3 (tiles span images), 1, and the kernel's own choice."""
    from refign_amd import mfma
    C, heads, r, H, W = case
    m, x, _, _ = _setup(dev, case, dtype)
    arena = GuardArena(dev, 0xFF, 24 << 20)
    with arena.allocations():
        kvr, kvt, Nkv, nkblk, kv = _fused(m, x, case, blocks=blocks)
    arena.check()
    assert Nkv == (H // r) * (W // r) and nkblk % 2 == 0 and nkblk * 32 >= Nkv and tuple(kv.shape) == (B, Nkv, 2 * C)
    (pr, pt), _ = mfma._pack(kv, kv.stride(0), kv.stride(1), B, 2 * heads, Nkv, nkblk)
    k_got, v_got = _written(kvr, kvt, heads)
    k_want, v_want = _written(pr, pt, heads)
    assert torch.equal(k_got, k_want) and torch.equal(v_got, v_want)
    # R-pack [8 d-chunks][32 rows][16 bytes], T-pack [8 row quads][64 d][4 rows x 2 bytes]: the rows past Nkv
    kb = k_got.reshape(B, heads, nkblk, 8, 32, 16).permute(0, 1, 2, 4, 3, 5).reshape(B, heads, nkblk * 32, -1)
    vb = v_got.reshape(B, heads, nkblk, 8, 64, 4, 2).permute(0, 1, 2, 3, 5, 4, 6).reshape(B, heads, nkblk * 32, -1)
    assert nkblk * 32 > Nkv                                          # every case has padding rows
    assert int(kb[:, :, Nkv:].max()) == 0 and int(vb[:, :, Nkv:].max()) == 0
    assert int(kb[:, :, :Nkv].max()) > 0 and int(vb[:, :, :Nkv].max()) > 0


@pytest.mark.parametrize("case,dtype", PARAMS, ids=IDS)
def test_plain_output_equals_todays_chain(dev, case, dtype):
    """Values: the plain kv output against patch_conv_tokens -> LayerNorm -> kv Linear on the same weights.  The roundings are at
    the same points and the kernel keeps the NT GEMM's MFMA shape and ascending K order: zero differing elements.  The errors of
    both against an fp64 evaluation of the chain are printed for profiles/kvpath_parity.txt."""
    m, x, kv_chain, fused = _setup(dev, case, dtype)
    kv = fused[4]
    assert kv.shape == kv_chain.shape and bool(torch.isfinite(kv.float()).all())
    ndiff = int((kv != kv_chain).sum())
    ref = _fp64_chain(m, x, case)
    ef, ec = kv.double() - ref, kv_chain.double() - ref
    print(f"kvpath parity {case} {dtype}: differing {ndiff} of {kv.numel()}; rms fused {float(ef.pow(2).mean().sqrt()):.4e} chain "
          f"{float(ec.pow(2).mean().sqrt()):.4e}; max fused {float(ef.abs().max()):.4e} chain {float(ec.abs().max()):.4e}; "
          f"max|ref| {float(ref.abs().max()):.3f}")
    assert ndiff == 0
    assert torch.equal(_fused(m, x, case, blocks=1)[4], kv_chain)        # one pack block per workgroup: the same bits


@pytest.mark.parametrize("case,dtype", PARAMS, ids=IDS)
def test_attention_module_switch_on_and_off(dev, case, dtype, monkeypatch):
    """Attention.forward under no_grad with seg._KV_FUSED on and off, each against fp32: q and kv as the layers give them (16-bit),
    test_mfma_gpu's _ref_attention formulation and the projection in fp32 on the 16-bit weights.  Bound (test_mfma_gpu's for the
    forward): 4 eps16 max|ref| + 1e-3."""
    from refign_amd import seg
    C, heads, r, H, W = case
    m, x, kv_chain, _ = _setup(dev, case, dtype)
    with torch.no_grad():
        q = m.q(x).float()
        k, v = kv_chain.float().view(B, -1, 2, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
        a = ((q.view(B, -1, heads, 64).transpose(1, 2) @ k.transpose(-2, -1)) * m.scale).softmax(-1)
        o = (a @ v).transpose(1, 2).reshape(B, H * W, C)
        ref = F.linear(o, m.proj.weight.to(dtype).float(), m.proj.bias.to(dtype).float())
        bound = 4 * EPS[dtype] * float(ref.abs().max()) + 1e-3
        for on in (True, False):
            monkeypatch.setattr(seg, "_KV_FUSED", on)
            y = m(x, H, W)
            err = float((y.float() - ref).abs().max())
            print(f"kvpath attention {case} {dtype} fused={on}: err {err:.4e} bound {bound:.4e}")
            assert y.dtype == dtype and err <= bound, (on, err, bound)


@pytest.mark.parametrize("case", CASES, ids=[f"C{c[0]}r{c[2]}-{c[3]}x{c[4]}" for c in CASES])
@pytest.mark.parametrize("fill,blocks", [(0xFF, 3), (0x7B, 3), (0xFF, 1)])
def test_guard_band(dev, case, fill, blocks):
    """The token map placed in a poisoned arena (NaN / large values right behind its last element) and every output carved from
    it: nothing outside the outputs is written, and the result is what clean memory gives."""
    C, heads, r, H, W = case
    m, x, _, fused = _setup(dev, case, torch.bfloat16)
    arena = GuardArena(dev, fill, 24 << 20)
    xa = arena.place(x)
    with arena.allocations():
        kvr, kvt, Nkv, nkblk, kv = _fused(m, xa, case, blocks=blocks)
    arena.check()
    assert torch.equal(kv, fused[4])
    for got, want in zip(_written(kvr, kvt, heads), _written(fused[0], fused[1], heads)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("blocks", [3, 1])
@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[4]], ids=["C128r4", "C320r2", "C512r1"])
def test_graph_replay_sees_refreshed_weights(dev, case, blocks):
    """The call captured in a graph; the layer's weights changed in place and the cached 16-bit copies re-filled by
    params.refresh(); the replay equals an eager call with the new weights."""
    from refign_amd import params
    from refign_amd.seg import Attention
    C, heads, r, H, W = case
    torch.manual_seed(7)
    m = Attention(C, num_heads=heads, qkv_bias=True, sr_ratio=r).to(dev).eval()
    x = torch.randn(B, H * W, C, device=dev).to(torch.bfloat16)
    before = _fused(m, x, case, blocks=blocks)                      # (makes the cached copies; nothing is created under capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _fused(m, x, case, blocks=blocks)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.25).add_(0.01)
    params.refresh(list(m.parameters()))
    g.replay()
    torch.cuda.synchronize()
    eager = _fused(m, x, case, blocks=blocks)
    assert not torch.equal(eager[4], before[4])
    assert torch.equal(out[4], eager[4])
    for got, want in zip(_written(out[0], out[1], heads), _written(eager[0], eager[1], heads)):
        assert torch.equal(got, want)


def test_fallback_outside_the_domain(dev, monkeypatch):
    """A gradient-enabled call and an fp32 call take today's path: rfn_kv_path is not launched and the results are those of the
    switched-off module; the gradient-free 16-bit call launches it once."""
    from refign_amd import _lib, seg
    case = CASES[1]
    C, heads, r, H, W = case
    m, x, _, _ = _setup(dev, case, torch.bfloat16)
    calls = []
    real = _lib.call

    def counting(name, *a):
        calls.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", counting)
    results = {}
    for on in (True, False):
        monkeypatch.setattr(seg, "_KV_FUSED", on)
        del calls[:]
        xg = x.clone().requires_grad_(True)
        y_grad = m(xg, H, W)
        with torch.no_grad():
            y_f32 = m(x.float(), H, W)
        assert "rfn_kv_path" not in calls
        results[on] = (y_grad.detach(), y_f32)
    assert y_grad.requires_grad
    assert torch.equal(results[True][0], results[False][0]) and torch.equal(results[True][1], results[False][1])
    monkeypatch.setattr(seg, "_KV_FUSED", True)
    del calls[:]
    with torch.no_grad():
        m(x, H, W)
    assert calls.count("rfn_kv_path") == 1 and "rfn_patchify_tokens" not in calls and "rfn_attn_pack" not in calls

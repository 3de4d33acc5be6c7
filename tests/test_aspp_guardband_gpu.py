"""GPU: the two tap-sum wrappers of refign_amd/resnet.py (_tapsum, _tapsum_bwd: csrc/aspp.hip) under poisoned neighbours and
stale memory (tests/guardband.py, as it is).

Z, the bias rows and the incoming gradient live in a GuardArena; Y is allocated inside `arena.allocations()`, dZ is carved out of
the arena poisoned.  Z's padding columns [T Np, Nz) -- which the forward must not read -- and every byte around the operands hold
the fill.  For the fills 0x00 / 0xFF / 0x7B at the 7 x 9 and 25 x 13 maps (12 and 24 live taps) the guards stay untouched and the
outputs have the bits of the same calls on ordinary tensors."""
import pytest
import torch

from guardband import FILLS, GuardArena

pytestmark = pytest.mark.gpu

SHAPES = [(2, 7, 9), (1, 25, 13)]
DILATIONS = (6, 12, 18, 24)
K = 19


def _bits(t):
    return t.contiguous().view(torch.int16).clone()


def _operands(B, H, W, plan, dtype, dev):
    g = torch.Generator().manual_seed(31 * H + W)
    M = B * H * W
    Z = torch.randn(M, plan.Nz, generator=g).to(dtype).to(dev)
    bias = torch.zeros(len(DILATIONS), plan.Np)
    bias[:, :K] = torch.randn(len(DILATIONS), K, generator=g)
    gh = torch.zeros(B, H, W, plan.Np)
    gh[..., :K] = torch.randn(B, H, W, K, generator=g)
    return Z, bias.to(dev), gh.to(dtype).to(dev)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_tapsum_wrappers_in_the_poisoned_arena(dev, B, H, W, dtype):
    from refign_amd import resnet
    plan = resnet._Plan(H, W, DILATIONS, K)
    assert plan.Np == 24 and plan.T == {(7, 9): 12, (25, 13): 24}[(H, W)] and plan.Nz % 64 == 0 and plan.Nz == {(7, 9): 320, (25, 13): 576}[(H, W)]
    Z0, bias0, gh0 = _operands(B, H, W, plan, dtype, dev)
    M = B * H * W
    want_y = resnet._tapsum(Z0, plan, bias0, B, H, W, dtype)
    want_dz = resnet._tapsum_bwd(gh0, plan, torch.empty((M, plan.Nz), dtype=dtype, device=dev), B, H, W, dtype)
    torch.cuda.synchronize()
    # the forward does not read Z's padding columns: the same bits with NaN there
    Zn = Z0.clone()
    Zn[:, plan.T * plan.Np:] = float("nan")                  # (7 x 9: 32 columns; 25 x 13 has none)
    assert torch.equal(_bits(resnet._tapsum(Zn, plan, bias0, B, H, W, dtype)), _bits(want_y))
    # the backward writes every element of dZ, zeros in the padding columns
    assert not bool(want_dz[:, plan.T * plan.Np:].float().abs().any())
    for fill in FILLS:
        arena = GuardArena(dev, fill, 8 << 20)
        Z, bias, gh = arena.place(Z0), arena.place(bias0), arena.place(gh0)
        Z[:, plan.T * plan.Np:] = torch.full((2,), fill, dtype=torch.uint8, device=dev).view(dtype)   # stale memory there too
        with arena.allocations():
            y = resnet._tapsum(Z, plan, bias, B, H, W, dtype)
            dz = resnet._tapsum_bwd(gh, plan, torch.empty((M, plan.Nz), dtype=dtype, device=dev), B, H, W, dtype)
        arena.check()
        assert torch.equal(_bits(y), _bits(want_y)), f"fill 0x{fill:02X}: Y differs from the run on ordinary tensors"
        assert torch.equal(_bits(dz), _bits(want_dz)), f"fill 0x{fill:02X}: dZ differs from the run on ordinary tensors"

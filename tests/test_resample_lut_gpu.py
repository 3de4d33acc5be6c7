"""GPU: the label encode fused into the NEAREST resize (csrc/resample.hip: resize_nearest_lut_kernel through
resample.resize_nearest_u8(lut=)) against the numpy restatement resample.resize_nearest_reference(lut=), bit for bit.

Shapes: one pixel; a few pixels; both axes changing in opposite directions with odd sizes; the identity size (the encode alone)
with a row one pixel wider than a 256-lane workgroup; up-scaling across two and a bit workgroups per row.  The labels hold all
256 codes and the table is a random permutation with no fixed point, so that a skipped lookup (or a lookup applied twice) shows
at every pixel.  lut=None must stay what it was: the plain gather.  One case runs inside the guard-band arena
(tests/guardband.py): poisoned neighbours untouched, the same bits under the three fills."""
import numpy as np
import pytest
import torch
from guardband import FILLS, GuardArena

pytestmark = pytest.mark.gpu

SHAPES = [((1, 1), (1, 1)), ((5, 7), (3, 4)), ((37, 53), (53, 37)), ((64, 257), (64, 257)), ((3, 300), (2, 513))]


def labels(H, W):
    """every code 0 ... 255 where there is room, in an order that is no ramp"""
    rng = np.random.default_rng(H * 1000 + W)
    n = H * W
    a = np.concatenate([rng.permutation(256).astype(np.uint8) for _ in range(-(-n // 256))])[:n]
    return np.ascontiguousarray(a.reshape(H, W))


def table():
    """a permutation of the 256 codes without a fixed point: lut[c] != c and lut[lut[c]] != lut[c] for every c"""
    rng = np.random.default_rng(77)
    while True:
        lut = rng.permutation(256).astype(np.uint8)
        if not (lut == np.arange(256)).any():
            return lut


@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{s[0]}x{s[1]}to{d[0]}x{d[1]}" for s, d in SHAPES])
def test_encode_and_resize_equal_the_restatement(dev, src, dst):
    from refign_amd.resample import resize_nearest_reference, resize_nearest_u8
    lbl, lut = labels(*src), table()
    if src[0] * src[1] >= 256:
        assert len(np.unique(lbl)) == 256
    d_lbl, d_lut = torch.from_numpy(lbl).to(dev), torch.from_numpy(lut).to(dev)
    got = resize_nearest_u8(d_lbl, dst, lut=d_lut)
    assert got.dtype == torch.uint8 and tuple(got.shape) == dst and got.is_contiguous()
    want = resize_nearest_reference(lbl, dst, lut=lut)
    assert np.array_equal(got.cpu().numpy(), want)
    plain = resize_nearest_u8(d_lbl, dst)                           # lut=None: the gather as it was
    assert np.array_equal(plain.cpu().numpy(), resize_nearest_reference(lbl, dst))
    assert np.array_equal(lut[plain.cpu().numpy()], want) and not np.array_equal(plain.cpu().numpy(), want)
    assert torch.equal(d_lbl.cpu(), torch.from_numpy(lbl))          # the input is read only


def test_the_table_is_checked(dev):
    from refign_amd import _lib, resample
    from refign_amd._tensor import ptr
    lbl = torch.zeros((4, 4), dtype=torch.uint8, device=dev)
    for bad in (torch.zeros(255, dtype=torch.uint8, device=dev), torch.zeros(256, dtype=torch.int32, device=dev),
                torch.zeros(256, dtype=torch.uint8), torch.zeros(512, dtype=torch.uint8, device=dev)[::2]):
        with pytest.raises(RuntimeError, match="256-element uint8"):
            resample.resize_nearest_u8(lbl, (4, 4), lut=bad)
    ty = resample._device_tables("nearest", 4, 4, lbl.device)
    out = torch.empty_like(lbl)
    with pytest.raises(RuntimeError, match="null pointer"):         # the entry point itself: nothing is launched
        _lib.call("rfn_resize_nearest_lut_u8", lbl.device, ptr(lbl), 4, 4, 4, 4, ptr(ty), ptr(ty), None, ptr(out))


def test_in_the_poisoned_arena(dev):
    """37 x 53 -> 53 x 37 with input, table and output carved out of a guard-band arena, one byte past a 256-byte boundary as
    well: the guards stay as they were filled and the output has the restatement's bits under every fill"""
    from refign_amd.resample import resize_nearest_reference, resize_nearest_u8
    lbl, lut = labels(37, 53), table()
    want = torch.from_numpy(resize_nearest_reference(lbl, (53, 37), lut=lut))
    lbl0, lut0 = torch.from_numpy(lbl).to(dev), torch.from_numpy(lut).to(dev)
    for fill in FILLS:
        for aligned in (True, False):
            arena = GuardArena(dev, fill, 1 << 20)
            d_lbl, d_lut = arena.place(lbl0, 0 if aligned else 1), arena.place(lut0, 0 if aligned else 1)
            with arena.allocations():
                got = resize_nearest_u8(d_lbl, (53, 37), lut=d_lut)
            arena.check()
            assert torch.equal(got.cpu(), want), f"fill 0x{fill:02X}, {'aligned' if aligned else 'one byte past a boundary'}"

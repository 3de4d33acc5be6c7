"""GPU: the four gradient-clipping entry points under poisoned neighbours and stale memory (tests/guardband.py, as it is).

The flat buffer (n = 2 * 16384 + 7 with the ragged chunk table of test_gradclip_gpu.py), the table, the partials and -- inside
`arena.allocations()` -- the loss scaler's tensors, `out` and `coef` all live in a GuardArena.  For the fills 0x00 / 0xFF / 0x7B
and two placements of the buffer (on a 256-byte boundary and 16 bytes past one: the entry points ask for 16) the guards stay
untouched and every output has the bits of the same calls on ordinary tensors."""
import pytest
import torch

from guardband import FILLS, GuardArena
from test_gradclip_gpu import N_RAGGED, RAGGED, _bits, _chunk_mask, _content

pytestmark = pytest.mark.gpu

G, SCALE, MAX_NORM, CLAMP = 3, 16.0, 0.25, 0.5


def _run(flat, flat2, table, partials, alloc):
    """fused unscale-and-norm -> coefficient -> scale on `flat`, clamp on `flat2`; `alloc`: a context inside which the tensors
    the calls create are allocated."""
    from refign_amd.amp import LossScaler
    from refign_amd.steplog import GradNormPlan, grad_clamp_, grad_clip_coef, grad_scale_
    dev = flat.device
    plan = GradNormPlan([], G, N_RAGGED, dev)
    plan.chunks, plan.table, plan.partials = list(RAGGED), table, partials
    with alloc:
        scaler = LossScaler(dev, init_scale=SCALE)
        out = torch.empty(G + 1, dtype=torch.float64, device=dev)
        coef = torch.empty(2, dtype=torch.float32, device=dev)
        scaler.unscale_sqnorm_(flat, plan, out)
        grad_clip_coef(out, G, MAX_NORM, coef)
        grad_scale_(flat, coef)
        grad_clamp_(flat2, CLAMP)
    torch.cuda.synchronize(dev)
    return {"flat": _bits(flat), "found_inf": _bits(scaler.found_inf), "out": _bits(out), "coef": _bits(coef),
            "clamped": _bits(flat2)}


def test_clipping_entry_points_in_the_poisoned_arena(dev):
    import contextlib
    flat0 = _content("normal", N_RAGGED, dev, seed=6) * SCALE
    flat0[~_chunk_mask(RAGGED, N_RAGGED).to(dev)] = 0.0
    table0 = torch.tensor(RAGGED, dtype=torch.int64, device=dev)
    want = _run(flat0.clone(), flat0.clone(), table0, torch.zeros(len(RAGGED), dtype=torch.float64, device=dev),
                contextlib.nullcontext())
    assert float(want["coef"].view(torch.float32)[0]) < 1.0 and int(want["found_inf"]) == 0
    for skew in (0, 16):
        for fill in FILLS:
            arena = GuardArena(dev, fill, 4 << 20)
            flat, flat2 = arena.place(flat0, skew=skew), arena.place(flat0, skew=skew)
            table = arena.place(table0)
            partials = arena.place(torch.zeros(len(RAGGED), dtype=torch.float64, device=dev))
            got = _run(flat, flat2, table, partials, arena.allocations())
            arena.check()
            for k, b in got.items():
                assert torch.equal(b, want[k]), (f"fill 0x{fill:02X}, skew {skew}: output {k} differs from the run on ordinary "
                                                 f"tensors in {int((b != want[k]).sum())} of {b.numel()} elements")

"""GPU: the resized evaluation tail (evaltail.slide_argmax_confmat(..., out_size=): csrc/evaltail.hip,
rfn_slide_argmax_confmat_resized) under poisoned neighbours and stale memory (tests/guardband.py, as it is).

The ragged row and the shrinking row of test_evaltail_resize_gpu.py's table -- one pass through the footprint in LDS, and G output
pixels per pass.  Crop logits and target live in a GuardArena; the labels (torch.empty inside the wrapper) and the count matrix are
carved out of it inside `arena.allocations()`.  For the fills 0x00 / 0xFF / 0x7B and two placements (256-byte aligned, and one
element past it: the wrapper states no alignment) the guards stay untouched, labels and counts are bit-equal across all six runs
and equal to the run on ordinary tensors, and they pass the decided-pixel comparison with the float64 restatement."""
import pytest
import torch
from evaltail_resize_ref import case
from guardband import FILLS, GuardArena
from test_evaltail_gpu import count, random_target

pytestmark = pytest.mark.gpu

ROWS = [
    (2, 7, 97, 131, (64, 48), (33, 29), (16, 12), (150, 201), "f32"),            # ragged boxes and ragged output tiles
    (2, 19, 120, 200, (64, 64), (40, 48), (16, 16), (75, 131), "bf16"),          # the second stage shrinks
]


@pytest.mark.parametrize("B,C,H,W,crop,stride,lo,out,dtype", ROWS)
def test_resized_tail_in_the_poisoned_arena(dev, B, C, H, W, crop, stride, lo, out, dtype):
    from refign_amd import evaltail
    logits0, boxes, want, decided = case(B, C, H, W, crop, stride, lo, out, dtype)
    target0 = random_target(B, C, *out, 1)
    target0[~decided] = 255
    logits0, target0 = logits0.to(dev), target0.to(dev)
    cm0 = torch.zeros(C, C, dtype=torch.int64, device=dev)
    labels0 = evaltail.slide_argmax_confmat(logits0, boxes, (H, W), target0, 255, confmat=cm0, out_size=out)
    # the run on ordinary tensors against the restatement, on decided pixels
    assert torch.equal(labels0.cpu().long()[decided], want[decided])
    assert torch.equal(cm0.cpu(), count(target0, want, C)) and int(cm0.sum()) == int((target0 != 255).sum())
    for fill in FILLS:
        for aligned in (True, False):
            arena = GuardArena(dev, fill, 4 << 20)
            logits = arena.place(logits0, 0 if aligned else logits0.element_size())
            target = arena.place(target0, 0 if aligned else target0.element_size())
            with arena.allocations():
                cm = torch.zeros(C, C, dtype=torch.int64, device=dev)
                labels = evaltail.slide_argmax_confmat(logits, boxes, (H, W), target, 255, confmat=cm, out_size=out)
            arena.check()
            where = f"fill 0x{fill:02X}, {'aligned' if aligned else 'one element past a 256-byte boundary'}"
            assert torch.equal(labels, labels0), f"{where}: labels differ from the run on ordinary tensors"
            assert torch.equal(cm, cm0), f"{where}: counts differ from the run on ordinary tensors"

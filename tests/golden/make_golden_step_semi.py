"""tests/golden/make_golden_step_semi.py -- the step of the semi-supervised RobotCar recipe: one reference `training_step` of the
DAFormer MiT-B0 model of step_daformer_96x128 (make_golden_step.py: closed-form weights, augmentation off, seeds 77, global_step
3) on a batch with FOUR source samples next to TWO targets -- what CombinedDataModule hands the model under
`ignore_every_second_semantic_training_batch` when the coin shows tails (two labelled loaders, one pair loader, two samples
each).  The source half is make_batch(4, ...)'s, the target half make_batch(2, ...)'s.  Same keys as step_daformer_96x128.npz.
    python tests/golden/make_golden_step_semi.py      ->  step_daformer_semi_96x128.npz   (authoring container only)"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import as R  # noqa: E402
from make_golden_step import make_batch, run_reference, save  # noqa: E402

NAME, SIZE, BLK, N_SRC, N_TRG = "step_daformer_semi_96x128", (96, 128), 32, 4, 2


def semi_batch(make, *args):
    """`make(b, H, W, blk, ...)` twice: four source samples, two targets"""
    src, trg = make(N_SRC, *SIZE, BLK, *args), make(N_TRG, *SIZE, BLK, *args)
    return {"image_src": src["image_src"], "semantic_src": src["semantic_src"], "image_trg": trg["image_trg"],
            "image_ref": trg["image_ref"]}


if __name__ == "__main__":
    R.setup()
    torch.set_grad_enabled(True)
    model = run_reference(False)
    batch = semi_batch(make_batch)
    assert batch["image_src"].shape[0] == 4 and batch["image_trg"].shape[0] == 2
    random.seed(77); np.random.seed(77); torch.manual_seed(77)
    model.global_step = 3
    model.training_step(batch, 0)
    ema = float(sum(p.double().abs().sum() for p in model.ema_parameters()))
    live = float(sum(p.double().abs().sum() for p in model.live_parameters()))
    save(NAME, losses=np.array([model.logged["train_loss_src"], model.logged["train_loss_featdist_src"],
                                model.logged["train_loss_uda_trg"]]),
         grad_norms=np.array(model._rec.norms), ema_abs_sum=ema, live_abs_sum=live, size=np.array(SIZE))
    print("   ", model.logged, model._rec.norms)

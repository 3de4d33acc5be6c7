"""tests/golden/make_golden_refcheck.py -- fixtures that stand in for the reference at test time (authoring container only):

  refcorr_random.npz                 the compiled reference correlation (oracle/_ref) on two seeded random cases: inputs,
                                     arguments, forward output and both input gradients (tests/test_oracle_cpu.py)
  ref_checkpoint_hrda_mit_b0.json    the state_dict of the reference's HRDA model as make_golden_step builds it: key, shape
                                     and dtype in order, values of the non-floating entries (the floating ones are
                                     closed_form_fill of the key) -- what its strict load_state_dict checks
                                     (tests/test_checkpoint_cpu.py)"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))

# kH, kW, patchH, patchW, padH, padW, dilH, dilW, dpH, dpW, dH, dW
CORR_CASES = [(2, 7, 19, 23, (1, 1, 9, 9, 0, 0, 1, 1, 1, 1, 1, 1)),
              (1, 3, 14, 15, (3, 3, 7, 5, 2, 1, 1, 2, 2, 1, 2, 1))]


def refcorr():
    import build_ref
    ref = build_ref.load_prebuilt() or build_ref.build()
    rng = np.random.default_rng(7)
    arrays = {}
    for i, (B, C, H, W, args) in enumerate(CORR_CASES):
        a = rng.standard_normal((B, C, H, W)).astype(np.float32)
        b = rng.standard_normal((B, C, H, W)).astype(np.float32)
        out = ref.forward(torch.from_numpy(a), torch.from_numpy(b), *args).numpy()
        go = rng.standard_normal(out.shape).astype(np.float32)
        g1, g2 = ref.backward(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(go), *args)
        arrays.update({f"in1_{i}": a, f"in2_{i}": b, f"args_{i}": np.array(args, np.int64), f"out_{i}": out,
                       f"grad_out_{i}": go, f"grad_in1_{i}": g1.numpy(), f"grad_in2_{i}": g2.numpy()})
    path = os.path.join(HERE, "refcorr_random.npz")
    np.savez_compressed(path, **arrays)
    print(f"  wrote refcorr_random.npz  ({os.path.getsize(path) / 1024:.1f} kB)")


def ref_checkpoint():
    import _ref_import as R
    R.setup()
    import make_golden_step as G
    sd = G.run_reference(True).state_dict()
    entries = [{"key": k, "shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")} |
               ({} if v.is_floating_point() else {"value": v.tolist()}) for k, v in sd.items()]
    path = os.path.join(HERE, "ref_checkpoint_hrda_mit_b0.json")
    with open(path, "w") as f:
        json.dump(entries, f, indent=0)
    print(f"  wrote ref_checkpoint_hrda_mit_b0.json  ({len(entries)} entries)")


if __name__ == "__main__":
    refcorr()
    ref_checkpoint()

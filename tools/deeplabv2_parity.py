#!/usr/bin/env python3
"""tools/deeplabv2_parity.py -- the measured errors behind the bounds of tests/test_aspp_gpu.py and tests/test_deeplabv2_gpu.py,
written to profiles/deeplabv2_parity.txt (or --out):
  * DeepLabV2Head, fused (csrc/aspp.hip) and per-branch (four conv.Conv2d), against the fp64 reference: forward, dX, dW, db per
    shape and dtype, with the bound the test holds the fused path to;
  * ResNet-18 / 50 / 101-v1c under bf16 autocast on the kernels and on the torch library path against the CPU fp32 fixture:
    eval forward, train-mode forward, running statistics;
  * the UDA training step of tests/golden/step_deeplabv2_96x128.npz: fp32 on the library's convolutions (what the test asserts), fp32 on
    split-bf16 products and bf16 autocast (both recorded, not asserted).
    python tools/deeplabv2_parity.py [--out profiles/deeplabv2_parity.txt] [--no-step]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deeplabv2_parity.txt"))
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    import test_aspp_gpu as A
    import test_deeplabv2_gpu as D
    from conftest import golden
    dev = torch.device("cuda:0")
    lines = ["# DeepLabV2 family: measured errors (tools/deeplabv2_parity.py on " + torch.cuda.get_device_name(0) + ")", "",
             "## DeepLabV2Head against the fp64 reference of the four convolutions: max |error| per tensor",
             "## bound = 2 x per-branch error + 1 ulp of the tensor's dtype (finfo.eps x max |reference|); Z is 16-bit, Np = 24",
             f"{'B x C x H x W x classes':24s} {'dtype':5s} {'tensor':6s} {'fused':>10s} {'per-branch':>11s} {'bound':>10s} "
             f"{'fused-vs-pb':>12s}  verdict"]
    worst = 0.0
    for case in A.CASES:
        for dtype, name in zip(A.DTYPES, ("bf16", "f16")):
            for k, (e_fu, e_pb, bound, diff) in A.measure(case, dtype, dev).items():
                ok = e_fu <= bound and diff <= bound
                worst = max(worst, e_fu / bound, diff / bound)
                lines.append(f"{'x'.join(map(str, case)):24s} {name:5s} {k:6s} {e_fu:10.3e} {e_pb:11.3e} {bound:10.3e} {diff:12.3e}  "
                             f"{'within' if ok else 'OVER'}")
    lines += [f"largest error / bound over all rows: {worst:.3f}", "",
              "## ResNet-v1c under bf16 autocast against the CPU fp32 fixture (resnet_v1c_64x96.npz), per stage:",
              "## sample = max |a - ref| over the strided sample / max |ref|; abs-sum = relative error of sum |a|; kernels held to 2 x library",
              f"{'pass':28s} {'stage':5s} {'kernels sample':>15s} {'kernels abs-sum':>16s} {'library sample':>15s} {'library abs-sum':>16s}"]

    def rows(what, kern, lib):
        for i, ((ks, ka), (ls, la)) in enumerate(zip(kern, lib)):
            lines.append(f"{what:28s} {i:5d} {ks:15.3e} {ka:16.3e} {ls:15.3e} {la:16.3e}")

    for mt in ("resnet18_v1c", "resnet50_v1c", "resnet101_v1c"):
        kern, calls = D.eval_errors(mt, dev, True)
        lib, _ = D.eval_errors(mt, dev, False)
        rows(mt + " eval", kern, lib)
        lines.append(f"{'':28s} library fallbacks on the kernel path: {len(calls)}")
    kern, kstats, calls = D.train_errors(dev, True)
    lib, lstats, _ = D.train_errors(dev, False)
    rows("resnet101_v1c train", kern, lib)
    rows("  running_mean / running_var", [kstats["running_mean"], kstats["running_var"]], [lstats["running_mean"], lstats["running_var"]])
    lines.append(f"{'':28s} library fallbacks on the kernel path: {len(calls)}")
    if not args.no_step:
        import numpy as np
        g = golden("step_deeplabv2_96x128")
        lines += ["", "## one UDA training step (ResNet-101-v1c + DeepLabV2Head, 2 x 96 x 128) against the reference's (step_deeplabv2_96x128.npz)",
                  "## relative deviation of (loss_src, loss_featdist, loss_uda_trg) and of the four groups' gradient norms"]
        from refign_amd import resnet
        fmt = {"float_kind": lambda v: f"{v:.2e}"}
        for mode, autocast, fp32_library in (("fp32, library convolutions (asserted: 2e-3 / 2e-2)", False, True),
                                             ("fp32, split-bf16 products (recorded only)", False, False),
                                             ("bf16 autocast (recorded only)", True, True)):
            resnet.FP32_LIBRARY = fp32_library               # (False: what resnet.py's fp32 passes would be on conv.Conv2d)
            try:
                losses, norms, model, trainer = D.run_step(dev, autocast=autocast)
            finally:
                resnet.FP32_LIBRARY = True
            trainer.close()
            dl, dn = np.abs(losses / g["losses"] - 1), np.abs(norms / g["grad_norms"] - 1)
            lines.append(f"{mode:52s} losses {np.array2string(dl, formatter=fmt)}  gradient norms {np.array2string(dn, formatter=fmt)}")
            del model, trainer
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

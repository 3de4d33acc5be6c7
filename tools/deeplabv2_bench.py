#!/usr/bin/env python3
"""tools/deeplabv2_bench.py -- the DeepLabV2 family on the device, timed with device events (bf16 autocast throughout):

  head      DeepLabV2Head(2048 -> 19) at 2 x 2048 x 64 x 64 (the training crop's stage-4 map) and 1 x 2048 x 68 x 120
            (validation): forward alone (no_grad) and forward + backward, the fused tap-GEMM path (csrc/aspp.hip) against the
            per-branch path (four conv.Conv2d on the implicit-GEMM kernels, resnet.ASPP_FUSED = False) -- the baseline.  The two
            forms alternate round by round in one process; reported per form: the median over the rounds and their spread.
  backbone  ResNet-101-v1c (strides 1, 2, 1, 1; dilations 1, 1, 2, 4) at 2 x 3 x 512 x 512 and 1 x 3 x 540 x 960: eval under
            no_grad (folded BatchNorm) and train forward + backward; ms per pass and the fraction of the bf16 MFMA peak
            (2516.8 TFLOP/s dense) that the convolutions' FLOP count over that time amounts to -- a whole-pass rate, BatchNorm,
            ReLU and max-pool time included, not a kernel's share of peak.
  step      one refign_deeplabv2 training step: batch 2 (4 // 2 ranks), 512 x 512 crops, Trainer.step, ms per step after warm-up
            and the library-fallback summary.

    python tools/deeplabv2_bench.py [--rounds 7] [--iters 10] [--skip head|backbone|step ...] [--out profiles/deeplabv2_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16 = 2516.8e12
CFG = {"strides": (1, 2, 1, 1), "dilations": (1, 1, 2, 4)}
BF = torch.bfloat16


def timed(fn, iters):
    """ms per call of fn over `iters` back-to-back calls, from device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def ab(forms, rounds, iters, warmup=3):
    """forms: {name: fn}.  Alternating rounds -> {name: (median ms, min, max)}"""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            times[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def bench_head(lines, rounds, iters, dev):
    from refign_amd import resnet
    lines += ["## head: DeepLabV2Head(2048 -> 19, d = 6 / 12 / 18 / 24), bf16; ms per call, median [min .. max] over alternating rounds",
              f"{'shape':22s} {'pass':10s} {'fused':>26s} {'per-branch':>26s}  verdict"]
    wins = []
    for shape in ((2, 2048, 64, 64), (1, 2048, 68, 120)):
        torch.manual_seed(0)
        head = resnet.DeepLabV2Head(2048, 0, 19).to(dev).train()
        x = torch.randn(shape, device=dev).to(BF).requires_grad_()
        gy = torch.randn(shape[0], 19, *shape[2:], device=dev).to(BF)
        plist = list(head.parameters())

        def fwd(fused):
            def run():
                resnet.ASPP_FUSED = fused
                with torch.no_grad(), torch.autocast("cuda", dtype=BF):
                    head([x])
            return run

        def fwd_bwd(fused):
            def run():
                resnet.ASPP_FUSED = fused
                with torch.autocast("cuda", dtype=BF):
                    y = head([x])
                torch.autograd.grad(y, [x] + plist, gy)
            return run

        saved = resnet.ASPP_FUSED
        try:
            for what, mk in (("forward", fwd), ("fwd + bwd", fwd_bwd)):
                r = ab({"fused": mk(True), "per-branch": mk(False)}, rounds, iters)
                (fm, fl, fh), (pm, pl, ph) = r["fused"], r["per-branch"]
                win = fh < pl                                   # wins by more than the rounds' own spread: the ranges do not overlap
                wins.append(win)
                lines.append(f"{'x'.join(map(str, shape)):22s} {what:10s} {fm:8.3f} [{fl:7.3f} .. {fh:7.3f}] {pm:8.3f} [{pl:7.3f} .. {ph:7.3f}]  "
                             f"{'fused wins' if win else 'per-branch wins' if ph < fl else 'within the spread'} ({pm / fm:.2f}x)")
        finally:
            resnet.ASPP_FUSED = saved
        del head, x, gy
        torch.cuda.empty_cache()
    lines.append("decision: the fused form " + ("wins by more than the rounds' spread in every row: it is the default (ASPP_FUSED = True)"
                                                if all(wins) else "does NOT win every row by more than the rounds' spread: the default "
                                                "must be per-branch (ASPP_FUSED = False)"))
    lines.append("")


def conv_flops(model, x):
    """FLOPs of the convolutions of one forward of `model` on x (2 per multiply-add), counted by hooks from the shapes"""
    total = [0]

    def hook(m, inp, out):
        total[0] += 2 * out.numel() * m.in_channels // m.groups * m.kernel_size[0] * m.kernel_size[1]
    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        model(x)
    for h in hs:
        h.remove()
    return total[0]


def bench_backbone(lines, rounds, iters, dev):
    from refign_amd import mfma, resnet
    lines += ["## backbone: ResNet-101-v1c (strides 1 2 1 1, dilations 1 1 2 4), bf16; ms per pass, median [min .. max]; share of the bf16 MFMA",
              "## peak = convolution FLOPs (forward: 1x, forward + backward: 3x) / time / 2516.8 TFLOP/s -- a whole-pass rate",
              f"{'input':18s} {'pass':22s} {'ms':>26s} {'GFLOP':>9s} {'of peak':>8s}  fallbacks"]
    for shape in ((2, 3, 512, 512), (1, 3, 540, 960)):
        torch.manual_seed(0)
        m = resnet.ResNet("resnet101_v1c", zero_init_residual=False, **CFG).to(dev)
        x = torch.randn(shape, device=dev)
        m.train()                                                # (the folded eval pass does not go through the modules' hooks)
        flops = conv_flops(m, x)

        def ev():
            with torch.no_grad(), torch.autocast("cuda", dtype=BF):
                m(x)

        def tr():
            with torch.autocast("cuda", dtype=BF):
                y = m(x)[-1]
            torch.autograd.grad(y.float().mean(), plist)

        for what, fn, mult, mode in (("eval, no_grad", ev, 1, False), ("train, fwd + bwd", tr, 3, True)):
            m.train(mode)
            plist = [p for p in m.parameters() if p.requires_grad]
            mfma.LIBRARY_CALLS.clear()
            med, lo, hi = ab({"x": fn}, rounds, max(2, iters // 2))["x"]
            lines.append(f"{'x'.join(map(str, shape)):18s} {what:22s} {med:8.3f} [{lo:7.3f} .. {hi:7.3f}] {mult * flops / 1e9:9.1f} "
                         f"{100 * mult * flops / (med * 1e-3) / PEAK_BF16:7.2f}%  {mfma.library_summary() or 'none'}")
        del m, x
        torch.cuda.empty_cache()
    lines.append("")


def bench_step(lines, steps, dev):
    import copy
    import time
    from refign_amd import config, mfma
    from refign_amd.trainer import Trainer
    cfg = {"model": {"class_path": "models.DomainAdaptationSegmentationModel", "init_args": {
        "backbone_lr_factor": 0.1, "enable_fdist": True, "use_refign": True, "adapt_to_ref": False, "gamma": 0.25,
        "backbone": {"class_path": "models.backbones.ResNet", "init_args": {
            "pretrained": None, "model_type": "resnet101_v1c", "strides": [1, 2, 1, 1], "dilations": [1, 1, 2, 4]}},
        "head": {"class_path": "models.heads.DeepLabV2Head", "init_args": {"in_channels": 2048, "in_index": 3, "num_classes": 19}},
        "alignment_backbone": {"class_path": "models.backbones.VGG", "init_args": {"model_type": "vgg16", "pretrained": None,
                                                                                  "out_indices": [2, 3, 4]}},
        "alignment_head": {"class_path": "models.heads.UAWarpCHead", "init_args": {
            "in_index": [0, 1], "input_transform": "multiple_select", "estimate_uncertainty": True, "pretrained": None}},
        "loss": {"class_path": "models.losses.PixelWeightedCrossEntropyLoss"}}},
        "optimizer": {"class_path": "torch.optim.AdamW", "init_args": {"lr": 0.0006, "weight_decay": 0.01}},
        "lr_scheduler": {"class_path": "helpers.lr_scheduler.LinearWarmupPolynomialLR", "init_args": {
            "warmup_iters": 1500, "warmup_ratio": 0.000001, "power": 1.0, "max_steps": 40000}}}
    torch.manual_seed(0)
    model = config.build_model(copy.deepcopy(cfg), families=("deeplabv2",)).to(dev).train()
    trainer = Trainer(model, sync_batchnorm=True)
    b, H, W, blk = 2, 512, 512, 64
    g = torch.Generator().manual_seed(0)
    lbl = torch.randint(0, 19, (b, H // blk, W // blk), generator=g).repeat_interleave(blk, 1).repeat_interleave(blk, 2).contiguous()
    lbl[torch.rand(b, H, W, generator=g) < 0.05] = 255
    trg = torch.randn(b, 3, H, W, generator=g)
    batch = {"image_src": torch.randn(b, 3, H, W, generator=g).to(dev), "semantic_src": lbl.to(dev), "image_trg": trg.to(dev),
             "image_ref": (0.8 * torch.roll(trg, (3, -5), (2, 3)) + 0.2 * torch.randn(b, 3, H, W, generator=g)).to(dev)}

    def step():
        with torch.autocast("cuda", dtype=BF):
            trainer.step(batch)

    try:
        for _ in range(4):                                       # warm-up: two eager steps, then the passes' graph captures
            step()
        torch.cuda.synchronize()
        mfma.LIBRARY_CALLS.clear()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        finite = all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in model.logged.values())
        lines += ["## step: refign_deeplabv2 (ResNet-101-v1c + DeepLabV2Head, VGG-16 + UAWarpC align, feature distance), b = 2, 512 x 512, bf16",
                  f"{ms:.1f} ms per step over {steps} steps after 4 warm-up steps (host clock around a device synchronise); "
                  f"losses finite: {finite}", f"library fallbacks in the timed steps: {mfma.library_summary() or 'none'}", ""]
    finally:
        trainer.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip", nargs="*", default=[], choices=["head", "backbone", "step"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deeplabv2_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/deeplabv2_bench.py: a HIP device is required")
    dev = torch.device("cuda:0")
    lines = [f"# tools/deeplabv2_bench.py on {torch.cuda.get_device_name(0)}: rounds {args.rounds}, {args.iters} calls per round", ""]
    if "head" not in args.skip:
        bench_head(lines, args.rounds, args.iters, dev)
    if "backbone" not in args.skip:
        bench_backbone(lines, args.rounds, args.iters, dev)
    if "step" not in args.skip:
        bench_step(lines, args.steps, dev)
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

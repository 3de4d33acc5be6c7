#!/usr/bin/env python3
"""tools/eval_bench.py -- evaluation step of the bench model (HRDA MiT-B5, the
refign_hrda_star config: sliding-window inference, 1080x1080 crops, stride 420) on 1080x1920 images with 1080x1920 labels
and one IoU metric: images/s and peak memory.

--fused 1   the fused evaluation tail (refign_amd/evaltail.py: crop logits -> confusion counts in one kernel), what
            Trainer.validate runs by default
--fused 0   model.validation_step (up-sampled crops, image-sized sum / count, interpolation, arg-max, bincount)
--fused ab  both in one process on the same inputs: warm-up for both first, then --rounds rounds of --steps batches per path,
            alternating; peak-memory statistics are reset before every timed block
--kernel-only  no model: rfn_slide_argmax_confmat alone on random logits at the same geometry, HIP events around 50
            back-to-back launches (labels + counts, counts only, labels only, bf16 logits, one whole-image box)"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def kernel_only():
    from refign_amd import evaltail
    dev = torch.device("cuda:0")
    H, W, C = 1080, 1920, 19
    boxes3 = [(0, 1080, 0, 1080), (0, 1080, 420, 1500), (0, 1080, 840, 1920)]
    g = torch.Generator().manual_seed(0)

    def run(name, logits, boxes, target, want_labels, n=50):
        cm = torch.zeros(C, C, dtype=torch.int64, device=dev) if target is not None else None
        for _ in range(5):
            evaltail.slide_argmax_confmat(logits, boxes, (H, W), target, 255, want_labels, cm)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            evaltail.slide_argmax_confmat(logits, boxes, (H, W), target, 255, want_labels, cm)
        b.record()
        torch.cuda.synchronize()
        print(f"{name:58s} {a.elapsed_time(b) / n * 1e3:7.1f} us/launch (back to back)")

    for B in (1, 2):
        lg = (3 * torch.randn(3 * B, C, 270, 270, generator=g)).to(dev)
        y = torch.randint(0, C, (B, H, W), generator=g).to(dev)
        y[:, :40] = 255
        run(f"b={B} 3 boxes f32  labels + counts", lg, boxes3, y, True)
        run(f"b={B} 3 boxes f32  counts only", lg, boxes3, y, False)
        run(f"b={B} 3 boxes f32  labels only", lg, boxes3, None, True)
        run(f"b={B} 3 boxes bf16 counts only", lg.bfloat16(), boxes3, y, False)
    lg = (3 * torch.randn(1, C, 270, 480, generator=g)).to(dev)
    y = torch.randint(0, C, (1, H, W), generator=g).to(dev)
    run("b=1 whole image (one box, 270 x 480 logits) f32 counts only", lg, [(0, H, 0, W)], y, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--b", default="1", help="batch size, or a comma-separated list of them")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=None, help="timed blocks per path (default: 3 with --fused ab, else 1)")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--fused", choices=["0", "1", "ab"], default="1")
    args = ap.parse_args()
    if args.kernel_only:
        return kernel_only()
    from refign_amd import evaltail
    from refign_amd.metrics import IoU, MyMetricCollection
    dev = torch.device("cuda:0")
    wl = bench.RefignStep(dev, 1, 1234)
    model = wl.model.eval()
    model.valid_metrics = MyMetricCollection({"val_IoU": IoU(num_classes=model.head.num_classes, ignore_index=255)}).to(dev)
    print("slide inference:", model.use_slide_inference, model.inference_crop_size, model.inference_stride,
          "batched:", model.inference_batched_slide)
    paths = ["0", "1"] if args.fused == "ab" else [args.fused]
    rounds = args.rounds or (3 if args.fused == "ab" else 1)
    for b in [int(v) for v in args.b.split(",")]:
        x = torch.randn(b, 3, 1080, 1920, device=dev)
        y = torch.randint(0, 19, (b, 1080, 1920), device=dev)
        y[:, :40] = 255
        batch = {"image": x, "semantic": y}

        def step(path):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.precision == "bf16"):
                if path == "0":
                    model.validation_step(batch, 0, 0, src_name="")
                elif not evaltail.eval_step(model, model.valid_metrics, batch, ""):
                    raise RuntimeError("the fused evaluation step declined this batch")

        for path in paths:
            for _ in range(3):
                step(path)
        torch.cuda.synchronize()
        res = {p: {"ms": [], "host": [], "mem": 0} for p in paths}
        for _ in range(rounds):
            for path in paths:
                torch.cuda.reset_peak_memory_stats()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(path)
                host = (time.perf_counter() - t0) / args.steps    # what the host needs to enqueue a batch
                torch.cuda.synchronize()
                r = res[path]
                r["ms"].append((time.perf_counter() - t0) / args.steps * 1e3)
                r["host"].append(host * 1e3)
                r["mem"] = max(r["mem"], torch.cuda.max_memory_allocated())
        model.valid_metrics.reset()
        for path in paths:
            r = res[path]
            dt = sum(r["ms"]) / len(r["ms"])
            print(f"evaluation step fused={path} b={b} 1080x1920 ({args.precision}): {dt:.1f} ms/batch "
                  f"(blocks of {args.steps}: {', '.join(f'{v:.1f}' for v in r['ms'])}; host enqueue "
                  f"{sum(r['host']) / len(r['host']):.1f} ms), {b / dt * 1e3:.2f} images/s, "
                  f"max_memory_allocated {r['mem'] / 2 ** 20:.0f} MiB")


if __name__ == "__main__":
    main()

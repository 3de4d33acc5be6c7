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
            back-to-back launches (labels + counts, counts only, labels only, bf16 logits, one whole-image box), then
            rfn_slide_argmax_confmat_resized at the DAFormer `test:` geometry (below)
--preset daformer-test  the A/B legs on the `test:` section of refign_daformer.yaml instead: DAFormer MiT-B5, whole-image
            inference (one box) of a 540 x 960 image (logits 135 x 240), labels 1080 x 1920 -- forward(x, out_size) with a second
            interpolation, which the fused tail does inside its kernel.  --image-size H,W / --label-size Ho,Wo: other sizes"""
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

    def run(name, logits, boxes, target, want_labels, n=50, size=(H, W), out_size=None):
        cm = torch.zeros(C, C, dtype=torch.int64, device=dev) if target is not None else None
        for _ in range(5):
            evaltail.slide_argmax_confmat(logits, boxes, size, target, 255, want_labels, cm, out_size)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            evaltail.slide_argmax_confmat(logits, boxes, size, target, 255, want_labels, cm, out_size)
        b.record()
        torch.cuda.synchronize()
        print(f"{name:66s} {a.elapsed_time(b) / n * 1e3:7.1f} us/launch (back to back)")

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
    # rfn_slide_argmax_confmat_resized at the DAFormer `test:` geometry: image 540 x 960 (one box), logits 135 x 240, labels 1080 x 1920
    h2, w2 = PRESETS["daformer-test"]["image"]
    for B in (1, 2):
        lg = (3 * torch.randn(B, C, h2 // 4, w2 // 4, generator=g)).to(dev).bfloat16()
        y = torch.randint(0, C, (B, H, W), generator=g).to(dev)
        y[:, :40] = 255
        for what, target, want_labels in (("labels + counts", y, True), ("counts only", y, False), ("labels only", None, True)):
            run(f"b={B} resized: whole image {h2} x {w2}, labels {H} x {W}, bf16 {what}", lg, [(0, h2, 0, w2)], target, want_labels,
                size=(h2, w2), out_size=(H, W))


# geometry presets of the A/B legs: the bench workload, its inference mode, image and label size
PRESETS = {
    # refign_hrda_star.yaml: sliding-window inference on the full-size image, labels of the image's size
    "hrda": {"workload": "RefignStep", "slide": True, "image": (1080, 1920), "label": (1080, 1920)},
    # the `test:` section of refign_daformer.yaml: Resize(size=[540, 960], img_only=True), whole-image inference (one box, logits
    # 135 x 240), the label at the file's size
    "daformer-test": {"workload": "RefignDAFormerStep", "slide": False, "image": (540, 960), "label": (1080, 1920)},
}


def _pair(text):
    a, b = (int(v) for v in text.split(","))
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--b", default="1", help="batch size, or a comma-separated list of them")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=None, help="timed blocks per path (default: 3 with --fused ab, else 1)")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--fused", choices=["0", "1", "ab"], default="1")
    ap.add_argument("--preset", choices=sorted(PRESETS), default="hrda", help="model, inference mode, image and label size")
    ap.add_argument("--image-size", type=_pair, default=None, metavar="H,W", help="image size of the A/B legs (default: the preset's)")
    ap.add_argument("--label-size", type=_pair, default=None, metavar="Ho,Wo",
                    help="label size of the A/B legs (default: the preset's); another size than the image's: forward(x, out_size)")
    args = ap.parse_args()
    if args.kernel_only:
        return kernel_only()
    from refign_amd import evaltail
    from refign_amd.metrics import IoU, MyMetricCollection
    dev = torch.device("cuda:0")
    preset = PRESETS[args.preset]
    (H, W), (Ho, Wo) = args.image_size or preset["image"], args.label_size or preset["label"]
    wl = getattr(bench, preset["workload"])(dev, 1, 1234, H=H, W=W)
    model = wl.model.eval()
    model.use_slide_inference = preset["slide"]
    model.valid_metrics = MyMetricCollection({"val_IoU": IoU(num_classes=model.head.num_classes, ignore_index=255)}).to(dev)
    print("preset:", args.preset, "slide inference:", model.use_slide_inference, model.inference_crop_size, model.inference_stride,
          "batched:", model.inference_batched_slide, f"image {H}x{W} labels {Ho}x{Wo}")
    paths = ["0", "1"] if args.fused == "ab" else [args.fused]
    rounds = args.rounds or (3 if args.fused == "ab" else 1)
    for b in [int(v) for v in args.b.split(",")]:
        x = torch.randn(b, 3, H, W, device=dev)
        y = torch.randint(0, 19, (b, Ho, Wo), device=dev)
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
            print(f"evaluation step fused={path} b={b} image {H}x{W} labels {Ho}x{Wo} ({args.precision}): {dt:.1f} ms/batch "
                  f"(blocks of {args.steps}: {', '.join(f'{v:.1f}' for v in r['ms'])}; host enqueue "
                  f"{sum(r['host']) / len(r['host']):.1f} ms), {b / dt * 1e3:.2f} images/s, "
                  f"max_memory_allocated {r['mem'] / 2 ** 20:.0f} MiB")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tools/robotcar_ingest_bench.py -- the labelled RobotCar section (configs/cityscapes_robotcar/refign_*.yaml) from the decoded
file: a batch of 6 samples, decoded 1024 x 1024 -> dims 720 x 720 -> RandomRotation(10) -> RandomCrop(512) -> ColorJitter(0.25,
0.25, 0.25, hue 0.1) -> RandomHorizontalFlip -> conversion -> Normalize.  Times, per batch:
  device path   datastep.RotatedLabelledSampler.sample per sample, uploads of the decoded arrays included (`sampler`), and its
                pixel passes launched on ready operands: the two load-time resizes (`resize`), the label rotation
                (`rotate label`), and the fused pass -- gray sums + apply with the gather (`fused pass`).  The fused pass reads
                the 720 x 720 uint8 image (at most twice) and writes the fp32 crop; the rotated image, the jittered image
                and the mask are never stored.
  host          the same semantics on the CPU from the 720 x 720 arrays (the load-time resize is the reader's in the
                reference and left out): Pillow's rotate of image, label and mask, then the torch restatement of the chain
                (imported from tests/test_robotcar_ingest_gpu.py) on the crop, mirror, conversion, Normalize and the mask write.  Host clock.
Device events around `--reps` batches after `--warmup`.  The two paths are compared on the output of one batch (bit-equal).
    python tools/robotcar_ingest_bench.py [--reps 200] [--b 6] [--out profiles/robotcar_ingest_bench.txt]"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))              # the torch restatement of the chain lives with the tests
from refign_amd import datastep, photometric, resample  # noqa: E402

PLAN = {"dims": (720, 720), "crop_size": (512, 512), "cat_max_ratio": 1.0, "flip": 0.5, "mean": (0.485, 0.456, 0.406),
        "std": (0.229, 0.224, 0.225), "load_keys": ["image", "semantic"], "rotation": {"degrees": (-10.0, 10.0)},
        "jitter": {"brightness": (0.75, 1.25), "contrast": (0.75, 1.25), "saturation": (0.75, 1.25), "hue": (-0.1, 0.1),
                   "shuffle": False, "blur": None}}


def device_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def host_sample(img720, lbl720, angle, box, pp, flip):
    """Pillow + the torch restatement: -> (image fp32 (3, h, w), label int64 (h, w))"""
    from PIL import Image
    from test_robotcar_ingest_gpu import jitter, normalise
    top, left, h, w = box
    rot = Image.fromarray(img720).rotate(angle, Image.NEAREST, False, None, fillcolor=(0, 0, 0))
    rot_lbl = Image.fromarray(lbl720).rotate(angle, Image.NEAREST, False, None, fillcolor=255)
    mask = Image.new("1", (img720.shape[1], img720.shape[0]), 0).rotate(angle, Image.NEAREST, False, None, fillcolor=1)
    x = torch.from_numpy(np.array(rot)).permute(2, 0, 1)[:, top:top + h, left:left + w].contiguous()
    y = torch.from_numpy(np.array(rot_lbl))[top:top + h, left:left + w]
    m = torch.from_numpy(np.array(mask))[top:top + h, left:left + w]
    x = normalise(jitter(x, pp)[0], pp)
    if flip:
        x, y, m = x.flip(-1), y.flip(-1), m.flip(-1)
    x[m.expand_as(x)] = 0.0
    return x, y.to(torch.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--b", type=int, default=6)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("robotcar_ingest_bench: a HIP device is required")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    B, S, (Hd, Wd), (h, w) = args.b, args.size, PLAN["dims"], PLAN["crop_size"]
    decoded = [(rng.integers(0, 256, (S, S, 3), dtype=np.uint8), rng.integers(0, 19, (S, S), dtype=np.uint8)) for _ in range(B)]
    pinned = [(torch.from_numpy(i).pin_memory(), torch.from_numpy(l).pin_memory()) for i, l in decoded]
    sampler = datastep.RotatedLabelledSampler(lambda k: pinned[k], PLAN, dev)
    out_i = torch.empty((B, 3, h, w), dtype=torch.float32, device=dev)
    out_l = torch.empty((B, h, w), dtype=torch.int64, device=dev)

    def batch():
        for k in range(B):
            sampler.sample(k, out_i[k], out_l[k])

    # one batch on both paths, compared
    random.seed(0)
    torch.manual_seed(0)
    batch()
    got_i, got_l = out_i.cpu(), out_l.cpu()
    random.seed(0)
    torch.manual_seed(0)
    draws, img720, lbl720 = [], [], []
    for k in range(B):
        angle = float(torch.empty(1).uniform_(-10.0, 10.0).item())
        box, _ = datastep.draw_crop(Hd, Wd, (h, w))
        pp = photometric.draw(dict(PLAN["jitter"], mean=PLAN["mean"], std=PLAN["std"]))
        draws.append((angle, box, pp, random.random() < 0.5))
        img720.append(resample.resize_reference(decoded[k][0], (Hd, Wd)))
        lbl720.append(resample.resize_nearest_reference(decoded[k][1], (Hd, Wd)))
    differ = 0
    for k in range(B):
        x, y = host_sample(img720[k], lbl720[k], *draws[k])
        differ += int((x.view(torch.int32) != got_i[k].view(torch.int32)).sum()) + int((y != got_l[k]).sum())
    t0 = time.perf_counter()
    for _ in range(args.host_reps):
        for k in range(B):
            host_sample(img720[k], lbl720[k], *draws[k])
    host_ms = (time.perf_counter() - t0) * 1e3 / args.host_reps

    # the device passes on ready operands
    d_img = [p[0].to(dev) for p in pinned]
    d_lbl = [p[1].to(dev) for p in pinned]
    r_img = torch.stack([resample.resize_u8(x, (Hd, Wd)) for x in d_img])
    r_lbl = [resample.resize_nearest_u8(x, (Hd, Wd)) for x in d_lbl]
    params = [d[2] for d in draws]
    geometry = [photometric.RotateCrop(d[0], *d[1], d[3]) for d in draws]
    t_sampler = device_ms(batch, args.reps, args.warmup)
    t_resize = device_ms(lambda: [(resample.resize_u8(d_img[k], (Hd, Wd)), resample.resize_nearest_u8(d_lbl[k], (Hd, Wd)))
                                  for k in range(B)], args.reps, args.warmup)
    t_rotate = device_ms(lambda: [resample.rotate_nearest_u8(r_lbl[k], draws[k][0], 255) for k in range(B)], args.reps, args.warmup)
    t_fused = device_ms(lambda: photometric.apply(r_img, params, out=out_i, geometry=geometry), args.reps, args.warmup)
    moved = B * (2 * 3 * Hd * Wd + 12 * h * w)
    lines = ["profiles/robotcar_ingest_bench.txt -- python tools/robotcar_ingest_bench.py on one MI355X (device events; see the tool's "
             "docstring)", "",
             f"robotcar_ingest_bench: batch {B}, decoded {S} x {S} -> {Hd} x {Wd} -> {h} x {w}, device: {torch.cuda.get_device_name(0)}, "
             f"device events over {args.reps} batches after {args.warmup}",
             f"  device  sampler (uploads, draws, all passes)   {t_sampler:8.3f} ms / batch",
             f"  device  resize (image bilinear + label nearest) {t_resize:7.3f} ms / batch",
             f"  device  rotate label                          {t_rotate:8.3f} ms / batch",
             f"  device  fused pass (gray sums + apply, one call for the batch) {t_fused:8.3f} ms / batch  "
             f"({moved / 1e6:.1f} MB at most: {moved / (t_fused * 1e-3) / 1e9:.0f} GB/s)",
             f"  host    Pillow rotate x 3 + torch restatement, from the {Hd} x {Wd} arrays (host clock, {args.host_reps} batches) "
             f"{host_ms:9.1f} ms / batch",
             f"  outputs of one batch, device against host: {differ} differing values of {got_i.numel() + got_l.numel()}"]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

"""tools/ingest_bench.py -- from a DECODED image to its normalised crop in a batch slot, two ways, on one MI355X:

  (a) today's path   Pillow's resize on the host (the data set readers' Image.resize(dims, BILINEAR)), upload of the resized
                     (3, Hd, Wd) image, datastep.crop_flip_normalize;
  (b) this path      upload of the decoded (H, W, 3) image, resample.resize_crop_flip_normalize (resize fused into the crop);
  kernel             the fused kernel alone, from device events around a train of launches.

at the two load-time resizes of refign_daformer.yaml / refign_deeplabv2.yaml: Cityscapes 1024 x 2048 -> 512 x 1024 and ACDC
1080 x 1920 -> 540 x 960, each with a 512 x 512 crop.  Both paths start from pinned host memory and end with a device synchronise
(host clock around it); the two results are compared bit for bit before anything is timed.  Next to the kernel's time stand the
bytes of the source the crop's footprint covers (from the tables: first to last source row / column of the crop, x 3), i.e. what
the kernel has to read, and the fp32 bytes it writes.

    python tools/ingest_bench.py [--iters 200] [--out profiles/ingest_bench.txt]"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("cityscapes", (1024, 2048), (512, 1024), (0, 256, 512, 512)), ("acdc", (1080, 1920), (540, 960), (14, 224, 512, 512))]


def footprint_bytes(size, dims, box):
    """bytes of the decoded image under the crop: (source rows) x (source columns) x 3"""
    from refign_amd.resample import bilinear_tables
    (H, W), (Hd, Wd), (top, left, h, w) = size, dims, box
    ymin, yn, _ = bilinear_tables(H, Hd)
    xmin, xn, _ = bilinear_tables(W, Wd)
    rows = int(ymin[top + h - 1] + yn[top + h - 1] - ymin[top])
    cols = int(xmin[left + w - 1] + xn[left + w - 1] - xmin[left])
    return rows * cols * 3


def wall(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    t.sort()
    return 1e3 * t[len(t) // 2], 1e3 * t[len(t) // 10], 1e3 * t[-1 - len(t) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench: no GPU (a timing from anywhere else says nothing about the MI355X)")
    from PIL import Image
    warnings.filterwarnings("ignore", message="The given NumPy array is not writable")   # np.asarray(PIL image): read only here

    from refign_amd.datastep import crop_flip_normalize
    from refign_amd.resample import resize_crop_flip_normalize
    dev = torch.device("cuda:0")
    lines = [f"tools/ingest_bench.py --iters {args.iters} on {torch.cuda.get_device_name(0)}: decoded image -> normalised 512 x 512 crop",
             "wall times: median (10th .. 90th percentile) of single calls, each ended by a device synchronise", ""]
    rng = np.random.default_rng(0)
    for name, (H, W), (Hd, Wd), box in CASES:
        top, left, h, w = box
        # a smooth image with noise on top (a resize of pure noise is as good for the arithmetic, but not what a camera gives)
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([127 + 100 * np.sin(xx / 37.0 + c) * np.cos(yy / 23.0) for c in range(3)], -1)
        decoded = np.clip(base + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
        pil = Image.fromarray(decoded)
        pinned_full = torch.from_numpy(decoded).pin_memory()
        pinned_small = torch.empty((3, Hd, Wd), dtype=torch.uint8).pin_memory()
        out_a = torch.empty((3, h, w), dtype=torch.float32, device=dev)
        out_b = torch.empty((3, h, w), dtype=torch.float32, device=dev)

        def host_resize():
            pinned_small.copy_(torch.from_numpy(np.asarray(pil.resize((Wd, Hd), Image.BILINEAR))).permute(2, 0, 1))

        def path_a():
            host_resize()
            crop_flip_normalize(pinned_small.to(dev, non_blocking=True), None, top, left, h, w, False, out_a)

        def path_b():
            resize_crop_flip_normalize(pinned_full.to(dev, non_blocking=True), (Hd, Wd), top, left, h, w, False, out_b)

        path_a(), path_b()
        torch.cuda.synchronize()
        same = torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))
        t_resize = wall(host_resize, max(args.iters // 4, 10))
        t_a, t_b = wall(path_a, max(args.iters // 4, 10)), wall(path_b, args.iters)
        full_d = pinned_full.to(dev)
        for _ in range(10):
            resize_crop_flip_normalize(full_d, (Hd, Wd), top, left, h, w, False, out_b)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            resize_crop_flip_normalize(full_d, (Hd, Wd), top, left, h, w, False, out_b)
        e1.record()
        torch.cuda.synchronize()
        k_us = 1e3 * e0.elapsed_time(e1) / args.iters
        rd, wr = footprint_bytes((H, W), (Hd, Wd), box), 3 * h * w * 4
        lines += [f"{name}: {H} x {W} -> {Hd} x {Wd}, crop (top, left, h, w) = {box}; bits equal to path (a): {same}",
                  f"  (a) Pillow resize + upload {3 * Hd * Wd} B + crop_flip_normalize   {t_a[0]:8.3f} ms ({t_a[1]:.3f} .. {t_a[2]:.3f})"
                  f"   of which the host resize {t_resize[0]:.3f} ms ({t_resize[1]:.3f} .. {t_resize[2]:.3f})",
                  f"  (b) upload {3 * H * W} B + fused resize_crop_flip_normalize      {t_b[0]:8.3f} ms ({t_b[1]:.3f} .. {t_b[2]:.3f})",
                  f"  fused kernel alone (device events, {args.iters} launches back to back)  {k_us:8.2f} us per launch, launch gaps included;"
                  f" reads {rd} B of source under the crop, writes {wr} B: {(rd + wr) / k_us / 1e3:.1f} GB/s", ""]
        if not same:
            lines.append("  MISMATCH between the two paths")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if "MISMATCH" in text:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

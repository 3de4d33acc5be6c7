#!/usr/bin/env python3
"""tools/photometric_bench.py -- the photometric chain on image_prime at the shapes of configs/megadepth/uawarpc_stage2.yaml:
batch 6, 750 x 750 uint8, ColorJitter(0.6, 0.6, 0.6, hue 0) -> ChannelShuffle -> Gaussian blur (7 x 7, sigma 0.2 .. 2.0) ->
conversion and Normalize, with the blur forced on for 0, 1 and all 6 samples.  Times, per batch:
  device path   refign_amd.photometric: the mean pass (the zero fill and the gray sums) and the apply pass launched on ready
                records (`mean pass`, `apply pass`), and photometric.apply as called, with the pinned upload of the records
                (`total`).  Next to each kernel the bytes it must move -- the mean pass reads the uint8 image, the apply pass
                reads it again and writes the fp32 image: 2 x 1.69 MB read and 6.75 MB written per sample -- and what share of
                8 TB/s that is at the measured time.
  torch path    the same chain written as torch operations on the same device (the blur as a grouped conv2d in fp32)
  host          the same torch operations on the host CPU (host clock, `--host-reps` batches)
Device events around a window of `--reps` batches after `--warmup` (a launch takes tens of microseconds: the window is sized
in thousands).  The paths are compared on the output: without blur the grey levels must be equal, with blur they may differ by
one where the 49-tap sum lies at a half.
    python tools/photometric_bench.py [--reps 2000] [--b 6] [--size 750] [--out profiles/photometric_bench.txt]"""
import argparse
import os
import random
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refign_amd import _lib, photometric  # noqa: E402
from refign_amd._tensor import ptr, upload_async  # noqa: E402

STAGE2 = {"brightness": (0.4, 1.6), "contrast": (0.4, 1.6), "saturation": (0.4, 1.6), "shuffle": True,
          "blur": {"p": 0.0, "kernel_size": 7, "sigma": (0.2, 2.0)}, "mean": (0.485, 0.456, 0.406), "std": (0.229, 0.224, 0.225)}
PEAK_BYTES_PER_S = 8e12


def gray(img):
    r, g, b = img.unbind(0)
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(torch.uint8)


def blend(a, b, f):
    return (f * a + (1.0 - f) * b).clamp(0, 255).to(torch.uint8)


def torch_chain(img, p):
    """one sample in torch operations on img's device (the contrast mean: the exact integer sum divided once)"""
    x = img
    for s in p.order:
        f = p.factors[s] if s < 3 else None
        if f is None:
            continue
        if s == 0:
            x = blend(x, torch.zeros_like(x), f)
        elif s == 1:
            g = gray(x)
            x = blend(x, g.sum(dtype=torch.int64).to(torch.float32) / float(g.numel()), f)
        else:
            x = blend(x, gray(x).unsqueeze(0), f)
    x = x[list(p.perm)]
    if p.sigma is not None:
        k = p.kernel.to(img.device).view(1, 1, 7, 7).expand(3, 1, 7, 7)
        x = torch.round(F.conv2d(F.pad(x.to(torch.float32)[None], (3, 3, 3, 3), mode="reflect"), k, groups=3))[0].to(torch.uint8)
    mean = torch.tensor(p.mean, device=img.device).view(3, 1, 1)
    std = torch.tensor(p.std, device=img.device).view(3, 1, 1)
    return (x.to(torch.float32) / 255 - mean) / std


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--torch-reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--b", type=int, default=6)
    ap.add_argument("--size", type=int, default=750)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S = args.b, args.size
    random.seed(0)
    torch.manual_seed(0)
    drawn = [photometric.draw(STAGE2) for _ in range(B)]
    sigmas = [torch.empty(1).uniform_(0.2, 2.0).item() for _ in range(B)]
    img_cpu = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8)
    img = img_cpu.to(dev)
    out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    sums = torch.empty(B, dtype=torch.int64, device=dev)
    mb_image, mb_out = 3 * S * S / 1e6, 3 * S * S * 4 / 1e6
    lines = [f"photometric_bench: B={B} {S}x{S} uint8 -> fp32, the stage-2 plan; orders drawn {[p.order for p in drawn]}; "
             f"permutations {[p.perm for p in drawn]}",
             f"device: {torch.cuda.get_device_name(0)}; ms per batch of {B}, device events over {args.reps} batches after "
             f"{args.warmup} (torch path: {args.torch_reps} after 2; host: host clock over {args.host_reps})",
             f"bytes a kernel must move per sample: mean pass {mb_image:.2f} MB read; apply pass {mb_image:.2f} MB read + "
             f"{mb_out:.2f} MB written; share = bytes / time / 8 TB/s"]
    for n_blur in sorted({0, min(1, B), B}):
        params = [photometric.params_from(p.order, *p.factors, p.perm, sigmas[i] if i < n_blur else None, mean=p.mean, std=p.std)
                  for i, p in enumerate(drawn)]
        records = upload_async(torch.stack([torch.from_numpy(p.record()) for p in params]), torch.int32, dev)
        n_contrast = sum(p.contrast is not None for p in params)

        def mean_pass():
            _lib.call("rfn_photometric_gray_sums_u8", dev, ptr(img), ptr(records), B, S, S, ptr(sums))

        def apply_pass():
            _lib.call("rfn_photometric_apply_u8", dev, ptr(img), ptr(records), ptr(sums), B, S, S, ptr(out))

        ms_mean = device_ms(mean_pass, args.reps, args.warmup)
        ms_apply = device_ms(apply_pass, args.reps, args.warmup)
        ms_total = device_ms(lambda: photometric.apply(img, params, out=out), args.reps, args.warmup)
        ms_torch = device_ms(lambda: [torch_chain(img[i], p) for i, p in enumerate(params)], args.torch_reps, 2)
        t0 = time.perf_counter()
        for _ in range(args.host_reps):
            host = [torch_chain(img_cpu[i], p) for i, p in enumerate(params)]
        ms_host = (time.perf_counter() - t0) * 1e3 / args.host_reps
        got = photometric.apply(img, params)
        want = torch.stack([torch_chain(img[i], p) for i, p in enumerate(params)])
        # in grey levels: torch's device kernels divide by a constant through its reciprocal, so the last bit of a value may differ
        level_err = (got - want).abs() * torch.tensor(STAGE2["std"], device=dev).view(1, 3, 1, 1) * 255
        differ, worst = int((level_err > 0.5).sum()), float(level_err.max())
        host_differ = int((got.cpu() != torch.stack(host)).sum())
        b_mean, b_apply = n_contrast * mb_image * 1e6, B * (mb_image + mb_out) * 1e6
        lines += [f"blur on {n_blur} of {B} samples" + (f" (sigma {[round(s, 3) for s in sigmas[:n_blur]]})" if n_blur else ""),
                  f"  device path   mean pass (zero fill + gray sums, {n_contrast} samples with contrast)  {ms_mean:8.4f} ms   "
                  f"{b_mean / 1e6:6.2f} MB   {b_mean / (ms_mean * 1e-3) / PEAK_BYTES_PER_S * 100:5.1f} % of 8 TB/s",
                  f"                apply pass                                              {ms_apply:8.4f} ms   "
                  f"{b_apply / 1e6:6.2f} MB   {b_apply / (ms_apply * 1e-3) / PEAK_BYTES_PER_S * 100:5.1f} % of 8 TB/s",
                  f"                total: photometric.apply with the upload of the records {ms_total:8.4f} ms",
                  f"  torch path    the same chain as torch operations on the same device   {ms_torch:8.4f} ms   "
                  f"({ms_torch / ms_total:.1f} x the device path)",
                  f"  host          the same torch operations on the host CPU               {ms_host:8.2f} ms",
                  f"  agreement     {differ} of {got.numel()} values lie another grey level than the torch path's (largest "
                  f"difference {worst:.4f} levels); {host_differ} values differ in any bit from the host's"]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

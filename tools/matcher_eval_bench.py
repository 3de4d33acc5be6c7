"""tools/matcher_eval_bench.py -- what surrounds the matcher's forward in an evaluation run, two ways, on one MI355X.  One leg per
invocation (--leg ingest | metric), every time from device events around the timed call (median of --iters calls after warm-up):

  ingest   a MegaDepth-like decoded 1067 x 1600 image -> Resize(480, lanczos) = 480 x 719 -> normalise -> pad to 480 x 720
           (a) Pillow's LANCZOS resize on the host + upload of the resized image + crop_flip_normalize + F.pad;
           (b) upload of the decoded image + the fused kernel (resample.resize_crop_flip_normalize, filter="lanczos", pad_to=);
           (c) the fused kernel alone, the decoded image already on the device.
           (a) and (b) are compared bit for bit before anything is timed.
  metric   SparseEPE.update (metrics.py: the host-driven mirror of the reference) against the fused kernel
           (sparse_epe.sparse_epe_rows + SparseEPE.add_rows) at n = 1 000 and n = 8 192 correspondences, B = 1, 480 x 720, in ONE
           process.  The fused path must not come out slower: the tool exits 1 if it does.

    python tools/matcher_eval_bench.py --leg ingest [--iters 30] [--out profiles/matcher_eval_bench.txt]   (--out appends)"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZE, RESIZE, PAD = (1067, 1600), 480, (480, 720)


def timed(fn, iters, warmup=5):
    """median / 10th / 90th percentile in ms of single calls, each between two device events (the host part of a call that the
    device has to wait for is inside)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    t.sort()
    return t[len(t) // 2], t[len(t) // 10], t[-1 - len(t) // 10]


def fmt(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def leg_ingest(dev, iters):
    from PIL import Image
    warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
    from refign_amd.datastep import crop_flip_normalize
    from refign_amd.resample import resize_crop_flip_normalize, target_size
    H, W = SIZE
    h, w = target_size(H, W, RESIZE)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([127 + 100 * np.sin(xx / 37.0 + c) * np.cos(yy / 23.0) for c in range(3)], -1)
    decoded = np.clip(base + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
    pil = Image.fromarray(decoded)
    pinned_full = torch.from_numpy(decoded).pin_memory()
    pinned_small = torch.empty((3, h, w), dtype=torch.uint8).pin_memory()
    out_b = torch.empty((3,) + PAD, dtype=torch.float32, device=dev)
    res = {}

    def path_a():
        pinned_small.copy_(torch.from_numpy(np.asarray(pil.resize((w, h), Image.LANCZOS))).permute(2, 0, 1))
        x, _ = crop_flip_normalize(pinned_small.to(dev, non_blocking=True), None, 0, 0, h, w, False)
        res["a"] = torch.nn.functional.pad(x, (0, PAD[1] - w, 0, PAD[0] - h), value=0.0)

    def path_b():
        resize_crop_flip_normalize(pinned_full.to(dev, non_blocking=True), (h, w), 0, 0, h, w, False, out_b, filter="lanczos", pad_to=PAD)

    path_a(), path_b()
    torch.cuda.synchronize()
    same = torch.equal(res["a"].view(torch.int32), out_b.view(torch.int32))
    full_d = pinned_full.to(dev)
    t_a, t_b = timed(path_a, iters), timed(path_b, iters)
    t_c = timed(lambda: resize_crop_flip_normalize(full_d, (h, w), 0, 0, h, w, False, out_b, filter="lanczos", pad_to=PAD), iters)
    lines = [f"ingest: decoded {H} x {W} -> Resize({RESIZE}, lanczos) = {h} x {w} -> normalise -> pad to {PAD[0]} x {PAD[1]}; "
             f"bits of (a) and (b) equal: {same}",
             f"  (a) Pillow LANCZOS on the host + upload {3 * h * w} B + crop_flip_normalize + pad  {fmt(t_a)}",
             f"  (b) upload {3 * H * W} B + fused resize / normalise / pad kernel                 {fmt(t_b)}",
             f"  (c) the fused kernel alone (image on the device)                                {fmt(t_c)}"]
    return lines, same


def leg_metric(dev, iters):
    from refign_amd.metrics import SparseEPE
    from refign_amd.sparse_epe import sparse_epe_rows
    H, W = PAD
    g = torch.Generator().manual_seed(0)
    flow = ((torch.rand(1, 2, H, W, generator=g) - 0.5) * 12).to(dev)
    unc = torch.rand(1, 1, H, W, generator=g).to(dev)
    lines, ok = ["metric: SparseEPE (uncertainty_estimation=True), B = 1, 480 x 720, one process"], True
    for n in (1000, 8192):
        pt = torch.stack([torch.rand(n, generator=g) * (W + 8) - 4, torch.rand(n, generator=g) * (H + 8) - 4], 1)
        ps = [(pt + torch.randn(n, 2, generator=g) * 4).to(dev)]
        pt = [pt.to(dev)]
        host, fused = SparseEPE(uncertainty_estimation=True), SparseEPE(uncertainty_estimation=True)
        t_host = timed(lambda: host.update(flow, ps, pt, (H, W), unc), iters, warmup=3)
        t_fused = timed(lambda: fused.add_rows(sparse_epe_rows(flow, ps, pt, unc)), iters, warmup=3)
        t_kernel = timed(lambda: sparse_epe_rows(flow, ps, pt, unc), iters, warmup=3)
        a, b = host.compute(), fused.compute()
        err = max(abs(float(a[k]) - float(b[k])) / max(1.0, abs(float(a[k]))) for k in a)
        lines += [f"  n = {n}: SparseEPE.update {fmt(t_host)}   sparse_epe_rows + add_rows {fmt(t_fused)}   "
                  f"sparse_epe_rows alone {fmt(t_kernel)}   x{t_host[0] / t_fused[0]:.1f}; largest relative difference of the "
                  f"results {err:.1e}"]
        ok = ok and t_fused[0] <= t_host[0]
    if not ok:
        lines.append("  THE FUSED METRIC IS SLOWER THAN SparseEPE.update")
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("ingest", "metric"), required=True)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("matcher_eval_bench: at least 20 timed calls per figure")
    if not torch.cuda.is_available():
        raise SystemExit("matcher_eval_bench: no GPU (a timing from anywhere else says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    head = [f"tools/matcher_eval_bench.py --leg {args.leg} --iters {args.iters} on {torch.cuda.get_device_name(0)}",
            "times: median (10th .. 90th percentile) of single calls, each between two device events, after warm-up"]
    lines, ok = (leg_ingest if args.leg == "ingest" else leg_metric)(dev, args.iters)
    text = "\n".join(head + lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

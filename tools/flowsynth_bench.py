#!/usr/bin/env python3
"""tools/flowsynth_bench.py -- the matcher's warp supervision at the shapes of configs/megadepth/uawarpc_stage2.yaml: batch 6,
750 x 750 frames, CompositeFlow(hom / tps / afftps, add_elastic) and CenterCrop to 520 x 520.  Times, per batch:
  device path   refign_amd.flowsynth: the two blurs per sample (`blur`), the flow and warp kernels with ready fields
                (`flow+warp`), and all of it from the uploaded noise to the cropped batch (`total`)
  torch path    the same semantics written as torch operations on the same device: full-size grids, grid_sample, the blur as
                two conv2d passes over a reflect-padded field in fp32 (NOT the fp64 accumulation of the device path)
  host          the draws of the batch (draw_composite: two torch.rand(750, 750) per sample and the small linear algebra) and
                the upload of the noise fields
Device events around a window of `--reps` batches after `--warmup`; the host figure is a host clock.  The reference's own path
(the CPU data-loader workers with cv2) cannot be timed where there is no cv2 and is not.
    python tools/flowsynth_bench.py [--reps 10] [--b 6] [--size 750] [--crop 520] [--out profiles/flowsynth_bench.txt]"""
import argparse
import math
import os
import random
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refign_amd import flowsynth  # noqa: E402

STAGE2 = dict(include_transforms=["hom", "tps", "afftps"], random_alpha=0.26, random_s=0.45, random_tx=0.25, random_ty=0.25,
              random_t_hom=0.4, random_t_tps=0.4, random_t_tps_for_afftps=0.26, add_elastic=True)


def torch_blur(x, sigma):
    taps = torch.from_numpy(flowsynth.gaussian_taps(sigma)).to(x.device)
    r = taps.numel() // 2
    x = x.unsqueeze(1)                                                                   # (planes, 1, h, w)
    x = F.conv2d(F.pad(x, (r, r, 0, 0), mode="reflect"), taps.view(1, 1, 1, -1))
    return F.conv2d(F.pad(x, (0, 0, r, r), mode="reflect"), taps.view(1, 1, -1, 1)).squeeze(1)


def torch_synthesize(img, p, crop, dev):
    """one sample as the reference computes it, in torch operations on `dev`"""
    h, w = p.h, p.w
    t = p.theta39.to(dev)
    gx = torch.linspace(-1, 1, w, device=dev).view(1, w).expand(h, w)
    gy = torch.linspace(-1, 1, h, device=dev).view(h, 1).expand(h, w)

    def tps():
        kx = torch.tensor([k // 3 - 1.0 for k in range(9)], device=dev).view(9, 1, 1)
        ky = torch.tensor([k % 3 - 1.0 for k in range(9)], device=dev).view(9, 1, 1)
        d = (gx - kx) ** 2 + (gy - ky) ** 2
        d = torch.where(d == 0, torch.ones_like(d), d)
        u = d * torch.log(d)
        X = t[27] + t[28] * gx + t[29] * gy + (t[9:18].view(9, 1, 1) * u).sum(0)
        Y = t[30] + t[31] * gx + t[32] * gy + (t[18:27].view(9, 1, 1) * u).sum(0)
        return torch.stack([X, Y], -1).unsqueeze(0)

    def sentinel(g, by):
        m = ((by[..., 0] > -1) & (by[..., 0] < 1) & (by[..., 1] > -1) & (by[..., 1] < 1)).unsqueeze(3).float()
        return m * g + (m - 1) * 1e10

    if p.kind == "hom":
        k = gx * t[6] + gy * t[7] + t[8]
        grid = torch.stack([(gx * t[0] + gy * t[1] + t[2]) / k, (gx * t[3] + gy * t[4] + t[5]) / k], -1).unsqueeze(0)
    elif p.kind == "tps":
        grid = tps()
    else:
        aff = F.affine_grid(t[33:].view(1, 2, 3), [1, 3, h, w], align_corners=False)
        grid = aff
        if p.kind == "afftps":
            tg = tps()
            comp = F.grid_sample(sentinel(aff, aff).permute(0, 3, 1, 2), tg, align_corners=True).permute(0, 2, 3, 1)
            grid = sentinel(comp, tg)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, w).expand(h, w)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(h, 1).expand(h, w)
    base = torch.stack([xx, yy])

    def warp(x, flo):
        v = base + flo
        g = torch.stack([2.0 * v[0] / (w - 1) - 1.0, 2.0 * v[1] / (h - 1) - 1.0], -1).unsqueeze(0)
        out = F.grid_sample(x.unsqueeze(0), g, align_corners=True, padding_mode="zeros")[0]
        return out, (g[0, ..., 0] > -1) & (g[0, ..., 1] > -1) & (g[0, ..., 0] < 1) & (g[0, ..., 1] < 1)

    flow = torch.stack([(grid[0, ..., 0] + 1) * (w - 1) / 2.0, (grid[0, ..., 1] + 1) * (h - 1) / 2.0]) - base
    e = p.elastic
    if e is not None:
        field = torch_blur(e["noise"].to(dev, non_blocking=True) * 2 - 1, e["sigma"]) * e["alpha"]
        mask = torch.zeros(h, w, device=dev)
        for x, y, s, scale in e["bumps"]:
            g1 = torch.exp(-(torch.arange(h, device=dev) - x) ** 2 / (2 * s * s))
            g2 = torch.exp(-(torch.arange(w, device=dev) - y) ** 2 / (2 * s * s))
            mask = mask + torch.clamp(scale * (torch.outer(g1, g2) / (s * 2 * math.pi)), 0.0, 1.0)
        flow = warp(flow + base, field * torch.clamp(mask, 0.0, 1.0))[0] - base
    out, m = warp(img, flow)
    mp = flow + base
    border = (mp[0] >= 0) & (mp[0] <= w - 1) & (mp[1] >= 0) & (mp[1] <= h - 1)
    m = torch.where(border.sum() < h * w * 0.1, border, m)
    c = (lambda a: a) if crop is None else (lambda a: flowsynth.center_crop(a, crop).contiguous())
    return c(out), c(flow), c(m)


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--b", type=int, default=6)
    ap.add_argument("--size", type=int, default=750)
    ap.add_argument("--crop", type=int, default=520)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S, crop = args.b, args.size, (args.crop, args.crop)
    random.seed(0)
    torch.manual_seed(0)
    t0 = time.perf_counter()
    params = [flowsynth.draw_composite(S, S, **STAGE2) for _ in range(B)]
    t_draw = (time.perf_counter() - t0) * 1e3
    img = torch.randn(B, 3, S, S).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        up = [flowsynth.upload_async(p.elastic["noise"], torch.float32, dev) for p in params]
    torch.cuda.synchronize()
    t_up = (time.perf_counter() - t0) * 1e3 / args.reps
    del up

    def blur_only():
        return [flowsynth.elastic_field(p, dev) for p in params]

    ready = []
    for p, f in zip(params, blur_only()):
        e = dict(p.elastic, field=f)
        q = flowsynth.FlowParams(p.kind, S, S, p.theta_hom, p.theta_aff, p.theta_tps, e)
        ready.append(q)
    lines = [f"flowsynth_bench: B={B} {S}x{S} -> {crop[0]}x{crop[1]}, stage-2 CompositeFlow with add_elastic; transforms drawn: "
             f"{[p.kind for p in params]}; blur taps {[flowsynth.gaussian_taps(p.elastic['sigma']).size for p in params]}; "
             f"bumps kept {[len(p.elastic['bumps']) for p in params]}",
             f"device: {torch.cuda.get_device_name(0)}; ms per batch of {B}, device events over {args.reps} batches after {args.warmup}"]
    ms_total = device_ms(lambda: flowsynth.synthesize(img, params, crop), args.reps, args.warmup)
    ms_blur = device_ms(blur_only, args.reps, args.warmup)
    ms_fw = device_ms(lambda: flowsynth.synthesize(img, ready, crop), args.reps, args.warmup)
    ms_torch = device_ms(lambda: [torch_synthesize(img[i], p, crop, dev) for i, p in enumerate(params)], max(args.reps // 2, 1), 1)
    # the two paths agree (the torch path's blur accumulates in fp32: compared on the flow, loosely)
    d_flow = flowsynth.synthesize(img, params, crop)[1]
    t_flow = torch.stack([torch_synthesize(img[i], p, crop, dev)[1] for i, p in enumerate(params)])
    ok = (d_flow.abs() < 1e4) & (t_flow.abs() < 1e4)
    diff = float((d_flow - t_flow)[ok].abs().max())
    lines += [f"device path   total (upload of the noise, 2 blurs, flow, warp + crop per sample)  {ms_total:9.3f} ms",
              f"              blur (upload + 2 planes x 2 passes per sample, fp64 accumulation)    {ms_blur:9.3f} ms",
              f"              flow + warp kernels with ready fields                                {ms_fw:9.3f} ms",
              f"torch path    the same semantics as torch operations on the same device            {ms_torch:9.3f} ms   ({ms_torch / ms_total:.1f} x the device path)",
              f"host          draw_composite x {B} (once, host clock)                                {t_draw:9.3f} ms",
              f"              pinned upload of the {B} x 2 noise fields (host clock, synchronised)     {t_up:9.3f} ms",
              f"agreement     max |flow(device path) - flow(torch path)| on non-sentinel pixels     {diff:.3e} px",
              "not measured: the reference's CPU path (data-loader workers, cv2.GaussianBlur): there is no cv2 on the GPU machine."]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

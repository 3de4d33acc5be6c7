#!/usr/bin/env python3
"""tools/gradclip_bench.py: what gradient clipping costs (Trainer(gradient_clip_val=...); bench.py is not touched).

  python tools/gradclip_bench.py [--rounds 3] [--steps 20] [--parent DIR] [--out profiles/gradclip_bench.txt]

1. The passes alone, device events around REPS launches each, on a buffer of the bench model's size (343 MB) and on one of the
   matcher's: rfn_grad_sqnorm_groups, rfn_grad_clip_coef, rfn_grad_scale_f32 (at a coefficient below 1 and at exactly 1),
   rfn_grad_clamp_f32 and rfn_amp_unscale_sqnorm_groups_f32, each with its share of 8 TB/s from the bytes it has to move (4 per
   element for the norm, 8 for scale / clamp / the fused pass).
2. The matcher's training step at the conventions of tools/matcher_bench.py --trainer (b = 6, 520 x 520, the fp16 recipe) in
   alternating child processes, ROUNDS times: the parent commit (--parent DIR: a checkout of it, built beforehand; without it the
   leg is "not measured"), this tree with defaults, with a threshold that never clips (1e30) and with one that always does (1e-6).
   Every child runs under `timeout -k 10`; the first one that fails ends the run and nothing is started after it.
Needs a GPU: there is no fall-back, and nothing is written about a run that did not happen."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8e12                               # bytes / s
BENCH_ELEMS = 343_000_000 // 4 // 64 * 64  # the bench model's flat gradient buffer (profiles/steplog_ab.txt)
LEGS = (("parent", None), ("defaults", None), ("never clips", 1e30), ("always clips", 1e-6))


def passes(say, matcher_elems, reps=20):
    import torch
    sys.path.insert(0, ROOT)
    from refign_amd.amp import LossScaler
    from refign_amd.steplog import GradNormPlan, grad_clamp_, grad_clip_coef, grad_scale_, grad_sqnorm_groups
    dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3                 # us per launch

    say(f"# passes: device events around {reps} launches each; share = bytes the pass must move / 8 TB/s / time")
    for what, n in (("bench model's buffer", BENCH_ELEMS), ("matcher's buffer", matcher_elems)):
        flat = torch.randn(n, device=dev) * 1e-3
        plan = GradNormPlan([(0, n, 0)], 1, n, dev)
        out = torch.zeros(2, dtype=torch.float64, device=dev)
        coef, one = torch.tensor([0.999, 0.0], device=dev), torch.tensor([1.0, 0.0], device=dev)
        scaler, coef2 = LossScaler(dev, init_scale=1.0), torch.empty(2, device=dev)
        rows = [("norm (rfn_grad_sqnorm_groups)", 4, lambda: grad_sqnorm_groups(flat, plan, out)),
                ("coef (rfn_grad_clip_coef)", 0, lambda: grad_clip_coef(out, 1, 1.0, coef2)),
                ("scale, coefficient < 1", 8, lambda: grad_scale_(flat, coef)),
                ("scale, coefficient == 1", 0, lambda: grad_scale_(flat, one)),
                ("clamp (rfn_grad_clamp_f32)", 8, lambda: grad_clamp_(flat, 1.0)),
                ("fused unscale + norm", 8, lambda: scaler.unscale_sqnorm_(flat, plan, out)),
                ("unscale, then norm (two passes)", 12, lambda: (scaler.unscale_(flat), grad_sqnorm_groups(flat, plan, out)))]
        say(f"{what}: {n} elements, {4 * n / 1e6:.1f} MB")
        for name, per, fn in rows:
            us = timed(fn)
            share = f"{100 * per * n / PEAK / (us * 1e-6):5.1f} % of 8 TB/s ({per} B / element)" if per else "(no pass over the buffer)"
            say(f"  {name:34s} {us:9.1f} us   {share}")
        del flat, plan


def leg(name, clip, tree, steps, warmup):
    """One child: the matcher's step through Trainer at tools/matcher_bench.py's conventions -> one JSON line."""
    import time

    import torch
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tools"))
    import matcher_bench as mb
    from refign_amd import config
    from refign_amd.matching import warp
    from refign_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = config.build_model({"model": mb.MODEL, "optimizer": mb.OPTIM, "lr_scheduler": mb.SCHED}).to(dev).train()
    b, S = 6, 520
    g = torch.Generator().manual_seed(1)
    trg = torch.randn(b, 3, S, S, generator=g)
    ref = 0.8 * torch.roll(trg, (3, -5), (2, 3)) + 0.2 * torch.randn(b, 3, S, S, generator=g)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    flow = torch.stack((4 + 0.02 * (xx - S / 2) + 3 * torch.sin(2 * torch.pi * yy / S),
                        -3 - 0.015 * (yy - S / 2) + 2 * torch.cos(2 * torch.pi * xx / S))).expand(b, 2, S, S).contiguous()
    batch = {"image_ref": ref.to(dev), "image_trg": trg.to(dev), "flow_prime": flow.to(dev),
             "mask_prime": torch.ones(b, S, S, dtype=torch.bool, device=dev),
             "prime_trg_idx": torch.tensor([i % 2 for i in range(b)], device=dev)}
    with torch.no_grad():
        srcs = torch.stack([(batch["image_ref"], batch["image_trg"])[i % 2][i] for i in range(b)])
        batch["image_prime"] = warp(srcs, batch["flow_prime"])
    trainer = Trainer(model, precision=16, **({} if clip is None else {"gradient_clip_val": clip}))
    for it in range(warmup):
        trainer.step(batch, it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(steps):
        trainer.step(batch, it)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    res = {"leg": name, "ms_per_step": ms, "flat_elems": trainer.grads.flat.numel(), "skipped": trainer.scaler.skipped_steps(),
           "fast_launches": trainer.fast_step.launches, "loss": float(model.logged["train_matching_loss"])}
    if clip is not None:
        res.update(coef=float(trainer._clip.coef[0]), norm=float(trainer._clip.coef[1]))
    trainer.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20, help="steps before the clock: the fp16 scale backs off from 2^16 in them")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, built")
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None, help="a file with the compiler's resource-usage figures, put in front of the report")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--clip", type=float, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg is not None:
        return leg(args.leg, args.clip, args.tree, args.steps, args.warmup)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"# tools/gradclip_bench.py --rounds {args.rounds} --steps {args.steps} --warmup {args.warmup}"
        + (" --parent <checkout of the parent commit>" if args.parent else ""))
    if args.resources:
        with open(args.resources) as f:
            say(f.read().rstrip())
    say("# matcher training step through Trainer(precision=16), b = 6, 520 x 520 (tools/matcher_bench.py --trainer --precision fp16), "
        "host clock around the timed steps, ended by a device synchronise")
    got = {name: [] for name, _ in LEGS}
    for r in range(args.rounds):
        for name, clip in LEGS:
            if name == "parent" and not args.parent:
                continue
            tree = os.path.abspath(args.parent) if name == "parent" else ROOT
            cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", name, "--tree", tree,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)] + ([] if clip is None else ["--clip", repr(clip)])
            p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True)
            res = next((json.loads(ln) for ln in reversed(p.stdout.splitlines()) if ln.startswith("{") and '"leg"' in ln), None)
            if p.returncode != 0 or res is None:
                say(f"round {r + 1} leg '{name}': exit code {p.returncode}; stopping, nothing is started after a failure\n" + p.stderr[-3000:])
                write()
                sys.exit(1)
            got[name].append(res)
            say(f"round {r + 1}  {name:13s} {res['ms_per_step']:8.2f} ms/step   skipped fp16 steps {res['skipped']}, one-launch Adam "
                f"steps {res['fast_launches']}" + (f", last coefficient {res['coef']:.3e} at norm {res['norm']:.3e}" if "coef" in res else ""))
    say(f"\n{'ms/step':13s} {'median':>9s} {'min':>9s} {'max':>9s}")
    for name, _ in LEGS:
        v = [x["ms_per_step"] for x in got[name]]
        say(f"{name:13s} " + (f"{statistics.median(v):9.2f} {min(v):9.2f} {max(v):9.2f}" if v else "not measured"))
    ref = [x["ms_per_step"] for x in got["parent"]]
    dfl = [x["ms_per_step"] for x in got["defaults"]]
    if ref:
        inside = min(ref) <= statistics.median(dfl) <= max(ref)
        say(f"parent's own round-to-round spread: {min(ref):.2f} .. {max(ref):.2f} ms/step; defaults' median {statistics.median(dfl):.2f} ms/step "
            f"lies {'inside' if inside else 'OUTSIDE'} it")
    else:
        say("parent's own round-to-round spread: not measured")
    write()                                                 # (the step times are on file before the passes run)
    say("")
    passes(say, got["defaults"][0]["flat_elems"])
    write()


if __name__ == "__main__":
    main()

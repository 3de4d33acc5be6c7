"""A/B of the fp16 recipe against the bf16 step bench.py times, on one box, in alternating fresh processes.

  python tools/amp16_bench.py [--rounds 2] [--steps 20] [--warmup 5] [--height 1080 --width 1920 --pairs 2]

Leg "bf16": bench.RefignStep as bench.py runs it (bf16 autocast around Trainer.step).  Leg "fp16": the same model and batch,
driven by Trainer(precision=16) (fp16 autocast + device-side loss scaling).  Each leg reports ms/step, the dense library
calls (mfma.library_summary()), whether every logged loss stayed finite, and for fp16 the final loss scale and the number
of skipped steps.  The result goes to profiles/amp16_bench.json (and one JSON line per leg on stdout)."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(mode, steps, warmup, H, W, b):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from refign_amd import mfma
    from refign_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    s = bench.RefignStep(dev, b, 0, H=H, W=W, precision="bf16" if mode == "bf16" else "fp32")
    if mode == "fp16":
        s.trainer.close()
        s.trainer = Trainer(s.model, sync_batchnorm=True, precision=16)     # bench's autocast is off: the trainer's own
    for _ in range(s.prime_steps + warmup):
        s.step()
    torch.cuda.synchronize()
    mfma.LIBRARY_CALLS.clear()
    finite, ts = True, []
    for _ in range(steps):
        t0 = time.perf_counter()
        s.step()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
        finite &= all(math.isfinite(float(v)) for v in s.model.logged.values() if torch.is_tensor(v) or isinstance(v, float))
    ts.sort()
    out = {"mode": mode, "ms_per_step": sum(ts) / len(ts), "ms_median": ts[len(ts) // 2], "steps": steps, "warmup": warmup,
           "size": [H, W], "pairs": b, "losses_finite": bool(finite), "library_fallbacks": mfma.library_summary()}
    if s.trainer.scaler is not None:
        out["final_scale"] = s.trainer.scaler.get_scale()
        out["skipped_steps"] = s.trainer.scaler.skipped_steps()
    print("AMP16_LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--leg", choices=["bf16", "fp16"], help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per leg")
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.steps, a.warmup, a.height, a.width, a.pairs)
    legs = []
    for r in range(a.rounds):
        for mode in (("bf16", "fp16") if r % 2 == 0 else ("fp16", "bf16")):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", mode, "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--height", str(a.height), "--width", str(a.width), "--pairs", str(a.pairs)]
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.timeout)
            got = [json.loads(l_[len("AMP16_LEG "):]) for l_ in p.stdout.splitlines() if l_.startswith("AMP16_LEG ")]
            if p.returncode != 0 or not got:
                sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
                raise SystemExit(f"amp16_bench: leg {mode} of round {r} ended with status {p.returncode}")
            print(json.dumps(got[0]), flush=True)
            legs.append(got[0])
    mean = lambda m: sum(x["ms_per_step"] for x in legs if x["mode"] == m) / a.rounds  # noqa: E731
    summary = {"bf16_ms": mean("bf16"), "fp16_ms": mean("fp16"), "fp16_over_bf16": mean("fp16") / mean("bf16"), "legs": legs}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "amp16_bench.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps({k: v for k, v in summary.items() if k != "legs"}))


if __name__ == "__main__":
    main()

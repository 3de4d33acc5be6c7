#!/usr/bin/env python3
"""tools/steplog_bench.py: what the step log costs, on bench.py's workload (bench.py itself is not touched).

One leg -- bench.py in this process with every Trainer it builds given a logger:
  python tools/steplog_bench.py --log-every 50 [--log-dir DIR] -- --gpus 1 --steps 60 --warmup 5
  rocprofv3 --kernel-trace --stats -- python tools/steplog_bench.py --log-every 1 -- --gpus 1 --steps 5 --warmup 2
prints bench.py's JSON line with "log_every_n_steps" (0: no logger, bench.py as it is), "log_rows", "log_stalls" and
"flat_grad_bytes" (what the norm kernel reads per row) added.
The logger is a TensorBoardLogger writing to --log-dir (a temporary directory by default): the file is part of the cost.

The A/B -- legs in alternating child processes, ROUNDS times (no logger, every 50 steps, every step; with --parent DIR also
DIR/bench.py of another checkout, built beforehand, as the first leg of every round):
  python tools/steplog_bench.py --rounds 3 [--parent DIR] [--leg-timeout 300] [--out FILE] -- --gpus 1 --steps 60 --warmup 5
Every child runs under `timeout -k 10`; the first child that fails ends the run and nothing is started after it.  Prints
one line per child and a summary (median, min, max per leg; the spread of the reference leg's own repeats is the bar)."""
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _take(args, flag, default=None):
    if flag in args:
        i = args.index(flag)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


def leg(log_every, log_dir, bench_args):
    sys.path.insert(0, ROOT)
    for i, a in enumerate(bench_args):                     # (the switch does not travel to the ranks bench.py starts)
        if (a == "--gpus" and i + 1 < len(bench_args) and int(bench_args[i + 1]) != 1) or (a.startswith("--gpus=") and int(a[7:]) != 1):
            sys.exit("tools/steplog_bench.py: --gpus 1 only")
    made = []
    if log_every:
        from refign_amd import trainer as _trainer
        from refign_amd.steplog import TensorBoardLogger
        _init = _trainer.Trainer.__init__

        def init(self, *a, **k):
            k.setdefault("logger", TensorBoardLogger(log_dir or tempfile.mkdtemp(prefix="steplog_bench_"), name="bench"))
            k.setdefault("log_every_n_steps", log_every)
            _init(self, *a, **k)
            made.append(self)
        _trainer.Trainer.__init__ = init
    import bench
    _dumps = json.dumps

    def dumps(obj, *a, **k):
        if isinstance(obj, dict) and "metric" in obj:
            stalls = sum(t.flush_log() for t in made)      # (after the timed region: waits for the rows' events only)
            obj = dict(obj, log_every_n_steps=log_every, log_rows=sum(len(t.log_history) for t in made), log_stalls=stalls,
                       flat_grad_bytes=sum(4 * t.grads.flat.numel() for t in made))
        return _dumps(obj, *a, **k)

    bench.json.dumps = dumps
    sys.argv = ["bench.py"] + bench_args
    bench.main()
    for t in made:
        t.close()


def ab(rounds, parent, leg_timeout, out, bench_args):
    legs = ([("parent", [sys.executable, os.path.join(parent, "bench.py")] + bench_args, parent)] if parent else []) + \
        [(name, [sys.executable, os.path.abspath(__file__), "--log-every", str(n), "--"] + bench_args, ROOT)
         for name, n in (("no logger", 0), ("every 50 steps", 50), ("every step", 1))]
    got = {name: [] for name, _, _ in legs}
    lines = []
    pairs = int(bench_args[bench_args.index("--pairs-per-gpu") + 1]) if "--pairs-per-gpu" in bench_args else 2
    ms = lambda x: 1e3 * pairs / x["value"]                # bench.py reports image pairs per second  # noqa: E731

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# tools/steplog_bench.py --rounds {rounds}" + (" --parent <checkout of the parent commit>" if parent else "")
        + " -- " + " ".join(bench_args))
    for r in range(rounds):
        for name, cmd, cwd in legs:
            p = subprocess.run(["timeout", "-k", "10", str(leg_timeout)] + cmd, cwd=cwd, capture_output=True, text=True)
            res = None
            for ln in reversed(p.stdout.splitlines()):
                if ln.startswith("{") and '"metric"' in ln:
                    res = json.loads(ln)
                    break
            if p.returncode != 0 or res is None:
                say(f"round {r + 1} leg '{name}': exit code {p.returncode}; stopping, nothing is started after a failure\n"
                    + p.stderr[-3000:])
                _write(out, lines)
                sys.exit(1)
            got[name].append(res)
            say(f"round {r + 1}  {name:15s} {res['value']:9.3f} {res['unit']}  {ms(res):8.2f} ms/step"
                + (f"   rows {res['log_rows']}  stalls {res['log_stalls']}" if "log_rows" in res else ""))
    say(f"\n{'ms/step':15s} {'median':>9s} {'min':>9s} {'max':>9s}   rows  stalls   ({got[legs[0][0]][0]['metric']}; "
        f"{pairs} pairs per step)")
    for name, _, _ in legs:
        v = [ms(x) for x in got[name]]
        say(f"{name:15s} {statistics.median(v):9.3f} {min(v):9.3f} {max(v):9.3f}   "
            f"{sum(x.get('log_rows', 0) for x in got[name]):4d}  {sum(x.get('log_stalls', 0) for x in got[name]):6d}")
    ref = [ms(x) for x in got[legs[0][0]]]
    say(f"spread of '{legs[0][0]}' over its own {rounds} repeats: {min(ref):.2f} .. {max(ref):.2f} ms/step")
    _write(out, lines)


def _write(out, lines):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    args = sys.argv[1:]
    bench_args = []
    if "--" in args:
        i = args.index("--")
        args, bench_args = args[:i], args[i + 1:]
    rounds = _take(args, "--rounds")
    if rounds is not None:
        parent = _take(args, "--parent")
        ab(int(rounds), os.path.abspath(parent) if parent else None, int(_take(args, "--leg-timeout", "300")),
           _take(args, "--out"), bench_args)
    else:
        leg(int(_take(args, "--log-every", "0")), _take(args, "--log-dir"), bench_args + args)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tools/deterministic_bench.py [--deterministic] [--] bench.py args...: bench.py's workload with every Trainer it builds in
deterministic mode (Trainer(deterministic=True): refign_amd/determinism.py) -- the A/B form of a switch that is a constructor
argument.  Without --deterministic it is bench.py itself.  Prints bench.py's JSON line with a "deterministic" key added.

  python tools/deterministic_bench.py --deterministic -- --gpus 1 --steps 20 --warmup 5
  rocprofv3 --kernel-trace --stats -- python tools/deterministic_bench.py --deterministic -- --gpus 1 --steps 5 --warmup 2
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = sys.argv[1:]
det = "--deterministic" in args
args = [a for a in args if a not in ("--deterministic", "--")]
# one process only: with --gpus N > 1 bench.py starts N ranks of bench.py ITSELF, which would measure the default mode
for i, a in enumerate(args):
    if (a == "--gpus" and i + 1 < len(args) and int(args[i + 1]) != 1) or (a.startswith("--gpus=") and int(a[7:]) != 1):
        sys.exit("tools/deterministic_bench.py: --gpus 1 only (the switch does not travel to the ranks bench.py starts)")
if det:
    from refign_amd import trainer as _trainer
    _init = _trainer.Trainer.__init__

    def init(self, *a, **k):
        k.setdefault("deterministic", True)
        _init(self, *a, **k)
    _trainer.Trainer.__init__ = init
import bench  # noqa: E402

_dumps = json.dumps


def dumps(obj, *a, **k):
    if isinstance(obj, dict) and "metric" in obj:
        obj = dict(obj, deterministic=det)
    return _dumps(obj, *a, **k)


bench.json.dumps = dumps
sys.argv = ["bench.py"] + args
bench.main()

"""Wall time of Trainer.save_checkpoint / load_checkpoint and the file size for the bench model (bench.py's RefignStep:
MiT-B5 + HRDA, 1080 x 1920, bf16) after two training steps, so that the optimizer holds its moments.
Usage: python tools/ckpt_bench.py OUT_DIR [--steps N]; prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--steps", type=int, default=2)
    args = ap.parse_args()
    import bench
    dev = torch.device("cuda:0")
    wl = bench.RefignStep(dev, 1, 0)
    for _ in range(args.steps):
        wl.step()
    torch.cuda.synchronize()
    path = os.path.join(args.out_dir, "last.ckpt")
    res = {"model": wl.name, "steps_before_save": args.steps}
    for rep in range(2):
        t0 = time.perf_counter()
        wl.trainer.save_checkpoint(path)
        res[f"save_s_{rep}"] = round(time.perf_counter() - t0, 3)
    res["file_bytes"] = os.path.getsize(path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    count = lambda obj: sum(t.numel() * t.element_size() for t in _tensors(obj))  # noqa: E731
    res["state_dict_bytes"] = count(ck["state_dict"])
    res["optimizer_bytes"] = count(ck["optimizer_states"])
    res["trainable_params"] = sum(p.numel() for g in wl.trainer.optimizer.param_groups for p in g["params"])
    del ck
    for rep in range(2):
        t0 = time.perf_counter()
        wl.trainer.load_checkpoint(path)
        torch.cuda.synchronize()
        res[f"load_s_{rep}"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    wl.step()
    torch.cuda.synchronize()
    res["first_step_after_load_s"] = round(time.perf_counter() - t0, 3)
    wl.trainer.close()
    os.unlink(path)
    print(json.dumps(res), flush=True)


def _tensors(obj):
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors(v)


if __name__ == "__main__":
    main()

"""tools/matching_datamodule_bench.py -- what MatchingDataModule.train_batches() adds to the matcher's training step, on one
MI355X, over a MegaDepth tree this tool writes itself: JPEG files of 1067 x 1600 (MegaDepth's typical size), one scene whose
pairs all qualify, under uawarpc_stage2.yaml's training section (dims 750 x 750, crop 520 x 520, the photometric chain, the
composite flow with the elastic field, exchange probability 0.5), b = 6, the fp16 recipe.

ms per Trainer.fit step, --rounds times in turn:
  (a) from batches kept on the device -- the step tools/matcher_bench.py --trainer --precision fp16 times, on batches of this
      loader; the spread of (a) between the rounds is the run-to-run spread the other two are held against
  (b) from train_batches() with prefetch=2 at num_workers=4
  (c) from train_batches() with prefetch=0
and per batch: the core-milliseconds of decoding (summed over the threads), the host time inside next() with its parts (waiting
for a file, the draws, the rest: uploads and launches), and the device time of one batch's ingest (events around next() on an
idle device with the files already decoded: uploads, resizes, photometric chain, flow synthesis, and the host gaps between
their launches -- an upper bound).  If (b) is slower than (a) by more than (a)'s spread, the last line names the largest part
of next() in (b).  No threshold.

--graph: the same with Trainer(graph_step=True) -- the replayed step leaves the host thread to next().

    python tools/matching_datamodule_bench.py [--steps 12] [--rounds 3] [--graph] [--out profiles/matching_datamodule_bench.txt]"""
import argparse
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from matcher_bench import MODEL, OPTIM, SCHED  # noqa: E402

_PIPE = "data_modules.transforms."
N_FILES, H, W = 12, 1067, 1600
SCENE = "0000"


def _image(rng, h, w):
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 100 * np.sin(x / 37.0 + c) * np.cos(y / 23.0) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def write_tree(data_dir):
    from PIL import Image
    rng = np.random.default_rng(0)
    root = os.path.join(data_dir, "MegaDepth")
    paths, sizes = np.empty(N_FILES, dtype=object), []
    points = np.empty(N_FILES, dtype=object)
    for i in range(N_FILES):
        rel = f"Undistorted_SfM/{SCENE}/images/{i:04d}.jpg"
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        Image.fromarray(_image(rng, H, W)).save(os.path.join(root, rel), quality=92)
        sizes.append(os.path.getsize(os.path.join(root, rel)))
        paths[i] = rel
        points[i] = {k: np.array([rng.uniform(0, W - 1), rng.uniform(0, H - 1)]) for k in range(200)}
    os.makedirs(os.path.join(root, "scene_info"))
    overlap = np.full((N_FILES, N_FILES), 0.5)
    np.fill_diagonal(overlap, -1.0)
    np.savez(os.path.join(root, "scene_info", f"{SCENE}.0.npz"), image_paths=paths, depth_paths=paths.copy(),
             points3D_id_to_2D=points, overlap_matrix=overlap)
    os.makedirs(os.path.join(root, "lists"))
    with open(os.path.join(root, "lists", "train_scenes_MegaDepth.txt"), "w") as f:
        f.write(SCENE + "\n")
    return sizes


def data_cfg(num_workers, b):
    keys = {"apply_keys": ["image_prime"]}
    transforms = [
        {"class_path": _PIPE + "ToTensor"},
        {"class_path": _PIPE + "ColorJitter", "init_args": dict(keys, brightness=0.6, contrast=0.6, saturation=0.6, hue=0)},
        {"class_path": _PIPE + "ChannelShuffle", "init_args": dict(keys)},
        {"class_path": _PIPE + "RandomGaussianBlur", "init_args": dict(keys, p=0.2, kernel_size=7, sigma=[0.2, 2.0])},
        {"class_path": _PIPE + "ConvertImageDtype"}, {"class_path": _PIPE + "Normalize"},
        {"class_path": _PIPE + "CompositeFlow", "init_args": dict(
            keys, include_transforms=["hom", "tps", "afftps"], random_alpha=0.26, random_s=0.45, random_tx=0.25, random_ty=0.25,
            random_t_hom=0.4, random_t_tps=0.4, random_t_tps_for_afftps=0.26, parameterize_with_gaussian=False, add_elastic=True)},
        {"class_path": _PIPE + "CenterCrop", "init_args": {"size": [520, 520]}}]
    return {"data": {"class_path": "data_modules.CombinedDataModule", "init_args": {"batch_size": b, "num_workers": num_workers, "load_config": {
        "train": {"MegaDepth": {"store_scene_info_in_memory": True, "exchange_images_with_proba": 0.5, "dims": [750, 750],
                                "load_keys": ["image", "image_ref", "image_prime"], "transforms": transforms}}}}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--b", type=int, default=6)
    ap.add_argument("--graph", action="store_true", help="Trainer(graph_step=True): the step replays from one hipGraph, which leaves "
                                                         "the host thread to next()")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("matching_datamodule_bench: no GPU (a timing from anywhere else says nothing about the MI355X)")
    from refign_amd import config
    from refign_amd.datamodule import MatchingDataModule
    from refign_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    data_dir = tempfile.mkdtemp(prefix="refign_match_bench_")
    try:
        sizes = write_tree(data_dir)
        random.seed(0); np.random.seed(0); torch.manual_seed(0)
        model = config.build_model({"model": MODEL, "optimizer": OPTIM, "lr_scheduler": SCHED}).to(dev).train()
        trainer = Trainer(model, precision=16, scaler_args={"init_scale": 2.0 ** 4}, graph_step=args.graph)

        def timed(batches):
            start = int(model.global_step)
            trainer.fit(batches, max_steps=start + 3, save_last=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.fit(batches, max_steps=start + 3 + args.steps, save_last=False)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / args.steps

        dm = MatchingDataModule(data_cfg(0, args.b), data_dir, dev, prefetch=0)
        it = dm.train_batches()
        kept = [{k: v.clone() for k, v in next(it).items()} for _ in range(2)]
        dm.close()
        names = ("(a) batches kept on the device", "(b) train_batches(), prefetch 2, num_workers 4", "(c) train_batches(), prefetch 0")
        ms = {n: [] for n in names}
        parts = {}
        for _ in range(args.rounds):
            ms[names[0]].append(timed(kept))
            for name, prefetch, workers in ((names[1], 2, 4), (names[2], 0, 0)):
                dm = MatchingDataModule(data_cfg(workers, args.b), data_dir, dev, prefetch=prefetch)
                it = dm.train_batches()
                ms[name].append(timed(it))
                n = it.batches
                parts[name] = tuple(1e3 * v / n for v in (it.decode_seconds, it.host_seconds, it.wait_seconds, it.draw_seconds))
                dm.close()
        # one batch's ingest on an idle device, its files decoded ahead
        dm = MatchingDataModule(data_cfg(4, args.b), data_dir, dev, prefetch=2)
        it = dm.train_batches()
        for _ in range(3):
            next(it)
        ingest = []
        for _ in range(6):
            time.sleep(0.3)                                  # the next batches' files get decoded meanwhile
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            next(it)
            e1.record()
            torch.cuda.synchronize()
            ingest.append(e0.elapsed_time(e1))
        dm.close()
        how = f" --graph (step graph captured: {trainer.step_graph.captured()})" if args.graph else ""
        trainer.close()
        lines = [f"tools/matching_datamodule_bench.py --steps {args.steps} --rounds {args.rounds} --b {args.b}{how} on {torch.cuda.get_device_name(0)}",
                 f"tree: {N_FILES} JPEG files of {H} x {W}, {np.mean(sizes) / 1e6:.2f} MB on average; a batch decodes {2 * args.b} of them",
                 f"section: uawarpc_stage2.yaml's (dims 750 x 750, crop 520 x 520, elastic field), b = {args.b}, precision 16", "",
                 f"Trainer.fit, ms per step over {args.steps} steps after 3, per round, and their mean:"]
        for n in names:
            lines.append(f"  {n:52s} " + "  ".join(f"{v:7.1f}" for v in ms[n]) + f"   mean {np.mean(ms[n]):7.1f}")
        spread = max(ms[names[0]]) - min(ms[names[0]])
        lines += [f"  run-to-run spread of (a): {spread:.1f} ms", "", "per batch, ms (last round):"]
        for n in names[1:]:
            dec, host, wait, draw = parts[n]
            lines.append(f"  {n:52s} decode {dec:7.1f} core-ms   next() {host:7.1f} = waiting for files {wait:7.1f} + draws {draw:6.1f} "
                         f"+ uploads and launches {host - wait - draw:6.1f}")
        lines.append(f"  one batch's ingest on an idle device (events around next(), files decoded ahead): "
                     f"{np.median(ingest):.1f} ms median of {len(ingest)}")
        gap = np.mean(ms[names[1]]) - np.mean(ms[names[0]])
        if gap > spread:
            dec, host, wait, draw = parts[names[1]]
            which = max((("waiting for decoded files (decode)", wait), ("the draws", draw), ("uploads and launches", host - wait - draw)),
                        key=lambda kv: kv[1])
            lines += ["", f"(b) is {gap:.1f} ms per step slower than (a), more than (a)'s spread: the largest part of next() is {which[0]}, "
                          f"{which[1]:.1f} ms per batch."]
        else:
            lines += ["", f"(b) - (a) = {gap:.1f} ms per step: within (a)'s run-to-run spread."]
    finally:
        shutil.rmtree(data_dir, ignore_errors=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

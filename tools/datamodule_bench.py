"""tools/datamodule_bench.py -- how fast SegmentationDataModule.train_batches() hands out batches, on one MI355X, over a tree of
PNG files this tool writes itself (Pillow; Cityscapes 1024 x 2048 with label maps, ACDC 1080 x 1920 with reference images),
under refign_hrda_star.yaml's data section (two + two samples per batch, 1024 x 1024 crops, rare-class sampling with the
category-ratio re-draws, no load-time resize).

For prefetch 0 / 2 and num_workers 0 / 4:
  free running   batches per second when nothing stands between two next() calls (what the loader can deliver at most)
  with a step    the host time inside next() when the caller is away for --step_ms between two calls, the way a training step
                 keeps it away (time.sleep: the decoding threads have the cores meanwhile): what the loader adds to a step
The images are smooth ramps under noise: PNG's filters do worse on them than on photographs, so the files are larger and
slower to decode than the data sets' own (Cityscapes: 2 - 2.5 MB a file; these: see the output).  No threshold.

  --with_step N  Trainer.fit over the loader against Trainer.fit over two batches kept on the device: the step's own time and
                 what the loader adds to it, measured and not inferred

    python tools/datamodule_bench.py [--batches 24] [--step_ms 0] [--with_step 0] [--out profiles/datamodule_bench.txt]"""
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

_PIPE = "data_modules.transforms."
N_FILES = 8


def _image(rng, h, w):
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 100 * np.sin(x / 37.0 + c) * np.cos(y / 23.0) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def _label(rng, h, w):
    coarse = rng.integers(0, 19, (h // 64, w // 64))
    coarse[rng.random(coarse.shape) < 0.3] = 0
    lbl = np.repeat(np.repeat(coarse, 64, 0), 64, 1).astype(np.uint8)
    lbl[rng.random((h, w)) < 0.01] = 255
    return lbl


def write_tree(data_dir):
    from PIL import Image
    rng = np.random.default_rng(0)
    sizes = []

    def save(arr, *path):
        os.makedirs(os.path.dirname(os.path.join(data_dir, *path)), exist_ok=True)
        Image.fromarray(arr).save(os.path.join(data_dir, *path), compress_level=3)
        sizes.append(os.path.getsize(os.path.join(data_dir, *path)))

    for i in range(N_FILES):
        save(_image(rng, 1024, 2048), "Cityscapes", "leftImg8bit", "train", "city", f"city_{i:06d}_000019_leftImg8bit.png")
        save(_label(rng, 1024, 2048), "Cityscapes", "gtFine", "train", "city", f"city_{i:06d}_000019_gtFine_labelTrainIds.png")
        save(_image(rng, 1080, 1920), "ACDC", "rgb_anon", "fog", "train", "GOPR0475", f"GOPR0475_frame_{i:06d}_rgb_anon.png")
        save(_image(rng, 1080, 1920), "ACDC", "rgb_anon", "fog", "train_ref", "GOPR0475", f"GOPR0475_frame_{i:06d}_rgb_ref_anon.png")
    os.makedirs(os.path.join(data_dir, "ACDC", "gt"), exist_ok=True)
    return sizes


def data_cfg(num_workers):
    pipe = lambda **crop: [{"class_path": _PIPE + "ToTensor"}, {"class_path": _PIPE + "RandomCrop", "init_args": crop},  # noqa: E731
                           {"class_path": _PIPE + "RandomHorizontalFlip"}, {"class_path": _PIPE + "ConvertImageDtype"},
                           {"class_path": _PIPE + "Normalize"}]
    return {"data": {"class_path": "data_modules.CombinedDataModule", "init_args": {"batch_size": 4, "num_workers": num_workers, "load_config": {
        "train": {"Cityscapes": {"rcs_enabled": True, "rcs_min_crop_ratio": 2.0, "load_keys": ["image", "semantic"],
                                 "transforms": pipe(size=[1024, 1024], cat_max_ratio=0.75)},
                  "ACDC": {"condition": "fog", "load_keys": ["image", "image_ref"], "transforms": pipe(size=[1024, 1024])}}}}}}


def measure(data_dir, dev, prefetch, workers, batches, step_ms):
    from refign_amd.datamodule import SegmentationDataModule
    random.seed(0); torch.manual_seed(0)
    dm = SegmentationDataModule(data_cfg(workers), data_dir, dev, prefetch=prefetch)
    it = dm.train_batches()
    for _ in range(4):                                           # buffers, tables, threads
        next(it)
    torch.cuda.synchronize()
    h0, t0 = it.host_seconds, time.perf_counter()
    for _ in range(batches):
        next(it)
        if step_ms > 0:
            time.sleep(step_ms / 1e3)
    torch.cuda.synchronize()
    wall, host = time.perf_counter() - t0, it.host_seconds - h0
    dm.close()
    return wall, host


def with_step(data_dir, dev, steps):
    """ms per training step of Trainer.fit (the bench's HRDA MiT-B5 model, random weights, bf16) when the batches come (a) from two
    batches kept on the device, (b) / (c) from train_batches().  The step works on the loader's 1024 x 1024 crops."""
    import copy

    import bench
    from refign_amd import config
    from refign_amd.datamodule import SegmentationDataModule
    from refign_amd.trainer import Trainer
    random.seed(0); torch.manual_seed(0)
    over = {"backbone.init_args.pretrained": None, "alignment_backbone.init_args.pretrained": None,
            "alignment_head.init_args.pretrained": None}
    model = config.build_model(copy.deepcopy(bench.REF_CFG), over).to(dev).train()
    trainer = Trainer(model, precision="bf16")

    def timed(batches):
        start = int(model.global_step)
        trainer.fit(batches, max_steps=start + 6, save_last=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.fit(batches, max_steps=start + 6 + steps, save_last=False)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    rows = []
    dm = SegmentationDataModule(data_cfg(0), data_dir, dev, prefetch=0)
    it = dm.train_batches()
    kept = [{k: v.clone() for k, v in next(it).items()} for _ in range(2)]
    dm.close()
    rows.append(("two batches kept on the device (no loader)", timed(kept)))
    for prefetch, workers in ((2, 4), (0, 0)):
        dm = SegmentationDataModule(data_cfg(workers), data_dir, dev, prefetch=prefetch)
        rows.append((f"train_batches(), prefetch {prefetch}, num_workers {workers}", timed(dm.train_batches())))
        dm.close()
    trainer.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--with_step", type=int, default=0, metavar="STEPS", help="also time Trainer.fit over the loader for STEPS steps")
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--step_ms", type=float, default=0.0, help="time the caller spends between two next() calls in the second table")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("datamodule_bench: no GPU (a timing from anywhere else says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    data_dir = tempfile.mkdtemp(prefix="refign_dm_bench_")
    try:
        sizes = write_tree(data_dir)
        from refign_amd.datasets import write_class_stats
        write_class_stats(os.path.join(data_dir, "Cityscapes"))
        lines = [f"tools/datamodule_bench.py --batches {args.batches} --step_ms {args.step_ms:g} --with_step {args.with_step} on {torch.cuda.get_device_name(0)}",
                 f"tree: {N_FILES} Cityscapes files 1024 x 2048 with labels, {N_FILES} ACDC pairs 1080 x 1920; image files "
                 f"{np.mean([s for s in sizes if s > 10 ** 6]) / 1e6:.2f} MB on average; a batch decodes 2 images + 2 label maps + 4 images",
                 "batch: 2 + 2 samples, 1024 x 1024 crops, rare-class sampling (refign_hrda_star.yaml's data section)", "",
                 "prefetch  num_workers   free running: batches/s   host ms in next()   |   caller away "
                 f"{args.step_ms:g} ms per batch: host ms in next()"]
        for prefetch, workers in ((0, 0), (0, 4), (2, 0), (2, 4)):
            wall, host = measure(data_dir, dev, prefetch, workers, args.batches, 0.0)
            row = f"{prefetch:8d}  {workers:11d}   {args.batches / wall:24.2f}   {1e3 * host / args.batches:17.1f}   |   "
            if args.step_ms > 0:
                _, host_s = measure(data_dir, dev, prefetch, workers, args.batches, args.step_ms)
                row += f"{1e3 * host_s / args.batches:10.1f}"
            else:
                row += "       (not run)"
            lines.append(row)
        if args.with_step > 0:
            lines += ["", f"Trainer.fit, HRDA MiT-B5 (random weights, bf16), 2 + 2 crops of 1024 x 1024, {args.with_step} steps after 6: ms per step"]
            lines += [f"  {name:58s} {ms:8.1f}" for name, ms in with_step(data_dir, dev, args.with_step)]
        lines += ["", "prefetch 2 with num_workers 0 decodes on one thread; prefetch 0 decodes inside next() whatever num_workers says."]
    finally:
        shutil.rmtree(data_dir, ignore_errors=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

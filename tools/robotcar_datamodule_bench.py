"""tools/robotcar_datamodule_bench.py -- the semi-supervised RobotCar recipe from folders on one MI355X: the data section of
configs/cityscapes_robotcar/refign_daformer.yaml (b = 6: two rare-class Cityscapes samples read at 512 x 1024, two labelled
RobotCar samples and two RobotCar pairs read at 720 x 720, 512 x 512 crops, `ignore_every_second_semantic_training_batch`) over a
tree of PNG files this tool writes itself at the real sizes (Cityscapes 1024 x 2048, RobotCar 1024 x 1024 with raw label ids),
under the DAFormer MiT-B5 model of that configuration (random weights, bf16).  Records, no threshold:

  ms per step    Trainer.fit over (a) batches kept on the device -- a source batch of four and one of two, in turn --,
                 (b) train_batches() with prefetch 2 / num_workers 4, (c) train_batches() with prefetch 0
  next()         host time per batch inside next(), free running, for both loader settings
  kernel         the fused encode + NEAREST resize of a 1024 x 1024 label map to 720 x 720 (resize_nearest_u8(lut=)) and the
                 encode alone at 1024 x 1024, next to the plain gather (lut=None: the kernel as it was before the table existed),
                 which moves the same bytes; device events, median of --reps launches

    python tools/robotcar_datamodule_bench.py [--steps 12] [--batches 16] [--reps 200] [--out profiles/robotcar_datamodule_bench.txt]"""
import argparse
import copy
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


def _label(rng, h, w, codes):
    coarse = rng.choice(codes, (h // 64, w // 64))
    coarse[rng.random(coarse.shape) < 0.3] = codes[0]
    return np.repeat(np.repeat(coarse, 64, 0), 64, 1).astype(np.uint8)


def write_tree(data_dir):
    from PIL import Image
    rng = np.random.default_rng(0)
    sizes = []

    def save(arr, *path):
        os.makedirs(os.path.dirname(os.path.join(data_dir, *path)), exist_ok=True)
        Image.fromarray(arr).save(os.path.join(data_dir, *path), compress_level=3)
        sizes.append(os.path.getsize(os.path.join(data_dir, *path)))

    train_ids, raw_ids = list(range(19)), [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33, 0]
    lines = []
    for i in range(N_FILES):
        save(_image(rng, 1024, 2048), "Cityscapes", "leftImg8bit", "train", "city", f"city_{i:06d}_000019_leftImg8bit.png")
        lbl = _label(rng, 1024, 2048, train_ids)
        lbl[rng.random(lbl.shape) < 0.01] = 255
        save(lbl, "Cityscapes", "gtFine", "train", "city", f"city_{i:06d}_000019_gtFine_labelTrainIds.png")
        save(_image(rng, 1024, 1024), "RobotCar", "segmented_images", "training", "imgs", f"{1417176458000000 + i}.png")
        save(_label(rng, 1024, 1024, raw_ids), "RobotCar", "segmented_images", "training", "annos", f"{1417176458000000 + i}.png")
        save(_image(rng, 1024, 1024), "RobotCar", "images", "overcast-reference", "rear", f"{1417176458000000 + i}.png")
        save(_image(rng, 1024, 1024), "RobotCar", "images", "night", "rear", f"{1418235225000000 + i}.png")
        lines.append(f"overcast-reference/rear/{1417176458000000 + i}.png,night/rear/{1418235225000000 + i}.png\n")
    os.makedirs(os.path.join(data_dir, "RobotCar", "lists"), exist_ok=True)
    with open(os.path.join(data_dir, "RobotCar", "lists", "correspondence_pairs.csv"), "w") as f:
        f.writelines(lines)
    return sizes


def data_cfg(num_workers):
    """refign_daformer.yaml's data section of cityscapes_robotcar (the training sections; cat_max_ratio of the RobotCar section
    next to init_args, as the file has it)"""
    def pipe(front=(), jitter=(), **crop):
        return list(front) + [{"class_path": _PIPE + "ToTensor"}, {"class_path": _PIPE + "RandomCrop", "init_args": crop}] + \
            list(jitter) + [{"class_path": _PIPE + "RandomHorizontalFlip"}, {"class_path": _PIPE + "ConvertImageDtype"},
                            {"class_path": _PIPE + "Normalize"}]
    rotation = [{"class_path": _PIPE + "RandomRotation", "init_args": {"degrees": 10}}]
    jitter = [{"class_path": _PIPE + "ColorJitter", "init_args": {"brightness": 0.25, "contrast": 0.25, "saturation": 0.25, "hue": 0.1}}]
    return {"data": {"class_path": "data_modules.CombinedDataModule", "init_args": {
        "batch_size": 6, "num_workers": num_workers, "ignore_every_second_semantic_training_batch": True, "load_config": {"train": {
            "Cityscapes": {"rcs_enabled": True, "dims": [512, 1024], "load_keys": ["image", "semantic"],
                           "transforms": pipe(size=[512, 512], cat_max_ratio=0.75)},
            "RobotCar": [{"load_keys": ["image", "semantic"], "dims": [720, 720], "transforms": pipe(rotation, jitter, size=[512, 512])},
                         {"load_keys": ["image", "image_ref"], "dims": [720, 720], "transforms": pipe(size=[512, 512])}]}}}}}


def next_times(data_dir, dev, prefetch, workers, batches):
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
    torch.cuda.synchronize()
    wall, host = time.perf_counter() - t0, it.host_seconds - h0
    dm.close()
    return 1e3 * wall / batches, 1e3 * host / batches


def step_times(data_dir, dev, steps):
    import bench
    from refign_amd import config
    from refign_amd.datamodule import SegmentationDataModule
    from refign_amd.trainer import Trainer
    random.seed(0); torch.manual_seed(0)
    cfg = copy.deepcopy(bench.REF_CFG)
    cfg["model"]["init_args"]["use_hrda"] = False                # the DAFormer model of cityscapes_robotcar/refign_daformer.yaml
    cfg["model"]["init_args"].pop("hrda_scale_attention")
    over = {"backbone.init_args.pretrained": None, "alignment_backbone.init_args.pretrained": None,
            "alignment_head.init_args.pretrained": None}
    model = config.build_model(cfg, over).to(dev).train()
    trainer = Trainer(model, precision="bf16")

    def timed(batches):
        start = int(model.global_step)
        trainer.fit(batches, max_steps=start + 8, save_last=False)       # both source batch sizes warm, their graphs captured
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.fit(batches, max_steps=start + 8 + steps, save_last=False)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    rows = []
    dm = SegmentationDataModule(data_cfg(0), data_dir, dev, prefetch=0)
    it = dm.train_batches()
    kept = []
    while len({b["image_src"].shape[0] for b in kept}) < 2 or len(kept) % 2:
        b = {k: v.clone() for k, v in next(it).items()}
        if not kept or b["image_src"].shape[0] != kept[-1]["image_src"].shape[0]:
            kept.append(b)
    dm.close()
    rows.append((f"batches kept on the device, source batches of {[b['image_src'].shape[0] for b in kept]} in turn (no loader)", timed(kept)))
    for prefetch, workers in ((2, 4), (0, 0)):
        dm = SegmentationDataModule(data_cfg(workers), data_dir, dev, prefetch=prefetch)
        rows.append((f"train_batches(), prefetch {prefetch}, num_workers {workers}", timed(dm.train_batches())))
        dm.close()
    trainer.close()
    return rows


def kernel_times(dev, reps):
    from refign_amd.datasets import RobotCar
    from refign_amd.resample import device_lut, resize_nearest_u8
    lbl = torch.from_numpy(np.random.default_rng(1).integers(0, 34, (1024, 1024), dtype=np.uint8)).to(dev)
    lut = device_lut(RobotCar.label_lut(), dev)
    rows = []
    for size in ((720, 720), (1024, 1024)):
        for name, table in (("plain gather (lut=None)", None), ("encode + gather (lut=)", lut)):
            for _ in range(10):
                resize_nearest_u8(lbl, size, table)
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                resize_nearest_u8(lbl, size, table)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            rows.append((f"1024 x 1024 -> {size[0]} x {size[1]}, {name}", 1e3 * float(np.median(ms)), 1e3 * float(np.min(ms))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("robotcar_datamodule_bench: no GPU (a timing from anywhere else says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    data_dir = tempfile.mkdtemp(prefix="refign_rc_bench_")
    try:
        sizes = write_tree(data_dir)
        from refign_amd.datasets import write_class_stats
        write_class_stats(os.path.join(data_dir, "Cityscapes"))
        lines = [f"tools/robotcar_datamodule_bench.py --steps {args.steps} --batches {args.batches} --reps {args.reps} on {torch.cuda.get_device_name(0)}",
                 f"tree: {N_FILES} Cityscapes files 1024 x 2048 with labels, {N_FILES} labelled RobotCar files and {N_FILES} RobotCar pairs "
                 f"1024 x 1024; image files {np.mean([s for s in sizes if s > 10 ** 6]) / 1e6:.2f} MB on average",
                 "batch: 2 + 2 + 2 samples (b = 6), dims 512 x 1024 / 720 x 720, 512 x 512 crops, the coin halves the source batch "
                 "(cityscapes_robotcar/refign_daformer.yaml's data section)", "",
                 f"Trainer.fit, DAFormer MiT-B5 (random weights, bf16), {args.steps} steps after 8: ms per step"]
        lines += [f"  {name:90s} {ms:8.1f}" for name, ms in step_times(data_dir, dev, args.steps)]
        lines += ["", f"next(), free running, {args.batches} batches after 4: wall ms per batch, host ms inside next() per batch"]
        for prefetch, workers in ((2, 4), (0, 0)):
            wall, host = next_times(data_dir, dev, prefetch, workers, args.batches)
            lines.append(f"  prefetch {prefetch}, num_workers {workers}: {wall:8.1f} {host:8.1f}")
        lines += ["", f"label map kernels, device events around one launch, {args.reps} launches: median us, fastest us "
                  "(the event pair's own cost is in every figure)"]
        lines += [f"  {name:58s} {med:8.1f} {best:8.1f}" for name, med, best in kernel_times(dev, args.reps)]
    finally:
        shutil.rmtree(data_dir, ignore_errors=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

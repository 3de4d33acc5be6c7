"""refign_amd/run.py -- the reference's `python tools/run.py fit | validate | test | predict --config X`, from dataset folders:

    python -m refign_amd.run {fit,validate,test,predict} --config X --data_dir D [--ckpt_path P] [--save_dir S]
                             [--set dotted.key=value ...] [--graph_step]

`--set` edits the loaded YAML before anything is built; the value is parsed by yaml.safe_load (`--set trainer.precision=16`,
`--set model.init_args.backbone.init_args.pretrained=null`, `--set data.init_args.batch_size=2`).  The reference's
`--trainer.*` / `--model.*` flags of LightningCLI are not reproduced: `--set trainer.precision=16` is the equivalent.
The model comes from config.build_model with every opt-in family of config.FAMILIES switched on (the refign_deeplabv2
configurations: ResNet-101-v1c + DeepLabV2Head, refign_amd/resnet.py), the Trainer from config.trainer_kwargs / trainer_logging / trainer_gradients /
trainer_deterministic, the batches from datamodule.SegmentationDataModule -- or, when the model is the matcher
(AlignmentModel: configs/megadepth/uawarpc_*.yaml), from datamodule.MatchingDataModule; the run is seeded as Lightning's
seed_everything seeds it (`seed_everything:` of the YAML: python's random, numpy, torch).  --graph_step is
Trainer(graph_step=True): the matcher's training step replayed from one hipGraph (a ValueError for the UDA model).
  fit        Trainer.fit over train_batches() with the `val` loaders; checkpoints (`last.ckpt`) go to --save_dir, or to
             `checkpoints` under the TensorBoard logger's directory, or to ./checkpoints
  validate / test / predict   the split's loaders; predict writes under --save_dir (default: the current directory) at the data
             set's original size (the matcher has no predict: config.OutOfScopeError)
Every segmentation configuration the reference ships runs this way, and every section of each (cityscapes_robotcar: the
semi-supervised three-loader recipe; `test` of the Dark Zurich configurations: DarkZurich, NighttimeDriving, BDD100kNight);
--datasets picks sections.  A data set without a reader makes the split that names it fail with config.OutOfScopeError."""
import argparse
import os
import random
import sys

import numpy as np
import torch
import yaml

from . import config


def apply_set(cfg, edits):
    """`dotted.key=value` edits of a loaded YAML, in place; a number in the path indexes a list; missing dicts are made"""
    for edit in edits or []:
        dotted, eq, text = edit.partition("=")
        if not eq or not dotted:
            raise ValueError(f"--set takes dotted.key=value, got {edit!r}")
        keys, node = dotted.split("."), cfg
        for depth, k in enumerate(keys):
            k = int(k) if isinstance(node, list) else k
            if depth == len(keys) - 1:
                node[k] = yaml.safe_load(text)
            else:
                if isinstance(node, dict) and not isinstance(node.get(k), (dict, list)):
                    node[k] = {}
                node = node[k]
    return cfg


def seed_everything(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m refign_amd.run", description="fit / validate / test / predict from dataset folders")
    p.add_argument("command", choices=("fit", "validate", "test", "predict"))
    p.add_argument("--config", required=True, help="a configuration of the reference (YAML)")
    p.add_argument("--data_dir", default=os.environ.get("DATA_DIR"),
                   help="holds Cityscapes/, ACDC/, DarkZurich/, RobotCar/, NighttimeDriving/, BDD100kNight/; for the matcher MegaDepth/, "
                        "RobotCarMatching/ ($DATA_DIR)")
    p.add_argument("--ckpt_path", default=None, help="a checkpoint of Trainer.save_checkpoint (or Lightning's layout) to start from")
    p.add_argument("--save_dir", default=None)
    p.add_argument("--set", dest="edits", action="append", default=[], metavar="dotted.key=value")
    p.add_argument("--datasets", nargs="+", default=None, help="the evaluation sections to run (default: all)")
    p.add_argument("--graph_step", action="store_true", help="Trainer(graph_step=True): the matcher's step from one hipGraph")
    args = p.parse_args(argv)
    if not args.data_dir:
        p.error("--data_dir (or $DATA_DIR) is required")
    return args


def main(argv=None, handles=None):
    """-> what the loop returns: fit's [(global_step, metrics)], validate's / test's metrics, predict's number of files.
    handles (a dict): receives `trainer` and `datamodule`, which are then left open for the caller to close."""
    from .alignment_model import AlignmentModel
    from .datamodule import MatchingDataModule, SegmentationDataModule
    from .trainer import Trainer
    args = parse_args(sys.argv[1:] if argv is None else argv)
    cfg = apply_set(config.load_config(args.config), args.edits)
    seed = cfg.get("seed_everything")
    if seed is not None and seed is not False:
        seed_everything(int(seed))
    if not torch.cuda.is_available():
        raise RuntimeError("refign_amd.run: a HIP device is required (the product path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    model = config.build_model(cfg, families=tuple(config.FAMILIES)).to(device).train()
    kw = config.trainer_kwargs(cfg)
    logging = config.trainer_logging(cfg)
    trainer = Trainer(model, sync_batchnorm=kw["sync_batchnorm"], precision=kw["precision"], ckpt_path=args.ckpt_path,
                      deterministic=config.trainer_deterministic(cfg), graph_step=args.graph_step, **logging,
                      **config.trainer_gradients(cfg))
    dm = (MatchingDataModule if isinstance(model, AlignmentModel) else SegmentationDataModule)(cfg, args.data_dir, device)
    try:
        if args.command == "fit":
            ckpt_dir = args.save_dir or os.path.join(getattr(logging["logger"], "log_dir", None) or ".", "checkpoints")
            val = dm.loaders("val", args.datasets) if kw["val_every_n_steps"] else None
            return trainer.fit(dm.train_batches(), val_loaders=val, max_steps=kw["max_steps"],
                               val_every_n_steps=kw["val_every_n_steps"], ckpt_dir=ckpt_dir, save_last=kw["save_last"])
        if args.command == "validate":
            return trainer.validate(dm.loaders("val", args.datasets))
        if args.command == "test":
            return trainer.test(dm.loaders("test", args.datasets))
        loaders = dm.loaders("predict", args.datasets)
        sizes = {dm.orig_dims[name] for name in loaders}
        if len(sizes) > 1:
            raise config.OutOfScopeError(f"refign_amd.run predict: data sets of different original sizes ({sorted(sizes)}): run them "
                                         f"one at a time with --datasets")
        # (fused_resize: the interpolation to the original size happens inside the evaluation tail's kernel; RFN_EVAL_FUSED=0
        # keeps model.predict_step)
        return trainer.predict(loaders, args.save_dir or ".", orig_size=sizes.pop() if sizes else None, fused_resize=True)
    finally:
        if handles is not None:
            handles.update(trainer=trainer, datamodule=dm)
        else:
            dm.close()
            trainer.close()


if __name__ == "__main__":
    print(main())

"""YAML `class_path` / `init_args` instantiation so that the reference's configs/*.yaml run unmodified.

The reference drives everything through LightningCLI + jsonargparse (tools/run.py:4-9, helpers/cli.py:10-21): every
object is a `{class_path: pkg.Class, init_args: {...}}` dict, nested recursively; `optimizer` and `lr_scheduler` are
linked into `model.init_args.{optimizer_init, lr_scheduler_init}` as dicts and instantiated later by
`instantiate_class` (segmentation_model.py:385-387).  Neither package is installed here, so this file provides the same
two operations.  Class paths of the reference's own packages are routed to their MI355X implementations.
"""
import importlib

import yaml

# reference class path -> implementation in this repo
ALIASES = {
    "models.DomainAdaptationSegmentationModel": "refign_amd.uda.DomainAdaptationSegmentationModel",
    "models.AlignmentModel": "refign_amd.alignment_model.AlignmentModel",
    "models.backbones.MixVisionTransformer": "refign_amd.seg.MixVisionTransformer",
    "models.backbones.VGG": "refign_amd.align.VGG",
    "models.heads.DAFormerHead": "refign_amd.seg.DAFormerHead",
    "models.heads.SegFormerHead": "refign_amd.seg.SegFormerHead",
    "models.heads.UAWarpCHead": "refign_amd.align.UAWarpCHead",
    "models.losses.PixelWeightedCrossEntropyLoss": "refign_amd.seg.PixelWeightedCrossEntropyLoss",
    "models.losses.HuberLoss": "refign_amd.losses.HuberLoss",
    "models.losses.MultiScaleFlowLoss": "refign_amd.losses.MultiScaleFlowLoss",
    "models.losses.WBipathLoss": "refign_amd.losses.WBipathLoss",
    "helpers.metrics.IoU": "refign_amd.metrics.IoU",
    "helpers.metrics.SparseEPE": "refign_amd.metrics.SparseEPE",
    "helpers.lr_scheduler.LinearWarmupPolynomialLR": "refign_amd.trainer.LinearWarmupPolynomialLR",
    "helpers.callbacks.ValEveryNSteps": "refign_amd.trainer.ValEveryNSteps",
}
# Opt-in model families: reference class path -> implementation, per family.  build_model(cfg, families=("deeplabv2",)) adds a
# family's map for that one call; ALIASES itself never changes, so a build without the keyword keeps refusing these classes.
FAMILIES = {
    "deeplabv2": {"models.backbones.ResNet": "refign_amd.resnet.ResNet",
                  "models.heads.DeepLabV2Head": "refign_amd.resnet.DeepLabV2Head"},
}
# subsystems that are out of scope here (host I/O, logging, evaluation): accepted in a config, not instantiated
IGNORED_PREFIXES = ("pytorch_lightning.", "data_modules.", "helpers.metrics.")
# class paths accepted in a config but kept as specs (none at present: the matcher-training losses of row N1 are built)
DEFERRED = ()


# reference packages whose classes are routed through ALIASES; anything of theirs that has no alias is a component
# outside the align-and-refine hot path (ResNet / DeepLabV2, data modules, metrics, ...)
_REFERENCE_PACKAGES = ("models.", "helpers.", "data_modules.")


class OutOfScopeError(NotImplementedError):
    pass


def family_aliases(families):
    """The alias map of the named opt-in families (a name or a sequence of names of FAMILIES), merged; {} for none."""
    extra = {}
    for name in ((families,) if isinstance(families, str) else tuple(families or ())):
        if name not in FAMILIES:
            raise ValueError(f"unknown model family {name!r} (one of {sorted(FAMILIES)})")
        extra.update(FAMILIES[name])
    return extra


def resolve(class_path, extra=None):
    """`extra`: an alias map looked up after ALIASES (family_aliases(...)); None: ALIASES alone."""
    path = ALIASES.get(class_path)
    if path is None and extra:
        path = extra.get(class_path)
    if path is None:
        if class_path.startswith(_REFERENCE_PACKAGES):
            optin = [name for name, m in sorted(FAMILIES.items()) if class_path in m]
            hint = (f"; it belongs to the opt-in family {optin[0]!r}: build_model(cfg, families=({optin[0]!r},)), which "
                    f"`python -m refign_amd.run` passes") if optin else ""
            raise OutOfScopeError(f"{class_path} is out of scope of refign_amd (the align-and-refine hot path: "
                                  f"{', '.join(sorted(ALIASES))}){hint}")
        path = class_path
    mod, _, name = path.rpartition(".")
    return getattr(importlib.import_module(mod), name)


def is_spec(x):
    return isinstance(x, dict) and "class_path" in x


def build(spec, extra=None):
    """Recursively instantiate a {class_path, init_args} tree (nested specs inside init_args are built first).
    `extra`: the alias map of the opt-in families, handed down to resolve."""
    if is_spec(spec):
        if spec["class_path"].startswith(IGNORED_PREFIXES) or spec["class_path"] in DEFERRED:
            return spec
        kwargs = {k: build(v, extra) for k, v in spec.get("init_args", {}).items()}
        return resolve(spec["class_path"], extra)(**kwargs)
    if isinstance(spec, list):
        return [build(v, extra) for v in spec]
    return spec


def instantiate_class(args, init):
    """pytorch_lightning.utilities.cli.instantiate_class: `init` = {class_path, init_args}, `args` = positional."""
    args = args if isinstance(args, tuple) else (args,)
    return resolve(init["class_path"])(*args, **init.get("init_args", {}))


def load_config(path):
    with open(path) as f:
        return yaml.safe_load(f)


def build_model(cfg, overrides=None, families=()):
    """Build `cfg['model']` with the optimizer / lr_scheduler sections linked in as dicts (helpers/cli.py:17-21).
    `overrides` (dict) is merged into model.init_args first, e.g. {'backbone.init_args.pretrained': None}.
    `families`: names of FAMILIES whose classes this call may build (("deeplabv2",): ResNet-v1c + DeepLabV2Head); without it
    those class paths raise OutOfScopeError as before.  Nothing is remembered between calls."""
    extra = family_aliases(families)
    model = dict(cfg["model"])
    init = dict(model.get("init_args", {}))
    init["optimizer_init"] = cfg.get("optimizer", init.get("optimizer_init"))
    init["lr_scheduler_init"] = cfg.get("lr_scheduler", init.get("lr_scheduler_init"))
    for dotted, val in (overrides or {}).items():
        node = init
        keys = dotted.split(".")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = val
    # metrics are evaluation-only (helpers.metrics, torchmetrics): kept as config, not built
    metrics = init.pop("metrics", {})
    kwargs = {k: (v if k in ("optimizer_init", "lr_scheduler_init") else build(v, extra)) for k, v in init.items()}
    return resolve(model["class_path"], extra)(metrics=metrics, **kwargs)


def trainer_kwargs(cfg):
    """What the loops of refign_amd.trainer.Trainer take from a loaded YAML's `trainer:` section (LightningCLI's Trainer
    arguments): `max_steps`, `sync_batchnorm`, `precision` as they stand, `val_every_n_steps` from the ValEveryNSteps
    callback's `every_n_steps` and `save_last` from ModelCheckpoint, found in the `callbacks` list by class_path.  Missing
    entries: None (False for the two flags).  Loggers and LearningRateMonitor are read by trainer_logging; every other
    Lightning argument stays ignored.
    -> Trainer(model, sync_batchnorm=, precision=) and Trainer.fit(max_steps=, val_every_n_steps=, save_last=)."""
    tr = (cfg or {}).get("trainer") or {}
    out = {"max_steps": tr.get("max_steps"), "val_every_n_steps": None, "save_last": False,
           "sync_batchnorm": bool(tr.get("sync_batchnorm", False)), "precision": tr.get("precision")}
    callbacks = tr.get("callbacks") or []
    for cb in ([callbacks] if is_spec(callbacks) else callbacks):
        if not is_spec(cb):
            continue
        name, args = cb["class_path"].rsplit(".", 1)[-1], cb.get("init_args") or {}
        if name == "ValEveryNSteps":
            out["val_every_n_steps"] = args.get("every_n_steps")
        elif name == "ModelCheckpoint":
            out["save_last"] = bool(args.get("save_last", False))
    return out


def trainer_deterministic(cfg):
    """`trainer.deterministic` of a loaded YAML (Lightning's `--trainer.deterministic true`; `warn` counts as on); False when
    absent.  Kept out of trainer_kwargs, whose five keys are what Trainer / Trainer.fit took before the mode existed:
    Trainer(model, ..., deterministic=trainer_deterministic(cfg))."""
    v = ((cfg or {}).get("trainer") or {}).get("deterministic", False)
    if isinstance(v, str):
        return v.strip().lower() in ("true", "1", "yes", "warn")
    return bool(v)


def trainer_gradients(cfg):
    """What shapes the gradient between the backward pass and the optimizer, from a loaded YAML's `trainer:` section:
    `gradient_clip_val` (None when absent), `gradient_clip_algorithm` ("norm") and `accumulate_grad_batches` (1), checked as
    Trainer checks them (ValueError for a negative or non-numeric threshold, an unknown algorithm, and an accumulation that
    is no int >= 1 -- Lightning's per-epoch dict among them).  Kept out of trainer_kwargs like trainer_deterministic.
    -> the three keywords of Trainer(model, ...)."""
    from .trainer import parse_accumulate, parse_gradient_clip
    tr = (cfg or {}).get("trainer") or {}
    val, alg = tr.get("gradient_clip_val"), tr.get("gradient_clip_algorithm")
    acc = tr.get("accumulate_grad_batches")
    alg, acc = "norm" if alg is None else alg, 1 if acc is None else acc
    parse_gradient_clip(val, alg)
    return {"gradient_clip_val": val, "gradient_clip_algorithm": alg, "accumulate_grad_batches": parse_accumulate(acc)}


def trainer_logging(cfg):
    """The record of the run as a loaded YAML asks for it: `trainer.logger` (one spec or a list; the first
    pytorch_lightning.loggers.TensorBoardLogger with its `save_dir` / `name` / `version` becomes a
    refign_amd.steplog.TensorBoardLogger, anything else is passed over), `trainer.log_every_n_steps` (Lightning's default 50
    when absent) and whether LearningRateMonitor is among the callbacks.  Kept out of trainer_kwargs like trainer_deterministic.
    -> {"logger": TensorBoardLogger or None, "log_every_n_steps": n, "log_lr": bool}, the keywords of Trainer(model, ...).
    The logger touches the disk on its first write only."""
    tr = (cfg or {}).get("trainer") or {}
    out = {"logger": None, "log_every_n_steps": int(tr.get("log_every_n_steps") or 50), "log_lr": False}
    loggers = tr.get("logger")
    for spec in ([loggers] if is_spec(loggers) else loggers if isinstance(loggers, list) else []):
        if is_spec(spec) and spec["class_path"].rsplit(".", 1)[-1] == "TensorBoardLogger" and out["logger"] is None:
            from .steplog import TensorBoardLogger
            args = spec.get("init_args") or {}
            out["logger"] = TensorBoardLogger(args.get("save_dir", "lightning_logs"), name=args.get("name", "default"),
                                              version=args.get("version"))
    callbacks = tr.get("callbacks") or []
    for cb in ([callbacks] if is_spec(callbacks) else callbacks):
        if is_spec(cb) and cb["class_path"].rsplit(".", 1)[-1] == "LearningRateMonitor":
            out["log_lr"] = True
    return out


# transforms of a data set's pipeline that the device data step covers, in the order the reference's configs apply them
_INGEST_ORDER = ("Resize", "ToTensor", "RandomCrop", "RandomHorizontalFlip", "ConvertImageDtype", "Normalize", "PadBottomRight")
_INGEST_ARGS = {"Resize": {"size", "img_only", "only_if_larger", "img_interpolation"}, "ToTensor": set(),
                "RandomCrop": {"size", "cat_max_ratio"}, "RandomHorizontalFlip": {"p"}, "ConvertImageDtype": set(),
                "Normalize": {"mean", "std"}, "PadBottomRight": {"size", "same_shape_keys"}}
_INGEST_FILTERS = ("bilinear", "lanczos")                 # Pillow filters the device resize restates (refign_amd/resample.py)


def ingest_plan(cfg, split, dataset):
    """What `data.init_args.load_config[split][dataset]` of a loaded YAML asks of the path from a decoded file to the batch
    tensors, as the keywords of the device data step (refign_amd/resample.py, refign_amd/datastep.py):
      dims           load-time size (h, w) of the data set reader as the section gives it, or None (a reader's own default --
                     RobotCarMatching's (1024, 1024) -- is the reader's business: readers are outside this package)
      resize         transforms.Resize's `size` (int or (h, w)), or None; img_only: its flag (the label keeps its size);
                     only_if_larger: its flag; interpolation: its `img_interpolation` ("bilinear" when absent)
      dims_interpolation  the filter of the reader's load-time resize: "lanczos" for MegaDepth, RobotCarMatching's
                     `resize_filter` ("lanczos" when absent), "bilinear" for every other data set
      pad            transforms.PadBottomRight after Normalize: None, "same" (`same_shape_keys`: both images at the larger
                     height and width) or its `size` (h, w)
      crop_size      RandomCrop's size (h, w), or None; cat_max_ratio: its ratio (1.0 when absent)
      flip           RandomHorizontalFlip's probability (0.0 when absent)
      mean / std     Normalize's statistics (ImageNet's by default)
      load_keys      the reader's keys, as given
    train: RareClassSourceSampler / PairSampler(..., dims=, crop_size=, cat_max_ratio=); val / test / predict:
    resample.EvalIngest(dims=, resize=, img_only=, only_if_larger=, interpolation=, dims_interpolation=, pad=).  The pipeline
    must be made of ToTensor / Resize / RandomCrop / RandomHorizontalFlip / ConvertImageDtype / Normalize / PadBottomRight in
    the reference's order with their defaults for everything the plan does not carry; anything else (ColorJitter, the MegaDepth
    flow synthesis, a filter other than bilinear / lanczos, ...) raises OutOfScopeError naming the transform or the value.
    `build` and IGNORED_PREFIXES are untouched: data_modules.* specs still come back as specs from there."""
    from .datastep import IMNET_MEAN, IMNET_STD
    try:
        sec = cfg["data"]["init_args"]["load_config"][split][dataset]
    except (KeyError, TypeError) as e:
        raise KeyError(f"ingest_plan: no data.init_args.load_config.{split}.{dataset} in this config") from e
    pair = lambda v: v if isinstance(v, int) else tuple(int(a) for a in v)  # noqa: E731
    plan = {"dims": pair(sec["dims"]) if sec.get("dims") is not None else None, "resize": None, "img_only": False,
            "only_if_larger": False, "crop_size": None, "cat_max_ratio": 1.0, "flip": 0.0, "mean": tuple(IMNET_MEAN),
            "std": tuple(IMNET_STD), "load_keys": list(sec.get("load_keys") or []), "interpolation": "bilinear",
            "dims_interpolation": {"MegaDepth": "lanczos", "RobotCarMatching": sec.get("resize_filter", "lanczos")}.get(
                dataset, "bilinear"), "pad": None}
    if plan["dims_interpolation"] not in _INGEST_FILTERS:
        raise OutOfScopeError(f"ingest_plan: resize_filter {plan['dims_interpolation']!r} ({split}.{dataset}) is outside the "
                              f"device resize ({' / '.join(_INGEST_FILTERS)})")
    stage = -1
    for spec in sec.get("transforms") or []:
        path = spec["class_path"] if is_spec(spec) else str(spec)
        name, args = path.rsplit(".", 1)[-1], (spec.get("init_args") or {}) if is_spec(spec) else {}
        if not path.startswith("data_modules.transforms.") or name not in _INGEST_ORDER:
            raise OutOfScopeError(f"ingest_plan: {path} ({split}.{dataset}) is outside the device data step "
                                  f"({' / '.join(_INGEST_ORDER)})")
        if _INGEST_ORDER.index(name) <= stage and name != "Resize":
            raise OutOfScopeError(f"ingest_plan: {path} ({split}.{dataset}) comes out of the order {' -> '.join(_INGEST_ORDER)}")
        extra = set(args) - _INGEST_ARGS[name]
        if extra or (name == "Resize" and plan["resize"] is not None):
            raise OutOfScopeError(f"ingest_plan: {path} ({split}.{dataset}) with {sorted(extra) or 'a second Resize'} is outside the "
                                  f"device data step")
        stage = _INGEST_ORDER.index(name)
        if name == "Resize":
            plan["resize"], plan["img_only"] = pair(args["size"]), bool(args.get("img_only", False))
            plan["only_if_larger"] = bool(args.get("only_if_larger", False))
            plan["interpolation"] = args.get("img_interpolation", "bilinear")
            if plan["interpolation"] not in _INGEST_FILTERS:
                raise OutOfScopeError(f"ingest_plan: {path} ({split}.{dataset}) with img_interpolation "
                                      f"{plan['interpolation']!r} is outside the device resize ({' / '.join(_INGEST_FILTERS)})")
        elif name == "RandomCrop":
            plan["crop_size"], plan["cat_max_ratio"] = pair(args["size"]), float(args.get("cat_max_ratio", 1.0))
        elif name == "RandomHorizontalFlip":
            plan["flip"] = float(args.get("p", 0.5))
        elif name == "Normalize":
            plan["mean"], plan["std"] = tuple(args.get("mean", IMNET_MEAN)), tuple(args.get("std", IMNET_STD))
        elif name == "PadBottomRight":
            keys, size = args.get("same_shape_keys"), args.get("size")
            if (keys is None) == (size is None) or (keys is not None and len(keys) != 2):
                raise OutOfScopeError(f"ingest_plan: {path} ({split}.{dataset}) takes `same_shape_keys` (two keys) or `size`")
            plan["pad"] = "same" if keys is not None else pair(size)
    return plan


# CompositeFlow's keywords that draw_composite carries (refign_amd/flowsynth.py), with the reference's defaults
_COMPOSITE_DEFAULTS = {"include_transforms": ["hom", "affine"], "random_alpha": 0.065, "random_s": 0.6, "random_tx": 0.3,
                       "random_ty": 0.1, "random_t_tps": 0, "random_t_hom": 0.3, "random_t_tps_for_afftps": 0,
                       "parameterize_with_gaussian": False, "add_elastic": False}


def warp_supervision_plan(cfg, split="train", dataset="MegaDepth"):
    """The geometric half of `data.init_args.load_config[split][dataset]`'s pipeline -- transforms.CompositeFlow and the
    transforms.CenterCrop after it -- as the keywords of refign_amd.flowsynth.WarpSupervision:
      composite                 draw_composite's keywords: CompositeFlow's init_args over the reference's defaults
      crop                      CenterCrop's size (h, w), or None when the section has none
      min_fraction_valid_corr   CompositeFlow's (0.1 when absent)
    Every other transform of the section (the photometric chain on image_prime, the conversions) is passed over: this reads two
    entries and builds nothing.  OutOfScopeError names what cannot be carried: a section without CompositeFlow or with two, a
    CenterCrop in front of it, apply_keys other than ['image_prime'], parameterize_with_gaussian, a transform name that
    draw_composite does not know, an unknown keyword.  ingest_plan keeps refusing such a section: it describes the path from a
    file to the batch tensors, this the step after it."""
    try:
        sec = cfg["data"]["init_args"]["load_config"][split][dataset]
    except (KeyError, TypeError) as e:
        raise KeyError(f"warp_supervision_plan: no data.init_args.load_config.{split}.{dataset} in this config") from e
    from .flowsynth import TRANSFORMS
    where = f"({split}.{dataset})"
    composite = crop = None
    min_fraction = 0.1
    for spec in sec.get("transforms") or []:
        path = spec["class_path"] if is_spec(spec) else str(spec)
        name, args = path.rsplit(".", 1)[-1], (spec.get("init_args") or {}) if is_spec(spec) else {}
        if not path.startswith("data_modules.transforms."):
            continue
        if name == "CompositeFlow":
            if composite is not None:
                raise OutOfScopeError(f"warp_supervision_plan: a second CompositeFlow {where}")
            if list(args.get("apply_keys") or []) != ["image_prime"]:
                raise OutOfScopeError(f"warp_supervision_plan: CompositeFlow with apply_keys {args.get('apply_keys', 'all')!r} {where}: "
                                      f"['image_prime'] is what the device path warps")
            extra = set(args) - set(_COMPOSITE_DEFAULTS) - {"apply_keys", "min_fraction_valid_corr"}
            if extra:
                raise OutOfScopeError(f"warp_supervision_plan: CompositeFlow with {sorted(extra)} {where}")
            composite = {k: args.get(k, v) for k, v in _COMPOSITE_DEFAULTS.items()}
            composite["include_transforms"] = list(composite["include_transforms"])
            if composite["parameterize_with_gaussian"]:
                raise OutOfScopeError(f"warp_supervision_plan: CompositeFlow with parameterize_with_gaussian {where}: the device "
                                      f"path carries the uniform draws only")
            unknown = [t for t in composite["include_transforms"] if t not in TRANSFORMS]
            if unknown:
                raise OutOfScopeError(f"warp_supervision_plan: CompositeFlow with transforms {unknown} {where} "
                                      f"({' / '.join(TRANSFORMS)})")
            min_fraction = float(args.get("min_fraction_valid_corr", 0.1))
        elif name == "CenterCrop":
            if composite is None or crop is not None:
                raise OutOfScopeError(f"warp_supervision_plan: CenterCrop {where} in front of CompositeFlow, or a second one")
            extra = set(args) - {"size", "apply_keys"}
            if extra or args.get("apply_keys", "all") != "all":
                raise OutOfScopeError(f"warp_supervision_plan: CenterCrop with {sorted(extra) or 'apply_keys'} {where}")
            size = args["size"]
            crop = (int(size), int(size)) if isinstance(size, int) else tuple(int(a) for a in size)
    if composite is None:
        raise OutOfScopeError(f"warp_supervision_plan: no data_modules.transforms.CompositeFlow {where}")
    return {"composite": composite, "crop": crop, "min_fraction_valid_corr": min_fraction}


# the photometric chain's transforms in the order the reference's configs apply them (refign_amd/photometric.py)
_PHOTOMETRIC_ORDER = ("ColorJitter", "ChannelShuffle", "RandomGaussianBlur")
_PHOTOMETRIC_ARGS = {"ColorJitter": {"apply_keys", "brightness", "contrast", "saturation", "hue"}, "ChannelShuffle": {"apply_keys"},
                     "RandomGaussianBlur": {"apply_keys", "p", "kernel_size", "sigma"}}


def photometric_plan(cfg, split="train", dataset="MegaDepth"):
    """The photometric half of `data.init_args.load_config[split][dataset]`'s pipeline -- transforms.ColorJitter,
    ChannelShuffle and RandomGaussianBlur on the uint8 image_prime, and the Normalize that follows the conversion -- as the
    plan of refign_amd.photometric.draw / flowsynth.WarpSupervision(plan, photometric=):
      brightness / contrast / saturation   the range (lo, hi) the factor is drawn from, [max(0, 1 - v), 1 + v] for a number v or
                                the pair as given; None where ColorJitter has no such step (0, or a range that is 1 only)
      shuffle                   whether the section has a ChannelShuffle
      blur                      None, or {"p", "kernel_size", "sigma": (lo, hi)} of RandomGaussianBlur (p 0.2, sigma (0.1, 2.0)
                                when absent, as the classes default them)
      mean / std                Normalize's statistics (ImageNet's by default)
    Every other transform of the section is passed over.  OutOfScopeError names what cannot be carried: a section without
    ColorJitter or with one of the three twice, `hue` other than 0 (the hue step's HSV round trip is left out), apply_keys other
    than ['image_prime'], an even kernel size or one above 7, the three in any order other than ColorJitter -> ChannelShuffle ->
    RandomGaussianBlur, any of them after ConvertImageDtype (the kernel works on the uint8 image), an unknown keyword.
    ingest_plan keeps refusing such a section."""
    from .datastep import IMNET_MEAN, IMNET_STD
    from .photometric import MAX_KERNEL
    try:
        sec = cfg["data"]["init_args"]["load_config"][split][dataset]
    except (KeyError, TypeError) as e:
        raise KeyError(f"photometric_plan: no data.init_args.load_config.{split}.{dataset} in this config") from e
    where = f"({split}.{dataset})"
    if not isinstance(sec, dict):
        raise OutOfScopeError(f"photometric_plan: {where} is a list of sections: pass a config that holds the one meant")
    plan = {"brightness": None, "contrast": None, "saturation": None, "shuffle": False, "blur": None,
            "mean": tuple(IMNET_MEAN), "std": tuple(IMNET_STD)}

    def jitter_range(name, value):
        """ColorJitter._check_input for the three steps centred on 1"""
        if isinstance(value, (int, float)):
            if value < 0:
                raise OutOfScopeError(f"photometric_plan: ColorJitter with {name} {value!r} {where}: a number must not be negative")
            lo, hi = max(1.0 - float(value), 0.0), 1.0 + float(value)
        elif isinstance(value, (list, tuple)) and len(value) == 2 and 0 <= value[0] <= value[1]:
            lo, hi = float(value[0]), float(value[1])
        else:
            raise OutOfScopeError(f"photometric_plan: ColorJitter with {name} {value!r} {where}: a number or a pair 0 <= lo <= hi")
        return None if lo == hi == 1.0 else (lo, hi)

    stage, seen, converted = -1, set(), False
    for spec in sec.get("transforms") or []:
        path = spec["class_path"] if is_spec(spec) else str(spec)
        name, args = path.rsplit(".", 1)[-1], (spec.get("init_args") or {}) if is_spec(spec) else {}
        if not path.startswith("data_modules.transforms."):
            continue
        if name == "ConvertImageDtype":
            converted = True
        elif name == "Normalize":
            plan["mean"], plan["std"] = tuple(args.get("mean", IMNET_MEAN)), tuple(args.get("std", IMNET_STD))
        if name not in _PHOTOMETRIC_ORDER:
            continue
        if converted:
            raise OutOfScopeError(f"photometric_plan: {name} after ConvertImageDtype {where}: the device chain works on the uint8 image")
        if name in seen:
            raise OutOfScopeError(f"photometric_plan: a second {name} {where}")
        if _PHOTOMETRIC_ORDER.index(name) < stage:
            raise OutOfScopeError(f"photometric_plan: {name} {where} comes out of the order {' -> '.join(_PHOTOMETRIC_ORDER)}")
        stage = _PHOTOMETRIC_ORDER.index(name)
        seen.add(name)
        if name == "ColorJitter":
            hue = args.get("hue", 0)
            if isinstance(hue, (list, tuple)) and len(hue) == 2 and hue[0] == hue[1] == 0:
                hue = 0
            if isinstance(hue, (list, tuple)) or hue != 0:
                raise OutOfScopeError(f"photometric_plan: ColorJitter with hue {hue!r} {where}: the hue step is outside the device "
                                      f"chain (brightness, contrast, saturation)")
        keys = args.get("apply_keys", "all")
        if isinstance(keys, str) or list(keys or []) != ["image_prime"]:
            raise OutOfScopeError(f"photometric_plan: {name} with apply_keys {keys!r} {where}: "
                                  f"['image_prime'] is what the device chain takes")
        extra = set(args) - _PHOTOMETRIC_ARGS[name]
        if extra:
            raise OutOfScopeError(f"photometric_plan: {name} with {sorted(extra)} {where}")
        if name == "ColorJitter":
            for k in ("brightness", "contrast", "saturation"):
                plan[k] = jitter_range(k, args.get(k, 0))
        elif name == "ChannelShuffle":
            plan["shuffle"] = True
        else:
            ksize = args.get("kernel_size")
            if isinstance(ksize, (list, tuple)) and len(ksize) == 2 and ksize[0] == ksize[1]:
                ksize = ksize[0]
            if not isinstance(ksize, int) or ksize < 1 or ksize % 2 == 0 or ksize > MAX_KERNEL:
                raise OutOfScopeError(f"photometric_plan: RandomGaussianBlur with kernel_size {args.get('kernel_size')!r} {where}: "
                                      f"one odd size of at most {MAX_KERNEL}")
            sigma = args.get("sigma", (0.1, 2.0))
            sigma = (float(sigma), float(sigma)) if isinstance(sigma, (int, float)) else tuple(float(v) for v in sigma)
            if len(sigma) != 2 or not 0.0 < sigma[0] <= sigma[1]:
                raise OutOfScopeError(f"photometric_plan: RandomGaussianBlur with sigma {args.get('sigma')!r} {where}: 0 < lo <= hi")
            plan["blur"] = {"p": float(args.get("p", 0.2)), "kernel_size": ksize, "sigma": sigma}
    if "ColorJitter" not in seen:
        raise OutOfScopeError(f"photometric_plan: no data_modules.transforms.ColorJitter {where}: the chain's draws begin with its "
                              f"step order")
    return plan


# the labelled RobotCar section's chain (configs/cityscapes_robotcar/refign_*.yaml), in its order
_SECTION_ORDER = ("RandomRotation", "ToTensor", "RandomCrop", "ColorJitter", "RandomHorizontalFlip", "ConvertImageDtype", "Normalize")
_SECTION_ARGS = {"RandomRotation": {"apply_keys", "degrees", "interpolation", "resample", "expand", "center", "fill"},
                 "ToTensor": set(), "RandomCrop": {"size", "cat_max_ratio"},
                 "ColorJitter": {"apply_keys", "brightness", "contrast", "saturation", "hue"}, "RandomHorizontalFlip": {"p"},
                 "ConvertImageDtype": set(), "Normalize": {"mean", "std"}}


def train_section_plan(cfg, dataset, section=None):
    """One training section `data.init_args.load_config.train[dataset]` -- `section` indexes a list of sections, as RobotCar has
    (labelled, then the adaptation pairs) -- whose pipeline is a sub-sequence of
        RandomRotation -> ToTensor -> RandomCrop -> ColorJitter -> RandomHorizontalFlip -> ConvertImageDtype -> Normalize
    as the plan of datastep.RotatedLabelledSampler: ingest_plan's keys (dims, crop_size, cat_max_ratio, flip, mean, std,
    load_keys, ...; ingest_plan itself reads a section without the two new transforms) plus
      rotation   {"degrees": (lo, hi)} of RandomRotation (a number d: (-d, d)), or None
      jitter     photometric.draw's plan of ColorJitter: brightness / contrast / saturation as photometric_plan gives them, "hue":
                 (lo, hi) -- (-v, v) for a number v in [0, 0.5], or the pair within [-0.5, 0.5] -- or None, "shuffle": False,
                 "blur": None; or None without a ColorJitter
    A keyword is read from `init_args` alone, as the reference's instantiate_class reads it: the RobotCar files indent RandomCrop's
    `cat_max_ratio: 0.75` NEXT to init_args, where it is dropped -- the plan then says 1.0, which is what the reference runs.
    OutOfScopeError names the cause: RandomRotation with expand, center, fill or an interpolation other than the defaults
    (NEAREST, no expand, the image centre, fill 0) or with apply_keys other than all; ColorJitter with apply_keys other than all;
    the transforms in another order or one of them twice; any other transform or keyword."""
    from .datastep import IMNET_MEAN, IMNET_STD
    try:
        sec = cfg["data"]["init_args"]["load_config"]["train"][dataset]
    except (KeyError, TypeError) as e:
        raise KeyError(f"train_section_plan: no data.init_args.load_config.train.{dataset} in this config") from e
    where = f"(train.{dataset})" if section is None else f"(train.{dataset}[{section}])"
    if isinstance(sec, list):
        if section is None:
            raise OutOfScopeError(f"train_section_plan: {where} is a list of {len(sec)} sections: say which with section=")
        if not 0 <= int(section) < len(sec):
            raise KeyError(f"train_section_plan: no section {section} in train.{dataset} ({len(sec)} sections)")
        sec = sec[int(section)]
    elif section not in (None, 0):
        raise KeyError(f"train_section_plan: train.{dataset} is one section, not a list")
    pair = lambda v: v if isinstance(v, int) else tuple(int(a) for a in v)  # noqa: E731
    plan = {"dims": pair(sec["dims"]) if sec.get("dims") is not None else None, "resize": None, "img_only": False,
            "only_if_larger": False, "crop_size": None, "cat_max_ratio": 1.0, "flip": 0.0, "mean": tuple(IMNET_MEAN),
            "std": tuple(IMNET_STD), "load_keys": list(sec.get("load_keys") or []), "interpolation": "bilinear",
            "dims_interpolation": "bilinear", "pad": None, "rotation": None, "jitter": None}

    def span(name, value, centre, lo_bound, hi_bound):
        """torchvision's _check_input / _setup_angle: a number v -> (centre - v, centre + v), a pair as given"""
        if isinstance(value, (int, float)) and not isinstance(value, bool):
            if value < 0:
                raise OutOfScopeError(f"train_section_plan: {name} {value!r} {where}: a number must not be negative")
            lo, hi = centre - float(value), centre + float(value)
            if name != "degrees" and centre == 1.0:
                lo = max(lo, 0.0)
        elif isinstance(value, (list, tuple)) and len(value) == 2 and value[0] <= value[1]:
            lo, hi = float(value[0]), float(value[1])
        else:
            raise OutOfScopeError(f"train_section_plan: {name} {value!r} {where}: a number or a pair lo <= hi")
        if lo < lo_bound or hi > hi_bound:
            raise OutOfScopeError(f"train_section_plan: {name} {value!r} {where}: outside [{lo_bound}, {hi_bound}]")
        return None if lo == hi == centre else (lo, hi)

    stage = -1
    for spec in sec.get("transforms") or []:
        path = spec["class_path"] if is_spec(spec) else str(spec)
        name, args = path.rsplit(".", 1)[-1], (spec.get("init_args") or {}) if is_spec(spec) else {}
        if not path.startswith("data_modules.transforms.") or name not in _SECTION_ORDER:
            raise OutOfScopeError(f"train_section_plan: {path} {where} is outside the device data step "
                                  f"({' / '.join(_SECTION_ORDER)})")
        if _SECTION_ORDER.index(name) <= stage:
            raise OutOfScopeError(f"train_section_plan: {path} {where} comes out of the order {' -> '.join(_SECTION_ORDER)}")
        stage = _SECTION_ORDER.index(name)
        extra = set(args) - _SECTION_ARGS[name]
        if extra:
            raise OutOfScopeError(f"train_section_plan: {path} {where} with {sorted(extra)} is outside the device data step")
        if name in ("RandomRotation", "ColorJitter") and args.get("apply_keys", "all") != "all":
            raise OutOfScopeError(f"train_section_plan: {name} with apply_keys {args['apply_keys']!r} {where}: the device path "
                                  f"takes it on all keys")
        if name == "RandomRotation":
            is_zero = lambda v: isinstance(v, int) and not isinstance(v, bool) and v == 0  # noqa: E731
            is_nearest = lambda v: is_zero(v) or (isinstance(v, str) and v.lower() == "nearest")  # noqa: E731
            defaults = {"expand": args.get("expand") in (None, False),
                        "center": args.get("center") is None,
                        "fill": args.get("fill") is None or is_zero(args.get("fill")),
                        "interpolation": args.get("interpolation") is None or is_nearest(args.get("interpolation")),
                        # older torchvision's name for the filter; its default was False
                        "resample": args.get("resample") in (None, False) or is_nearest(args.get("resample"))}
            for k, is_default in defaults.items():
                if not is_default:
                    raise OutOfScopeError(f"train_section_plan: RandomRotation with {k} {args[k]!r} {where}: the device rotation is "
                                          f"Pillow's NEAREST about the centre, no expand, fill 0")
            if "degrees" not in args:
                raise OutOfScopeError(f"train_section_plan: RandomRotation without degrees {where}")
            deg = span("degrees", args["degrees"], 0.0, -360.0, 360.0)
            plan["rotation"] = {"degrees": deg if deg is not None else (0.0, 0.0)}
        elif name == "RandomCrop":
            plan["crop_size"], plan["cat_max_ratio"] = pair(args["size"]), float(args.get("cat_max_ratio", 1.0))
        elif name == "ColorJitter":
            plan["jitter"] = {k: span(k, args.get(k, 0), 1.0, 0.0, float("inf")) for k in ("brightness", "contrast", "saturation")}
            plan["jitter"].update(hue=span("hue", args.get("hue", 0), 0.0, -0.5, 0.5), shuffle=False, blur=None)
        elif name == "RandomHorizontalFlip":
            plan["flip"] = float(args.get("p", 0.5))
        elif name == "Normalize":
            plan["mean"], plan["std"] = tuple(args.get("mean", IMNET_MEAN)), tuple(args.get("std", IMNET_STD))
    return plan


# the matcher's training section (configs/megadepth/uawarpc_stage*.yaml), in its order; the photometric three are optional
_MATCHING_ORDER = ("ToTensor", "ColorJitter", "ChannelShuffle", "RandomGaussianBlur", "ConvertImageDtype", "Normalize",
                   "CompositeFlow", "CenterCrop")
_MATCHING_READER_KEYS = ("load_keys", "dims", "exchange_images_with_proba", "store_scene_info_in_memory")


def matching_train_plan(cfg, dataset="MegaDepth"):
    """One training section `data.init_args.load_config.train[dataset]` of the matcher, whose pipeline is
        ToTensor -> [ColorJitter -> ChannelShuffle -> RandomGaussianBlur on image_prime] -> ConvertImageDtype -> Normalize
        -> CompositeFlow(image_prime) -> CenterCrop
    as what datamodule.MatchingDataModule runs:
      reader        the reader's keywords as the section gives them (load_keys, dims, exchange_images_with_proba,
                    store_scene_info_in_memory)
      dims          the load-time size (h, w)
      crop          CenterCrop's size (h, w), applied to every key
      mean / std    Normalize's statistics (ImageNet's by default)
      photometric   photometric_plan(cfg), or None for a section without the three photometric transforms
      warp          warp_supervision_plan(cfg)
    OutOfScopeError names the cause: a transform outside the chain, out of its order or twice; a section without image_prime
    among its load_keys, without dims, without CompositeFlow or without the CenterCrop after it; and whatever photometric_plan
    and warp_supervision_plan refuse (apply_keys other than ['image_prime'], hue, parameterize_with_gaussian, ...)."""
    from .datastep import IMNET_MEAN, IMNET_STD
    try:
        sec = cfg["data"]["init_args"]["load_config"]["train"][dataset]
    except (KeyError, TypeError) as e:
        raise KeyError(f"matching_train_plan: no data.init_args.load_config.train.{dataset} in this config") from e
    where = f"(train.{dataset})"
    if not isinstance(sec, dict):
        raise OutOfScopeError(f"matching_train_plan: {where} is a list of sections: pass a config that holds the one meant")
    keys = list(sec.get("load_keys") or [])
    if "image_prime" not in keys or "image" not in keys or "image_ref" not in keys:
        raise OutOfScopeError(f"matching_train_plan: load_keys {keys} {where}: image, image_ref and image_prime are what the "
                              f"matcher's training step reads (no image_prime: no warp supervision)")
    if sec.get("dims") is None:
        raise OutOfScopeError(f"matching_train_plan: no dims {where}: the batch needs one load-time size")
    stage, seen = -1, []
    mean, std = tuple(IMNET_MEAN), tuple(IMNET_STD)
    for spec in sec.get("transforms") or []:
        path = spec["class_path"] if is_spec(spec) else str(spec)
        name, args = path.rsplit(".", 1)[-1], (spec.get("init_args") or {}) if is_spec(spec) else {}
        if not path.startswith("data_modules.transforms.") or name not in _MATCHING_ORDER:
            raise OutOfScopeError(f"matching_train_plan: {path} {where} is outside the matcher's pipeline "
                                  f"({' / '.join(_MATCHING_ORDER)})")
        if name in seen:
            raise OutOfScopeError(f"matching_train_plan: a second {name} {where}")
        if _MATCHING_ORDER.index(name) < stage:
            raise OutOfScopeError(f"matching_train_plan: {name} {where} comes out of the order {' -> '.join(_MATCHING_ORDER)}")
        stage = _MATCHING_ORDER.index(name)
        seen.append(name)
        if name in ("ToTensor", "ConvertImageDtype") and args:
            raise OutOfScopeError(f"matching_train_plan: {name} with {sorted(args)} {where}")
        if name == "Normalize":
            extra = set(args) - {"mean", "std"}
            if extra:
                raise OutOfScopeError(f"matching_train_plan: Normalize with {sorted(extra)} {where}")
            mean, std = tuple(args.get("mean", IMNET_MEAN)), tuple(args.get("std", IMNET_STD))
    for name in ("ToTensor", "ConvertImageDtype", "Normalize", "CompositeFlow", "CenterCrop"):
        if name not in seen:
            raise OutOfScopeError(f"matching_train_plan: no data_modules.transforms.{name} {where}")
    one = {"data": {"init_args": {"load_config": {"train": {dataset: sec}}}}}
    photo = None
    if any(n in seen for n in _PHOTOMETRIC_ORDER):
        photo = photometric_plan(one, "train", dataset)
    warp = warp_supervision_plan(one, "train", dataset)
    dims = tuple(int(v) for v in sec["dims"])
    crop = warp["crop"]
    if crop[0] > dims[0] or crop[1] > dims[1]:
        raise OutOfScopeError(f"matching_train_plan: CenterCrop {crop} of dims {dims} {where}: the crop does not pad")
    return {"reader": {k: sec[k] for k in _MATCHING_READER_KEYS if k in sec}, "dims": dims, "crop": crop, "mean": mean,
            "std": std, "photometric": photo, "warp": warp}

"""refign_amd/datamodule.py -- the `data:` section of a Cityscapes -> ACDC / Cityscapes -> Dark Zurich configuration, from a
directory of data sets to the batches Trainer.fit / validate / test / predict take.

SegmentationDataModule reads `data.init_args` the way the reference's CombinedDataModule.__init__ does (sections, idx_to_name,
batch sizes), builds the readers of refign_amd/datasets.py and feeds what exists already: config.train_section_plan /
config.ingest_plan, datastep.RareClassSourceSampler / RotatedLabelledSampler / PairSampler / UDABatchAssembler,
resample.EvalIngest.  No worker process.

Who does what:
  * every random draw and every piece of device work happens on the thread that calls next(): a second thread issuing HIP work
    would break a graph capture in progress, and draws made elsewhere would interleave with the step's own;
  * only opening and decoding files runs in a ThreadPoolExecutor (`num_workers` threads, the YAML's value, at most 16), into
    pinned buffers that are used again once the copy that read them has finished.

What is pinned, and what is not: the epoch's index order is torch's RandomSampler (epoch_permutation), the readers are the
reference's, and with prefetch=0 the `random` and torch streams are consumed in the reference's order for loaders without
workers (the first loader's samples one after the other, then the second's, then the third's, then the coin of
`ignore_every_second_semantic_training_batch`).  Lightning is not installed here: the order in which ITS loops create and advance the loaders' iterators
(and the base seed a DataLoader iterator draws for its workers) is not restated, so parity with a Lightning run's batches is
not claimed.

MatchingDataModule, at the end, is the same for the matcher's configurations (configs/megadepth/uawarpc_*.yaml): MegaDepth pairs
with warp supervision for AlignmentModel.training_step, MegaDepth / RobotCarMatching with their correspondences for
validate / test.  Same division of work between the threads, and again no new kernel."""
import collections
import os
import random
from concurrent.futures import ThreadPoolExecutor

import torch

from . import config
from .datasets import SEGMENTATION_READERS as READERS

MAX_WORKERS = 16
_EVAL_KEYS = ("dims", "resize", "img_only", "only_if_larger", "mean", "std", "interpolation", "dims_interpolation", "pad")
_SPLITS = ("train", "val", "test", "predict")


def epoch_permutation(n):
    """One epoch's index order as torch.utils.data.RandomSampler draws it: one int64 seed from the global torch stream, then
    torch.randperm under a generator of its own."""
    seed = int(torch.empty((), dtype=torch.int64).random_().item())
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()


def _sections(load_config, split):
    """[(data set, section)] of a split: a dict is one section, a list under a data set several"""
    out = []
    for ds, conf in (load_config.get(split) or {}).items():
        if isinstance(conf, dict):
            out.append((ds, conf))
        elif isinstance(conf, list):
            out.extend((ds, el) for el in conf)
    return out


def _one_section_cfg(split, name, conf):
    """a config that holds this one section where the plan readers of refign_amd/config.py look for it"""
    return {"data": {"init_args": {"load_config": {split: {name: conf}}}}}


class SemiSupervisedOnly(config.OutOfScopeError, ValueError):
    """`ignore_every_second_semantic_training_batch` over one labelled section: the reference's assertion ("can only ignore in
    semi-supervised case") as a ValueError, and, like every shape of sections this module does not assemble, an OutOfScopeError"""


class _PinnedPool:
    """uint8 pinned host buffers by shape.  A buffer comes back with the event behind the copy that read it; it is handed out
    again after that event (waited for on the host, by the thread that asks)."""

    def __init__(self, pin):
        self.pin, self.free = pin, collections.defaultdict(list)

    def take(self, shape):
        shape = tuple(int(v) for v in shape)
        if self.free[shape]:
            buf, ev = self.free[shape].pop(0)
            if ev is not None:
                ev.synchronize()
            return buf
        return torch.empty(shape, dtype=torch.uint8, pin_memory=self.pin)

    def give(self, bufs, ev):
        for b in bufs:
            self.free[tuple(b.shape)].append((b, ev))


class _Source:
    """what UDABatchAssembler asks of its source: `size` and sample(out_image, out_label); hands the sampler the (class, index)
    pairs that were drawn ahead, when there are any"""

    def __init__(self, sampler):
        self.sampler, self.size, self.chosen = sampler, sampler.size, collections.deque()

    def sample(self, out_image=None, out_label=None):
        return self.sampler.sample(out_image, out_label, chosen=self.chosen.popleft() if self.chosen else None)


class _EvalLoader:
    """One evaluation section: decoded files through EvalIngest, stacked to the split's batch size, with `filename`.  Can be
    iterated again (Trainer.fit validates more than once).  With a pool the next batch's files are decoded meanwhile."""

    def __init__(self, reader, ingest, batch_size, pool):
        self.reader, self.ingest, self.b, self.pool = reader, ingest, int(batch_size), pool

    def __len__(self):
        return -(-len(self.reader) // self.b)

    def _decode(self, start):
        idx = range(start, min(start + self.b, len(self.reader)))
        if self.pool is None:
            return [self.reader.decode(i) for i in idx]
        return [self.pool.submit(self.reader.decode, i) for i in idx]

    def __iter__(self):
        starts = list(range(0, len(self.reader), self.b))
        ahead = self._decode(starts[0]) if starts else None
        for n, start in enumerate(starts):
            now, ahead = ahead, (self._decode(starts[n + 1]) if n + 1 < len(starts) else None)
            parts = []
            for s in now:
                s = s if isinstance(s, dict) else s.result()
                parts.append(self.ingest(s["image"], semantic=s.get("semantic"), image_ref=s.get("image_ref")))
            batch = {k: (parts[0][k] if len(parts) == 1 else torch.cat([p[k] for p in parts], dim=0)) for k in parts[0]}
            batch["filename"] = [self.reader.filename(i) for i in range(start, min(start + self.b, len(self.reader)))]
            yield batch


class SegmentationDataModule:
    """SegmentationDataModule(cfg, data_dir, device, prefetch=None): `cfg` is the loaded YAML; the data sets lie in
    <data_dir>/Cityscapes, /ACDC, /DarkZurich, /RobotCar, /NighttimeDriving and /BDD100kNight.
      train_on / val_on / test_on / predict_on, idx_to_name, batch_size, val_batch_size, test_batch_size: as CombinedDataModule
      train_batches()              an endless iterator of {image_src, semantic_src, image_trg, image_ref} on the device
      loaders(split, datasets)     {data set: iterable of batches} for Trainer.validate / test / predict
      orig_dims[name]              the size Trainer.predict(orig_size=) interpolates to, for the data sets the configuration names
      close()                      ends the decoding threads
    A data set without a reader here (MegaDepth, RobotCarMatching: the matcher's) or without its folder under data_dir raises
    config.OutOfScopeError naming the section when the section is asked for, not before; loaders(split, datasets=[...]) picks
    sections.
    Training sections: one rcs_enabled Cityscapes section, optionally one further labelled section (RobotCar's, whatever
    config.train_section_plan accepts: datastep.RotatedLabelledSampler with the reader's label_lut()), one (image, image_ref)
    section; a list under a data set (RobotCar's) gives one loader per entry, and a loader's batch is batch_size // loaders.
    `ignore_every_second_semantic_training_batch`: after a batch's samples ONE random.random() < 0.5 is drawn in next(); on
    heads image_src / semantic_src are views of the first half (the Cityscapes samples) of the assembled buffers.
    prefetch=0: files are decoded inside next(), and `random` is consumed in the reference's order.  prefetch=k > 0 (2 by default
    when the YAML's num_workers > 0): files are decoded k batches ahead, within the epoch.  The target indices are known from the
    permutation, and so are the second labelled section's; the source loader's (class, file) choices are drawn ahead from a random.Random of its own, seeded once from the
    global stream at the first next(); crop and flip draws stay in next(), on the global stream."""


    def __init__(self, cfg, data_dir, device, prefetch=None):
        args = dict(((cfg or {}).get("data") or {}).get("init_args") or {})
        self.cfg, self.data_dir, self.device = cfg, str(data_dir), torch.device(device)
        self.load_config = args.get("load_config") or {}
        self.num_workers = min(max(int(args.get("num_workers", 0)), 0), MAX_WORKERS)
        batch_size, divisor = int(args.get("batch_size", 8)), int(args.get("batch_size_divisor", 1))
        assert batch_size % divisor == 0, "batch_size must be divisible by batch_size_divisor"
        self.batch_size = batch_size // divisor
        self.pin_memory = bool(args.get("pin_memory", True))
        self.ignore_every_second_semantic_training_batch = bool(args.get("ignore_every_second_semantic_training_batch", False))
        self._sec = {split: _sections(self.load_config, split) for split in _SPLITS}
        self.train_on, self.val_on = [n for n, _ in self._sec["train"]], [n for n, _ in self._sec["val"]]
        self.test_on, self.predict_on = [n for n, _ in self._sec["test"]], [n for n, _ in self._sec["predict"]]
        self.idx_to_name = {split: {i: n for i, (n, _) in enumerate(self._sec[split])} for split in _SPLITS}
        # of the data sets this configuration names (and that have a reader here)
        self.orig_dims = {n: READERS[n].orig_dims for split in _SPLITS for n, _ in self._sec[split] if n in READERS}
        if self.train_on:
            assert self.batch_size % len(self.train_on) == 0, "batch size should be divisible by number of train datasets"
        self.val_batch_size = max(1, self.batch_size // max(len(self.train_on), 1) // 2)
        self.test_batch_size = 1
        self.prefetch = (2 if self.num_workers > 0 else 0) if prefetch is None else int(prefetch)
        if self.prefetch < 0:
            raise ValueError("SegmentationDataModule: prefetch must not be negative")
        self._pool = None
        self._iters = []

    # -- shared ------------------------------------------------------------------------------------------------------------
    def _executor(self):
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max(1, self.num_workers), thread_name_prefix="refign-decode")
        return self._pool

    def _reader(self, split, name, conf):
        if name not in READERS:
            raise config.OutOfScopeError(f"SegmentationDataModule: {name} ({split}) has no reader here ({' / '.join(READERS)}); "
                                         f"select the supported sections with datasets=")
        root = f"{self.data_dir}/{name}"
        if not os.path.isdir(root):
            # a configuration may name more data sets than a user holds (the Dark Zurich files test on three): the section is
            # named, and so is the way round it.  (OutOfScopeError is a RuntimeError, as the readers' own for a missing folder.)
            raise config.OutOfScopeError(f"SegmentationDataModule: {name} ({split}): dataset not found: there is no folder {root}; "
                                         f"select the sections to run with datasets=")
        kwargs = {k: v for k, v in conf.items() if k != "transforms"}
        return READERS[name](root, stage=split, **kwargs)

    def close(self):
        """ends the iterators' look-ahead and the decoding threads (waits for them)"""
        for it in self._iters:
            it.close()
        self._iters = []
        if self._pool is not None:
            self._pool.shutdown(wait=True, cancel_futures=True)
            self._pool = None

    # -- evaluation ----------------------------------------------------------------------------------------------------------
    def loaders(self, split, datasets=None):
        """{data set: iterable of batches} in idx_to_name[split]'s order.  A batch: resample.EvalIngest(**config.ingest_plan(cfg,
        split, name)) over the decoded files, stacked to the split's batch size (val: val_batch_size; test / predict: 1), plus
        `filename` (a list).  datasets: the names to keep (every section by default)."""
        if split not in ("val", "test", "predict"):
            raise ValueError(f"SegmentationDataModule.loaders: split must be 'val', 'test' or 'predict', got {split!r}")
        from .resample import EvalIngest
        out = {}
        for name, conf in self._sec[split]:
            if datasets is not None and name not in datasets:
                continue
            if name in out:
                raise config.OutOfScopeError(f"SegmentationDataModule: two sections of {name} in {split}: the loaders and the "
                                             f"metrics are named by data set")
            reader = self._reader(split, name, conf)
            plan = config.ingest_plan(_one_section_cfg(split, name, conf), split, name)
            kw = {k: plan[k] for k in _EVAL_KEYS}
            if kw["dims"] is None:
                kw["dims"] = tuple(reader.dims)                     # the reader's own default, which it resizes to as well
            lut = reader.label_lut() if hasattr(reader, "label_lut") else None   # RobotCar: raw ids, encoded on the device
            ingest = EvalIngest(device=self.device, label_lut=lut, **kw)
            out[name] = _EvalLoader(reader, ingest, self.val_batch_size if split == "val" else self.test_batch_size,
                                    self._executor() if self.num_workers > 0 else None)
        return out

    # -- training ------------------------------------------------------------------------------------------------------------
    def train_batches(self):
        """An endless iterator of training batches.  Per epoch and per loader (the source's, then the target's) one
        epoch_permutation is drawn when the epoch's first batch is asked for; the epoch has min over the loaders of
        len // per-loader batch size batches (`drop_last`, `multiple_trainloader_mode: min_size`).  Under rcs_enabled the source
        loader ignores its indices.  A yielded batch has been waited for on the current stream; its buffers are written again two
        batches later, after the work that was queued on the current stream by then (UDABatchAssembler.consumed for the batch that
        held them), which fits Trainer.fit's look-ahead of one batch as well as a plain `for batch in ...: step(batch)`."""
        readers = [self._reader("train", name, conf) for name, conf in self._sec["train"]]
        if self.ignore_every_second_semantic_training_batch and sum("semantic" in r.load_keys for r in readers) < 2:
            # the reference asserts len(image_src) > batch_size // len(train_on) in on_before_batch_transfer
            raise SemiSupervisedOnly("SegmentationDataModule: ignore_every_second_semantic_training_batch with one labelled "
                                     "training section: can only ignore in semi-supervised case")
        if self.device.type != "cuda":
            raise RuntimeError("SegmentationDataModule.train_batches: a HIP device is required (no CPU fallback)")
        it = _TrainIterator(self, readers)
        self._iters.append(it)
        return it


class _TrainIterator:
    def __init__(self, dm, readers):
        from .datastep import PairSampler, RareClassSourceSampler, RotatedLabelledSampler, UDABatchAssembler
        self.dm = dm
        secs = dm._sec["train"]
        plans = [config.train_section_plan(_one_section_cfg("train", name, conf), name) for name, conf in secs]
        src = [i for i, r in enumerate(readers) if "semantic" in r.load_keys]
        trg = [i for i, r in enumerate(readers) if "semantic" not in r.load_keys]
        if len(src) not in (1, 2) or len(trg) != 1 or not {"image", "image_ref"} <= set(readers[trg[0]].load_keys):
            raise config.OutOfScopeError(f"SegmentationDataModule: training sections {[n for n, _ in secs]}: one rare-class source "
                                         f"section, optionally one further labelled section, and one (image, image_ref) target "
                                         f"section is what the device data step assembles")
        s, t = src[0], trg[0]
        lab = src[1] if len(src) == 2 else None
        if src[-1] > t:
            raise config.OutOfScopeError(f"SegmentationDataModule: training sections {[n for n, _ in secs]}: the labelled sections "
                                         f"come first in every configuration carried here (their samples draw first)")
        self.src, self.trg = readers[s], readers[t]
        self.lab = None if lab is None else readers[lab]
        if not getattr(self.src, "rcs_enabled", False):
            raise config.OutOfScopeError(f"SegmentationDataModule: train.{secs[s][0]} without rcs_enabled: the first labelled "
                                         f"section's sampler on the device is the rare-class one")
        if lab is not None and getattr(self.lab, "rcs_enabled", False):
            raise config.OutOfScopeError(f"SegmentationDataModule: train.{secs[lab][0]}: a second rcs_enabled section")
        for i in (s, t):
            plan = plans[i]
            if plan["crop_size"] is None or plan["flip"] != 0.5 or plan["rotation"] is not None or plan["jitter"] is not None:
                raise config.OutOfScopeError(f"SegmentationDataModule: train.{secs[i][0]}: RandomCrop + RandomHorizontalFlip(p=0.5) "
                                             f"is the pipeline the rare-class and the pair sampler run")
        if lab is not None and (plans[lab]["crop_size"] is None or tuple(plans[lab]["crop_size"]) != tuple(plans[s]["crop_size"])):
            raise config.OutOfScopeError(f"SegmentationDataModule: train.{secs[lab][0]}: the two labelled sections share image_src, "
                                         f"so they need one RandomCrop size ({plans[lab]['crop_size']} and {plans[s]['crop_size']})")
        self.per_loader = dm.batch_size // len(secs)
        dims = [tuple(plans[i]["dims"] or readers[i].dims) for i in (s, t)]
        self.source = _Source(RareClassSourceSampler(
            self._load_src, self.src.rcs_classes, self.src.rcs_classprob, self.src.indices_with_class, plans[s]["crop_size"],
            dm.device, cat_max_ratio=plans[s]["cat_max_ratio"], rcs_min_pixels=self.src.rcs_min_pixels,
            rcs_min_crop_ratio=self.src.rcs_min_crop_ratio, mean=plans[s]["mean"], std=plans[s]["std"], dims=dims[0]))
        self.pairs = PairSampler(self._load_trg, plans[t]["crop_size"], dm.device, mean=plans[t]["mean"], std=plans[t]["std"],
                                 dims=dims[1])
        self.labelled = None
        if lab is not None:
            lut = self.lab.label_lut() if hasattr(self.lab, "label_lut") else None
            self.labelled = RotatedLabelledSampler(self._load_lab, dict(plans[lab], dims=tuple(plans[lab]["dims"] or self.lab.dims)),
                                                   dm.device, label_lut=lut)
        self.asm = UDABatchAssembler(self.source, self.pairs, self.per_loader, dm.device, labelled=self.labelled)
        self.halve = dm.ignore_every_second_semantic_training_batch
        self.halved = 0                                      # batches handed out with the first half of the source samples
        self.n_batches = min(len(r) for r in readers) // self.per_loader
        if self.n_batches == 0:
            raise ValueError("SegmentationDataModule: a training set holds fewer files than one loader's batch")
        self.pool = _PinnedPool(dm.pin_memory)
        self.k = dm.prefetch
        self.exe = dm._executor() if self.k > 0 else None
        self.private = None                                  # the source loader's own stream (prefetch > 0)
        self.order, self.pos = [], 0                         # the epoch's target indices and the next one to plan
        self.lab_order = []                                  # ... and the second labelled loader's
        self.pending = collections.deque()                   # planned batches: {"src": [...], "lab": [...], "trg": [...], "bufs"}
        self.current = None
        self.handed = collections.deque(maxlen=2)
        self.sizes = {}
        self.epoch, self.host_seconds = 0, 0.0

    def __iter__(self):
        return self

    # -- decoding ------------------------------------------------------------------------------------------------------------
    def _job(self, reader, which, index, bufs):
        """start (or, without threads, do) the decoding of one file set into pinned buffers -> a future or the sample"""
        key = (which, index)
        if key not in self.sizes:
            self.sizes[key] = {k: reader.size(index, k) for k in reader.load_keys}
        out = {}
        for k, (h, w) in self.sizes[key].items():
            out[k] = self.pool.take((h, w) if k == "semantic" else (h, w, 3))
            bufs.append(out[k])
        views = {k: v.numpy() for k, v in out.items()}
        if self.exe is None:
            reader.decode(index, views)
            return out
        return self.exe.submit(lambda: (reader.decode(index, views), out)[1])

    @staticmethod
    def _done(x):
        return x if isinstance(x, dict) else x.result()

    def _load_src(self, index):
        cur = self.current
        s = self._done(cur["src"].popleft()[2]) if cur["src"] else self._job(self.src, "src", index, cur["bufs"])
        return s["image"], s["semantic"]

    def _load_lab(self, index):
        cur = self.current
        s = self._done(cur["lab"].popleft()[1]) if cur["lab"] else self._job(self.lab, "lab", index, cur["bufs"])
        return s["image"], s["semantic"]

    def _load_trg(self, index):
        cur = self.current
        s = self._done(cur["trg"].popleft()[1]) if cur["trg"] else self._job(self.trg, "trg", index, cur["bufs"])
        return s["image"], s["image_ref"]

    # -- planning ------------------------------------------------------------------------------------------------------------
    def _new_epoch(self):
        epoch_permutation(len(self.src))                     # the source loader's: drawn, and ignored under rcs_enabled
        if self.lab is not None:                             # one permutation per loader, in loader order
            self.lab_order = epoch_permutation(len(self.lab))[:self.n_batches * self.per_loader]
        self.order = epoch_permutation(len(self.trg))[:self.n_batches * self.per_loader]
        self.pos = 0
        self.epoch += 1

    def _plan(self):
        """one more batch of the current epoch: its target (and second labelled) indices; with prefetch, its source choices
        and its decoding jobs"""
        idx = self.order[self.pos:self.pos + self.per_loader]
        lab_idx = self.lab_order[self.pos:self.pos + self.per_loader] if self.lab is not None else None
        self.pos += self.per_loader
        entry = {"indices": idx, "lab_indices": lab_idx, "src": collections.deque(), "lab": collections.deque(),
                 "trg": collections.deque(), "bufs": []}
        if self.k > 0:
            sam = self.source.sampler
            for _ in range(self.per_loader):
                c = self.private.choices(sam.rcs_classes, weights=sam.rcs_classprob, k=1)[0]
                i = self.private.choice(sam.indices_with_class[c])
                entry["src"].append((c, i, self._job(self.src, "src", i, entry["bufs"])))
            for i in lab_idx or ():
                entry["lab"].append((i, self._job(self.lab, "lab", i, entry["bufs"])))
            for i in idx:
                entry["trg"].append((i, self._job(self.trg, "trg", i, entry["bufs"])))
        self.pending.append(entry)

    def __next__(self):
        import time
        t0 = time.perf_counter()
        if self.k > 0 and self.private is None:
            self.private = random.Random(random.getrandbits(64))
        if not self.pending:
            if self.pos >= len(self.order):
                self._new_epoch()
            self._plan()
        cur = self.current = self.pending.popleft()
        while self.k > 0 and len(self.pending) < self.k and self.pos < len(self.order):
            self._plan()
        if len(self.handed) == 2:                            # the set that is written next was handed out two batches ago
            self.asm.consumed(self.handed[0])
        self.source.chosen.extend((c, i) for c, i, _ in cur["src"])
        batch, ev = self.asm.assemble(cur["indices"], cur["lab_indices"])
        self.pool.give(cur["bufs"], ev)
        torch.cuda.current_stream(self.dm.device).wait_event(ev)
        if self.halve and random.random() < 0.5:             # the reference's coin, after every sample's draws, on this thread
            n = batch["image_src"].shape[0] // 2             # views: the buffers stay the assembler's (consumed() knows them)
            batch = dict(batch, image_src=batch["image_src"][:n], semantic_src=batch["semantic_src"][:n])
            self.halved += 1
        self.handed.append(batch)
        self.current = None
        self.host_seconds += time.perf_counter() - t0
        return batch

    def close(self):
        for entry in self.pending:
            for job in [j[-1] for j in list(entry["src"]) + list(entry["lab"]) + list(entry["trg"])]:
                if not isinstance(job, dict) and not job.cancel():
                    job.result()
        self.pending.clear()


# ---------------------------------------------------------------------------------------------------------------------------
# The matcher's `data:` section (configs/megadepth/uawarpc_*.yaml): MegaDepth pairs with warp supervision for training,
# MegaDepth / RobotCarMatching with their sparse correspondences for evaluation.
class _PinnedArena:
    """uint8 pinned host buffers by CAPACITY: a request is rounded up to a multiple of `step` bytes and served by a flat buffer
    of that many bytes, viewed at the shape asked for.  MegaDepth's files have hundreds of sizes; staging memory grows with the
    number of capacity classes in flight, not with the number of shapes seen.  A buffer comes back with the event behind the copy
    that read it and is handed out again after that event (waited for on the host, by the thread that asks)."""
    STEP = 1 << 20

    def __init__(self, pin, step=STEP):
        self.pin, self.step, self.free, self.allocated = pin, int(step), collections.defaultdict(list), 0

    def take(self, shape):
        """-> (the flat buffer, to give back; its view at `shape`)"""
        shape = tuple(int(v) for v in shape)
        n = 1
        for v in shape:
            n *= v
        cap = max(1, -(-n // self.step)) * self.step
        if self.free[cap]:
            buf, ev = self.free[cap].pop(0)
            if ev is not None:
                ev.synchronize()
        else:
            buf = torch.empty(cap, dtype=torch.uint8, pin_memory=self.pin)
            self.allocated += cap
        return buf, buf[:n].view(shape)

    def give(self, bufs, ev):
        for b in bufs:
            self.free[b.numel()].append((b, ev))


def _exchange_coin(rng, proba):
    """the reference's `random.random() < self.exchange_images_with_proba`: thrown whatever the probability"""
    return rng.random() < proba


class _MatchingEvalLoader:
    """One evaluation section of the matcher: decoded pairs through EvalIngest (which scales the points with each resize),
    images stacked to the split's batch size, `corr_pts` / `corr_pts_ref` lists of per-sample (n, 2) device tensors (the
    reference's my_collate), plus `filename`.  Can be iterated again.  `coin`: the section's samples throw the exchange coin
    (MegaDepth's val split), on the calling thread, in file order, one batch ahead of the decoding at most."""

    def __init__(self, reader, ingest, batch_size, pool, coin):
        self.reader, self.ingest, self.b, self.pool, self.coin = reader, ingest, int(batch_size), pool, coin

    def __len__(self):
        return -(-len(self.reader) // self.b)

    def _decode(self, start):
        jobs = []
        for i in range(start, min(start + self.b, len(self.reader))):
            ex = _exchange_coin(random, self.reader.exchange_images_with_proba) if self.coin else False
            jobs.append(self.reader.decode(i, ex) if self.pool is None else self.pool.submit(self.reader.decode, i, ex))
        return jobs

    def __iter__(self):
        starts = list(range(0, len(self.reader), self.b))
        ahead = self._decode(starts[0]) if starts else None
        for n, start in enumerate(starts):
            now, ahead = ahead, (self._decode(starts[n + 1]) if n + 1 < len(starts) else None)
            parts = []
            for s in now:
                s = s if isinstance(s, dict) else s.result()
                parts.append(self.ingest(s["image"], image_ref=s["image_ref"], corr_pts=s["corr_pts"],
                                         corr_pts_ref=s["corr_pts_ref"]))
            if len({tuple(p[k].shape) for p in parts for k in ("image", "image_ref")}) > 1:
                raise ValueError(f"MatchingDataModule: a batch of {len(parts)} images of different sizes cannot be stacked: give the "
                                 f"section dims, or a batch size of 1")
            batch = {k: (parts[0][k] if len(parts) == 1 else torch.cat([p[k] for p in parts], dim=0)) for k in ("image", "image_ref")}
            for k in ("corr_pts", "corr_pts_ref"):
                batch[k] = [t for p in parts for t in p[k]]
            batch["filename"] = [self.reader.filename(i) for i in range(start, min(start + self.b, len(self.reader)))]
            yield batch


class MatchingDataModule:
    """MatchingDataModule(cfg, data_dir, device, prefetch=None): `cfg` is the loaded YAML of a matcher configuration; the data
    sets lie in <data_dir>/MegaDepth (<data_dir>/MegaDepth_debug under `debug: true`) and <data_dir>/RobotCarMatching.
      train_on / val_on / test_on / predict_on, idx_to_name, batch_size, val_batch_size, test_batch_size: as CombinedDataModule
      train_batches()              an endless iterator of {image_ref, image_trg, image_prime, flow_prime, mask_prime,
                                   prime_trg_idx} on the device: what AlignmentModel.training_step reads
      loaders(split, datasets)     {data set: iterable of batches} for Trainer.validate / test
      close()                      ends the decoding threads
    Training, per sample: the exchange coin, the two files decoded, image_ref through resize_crop_flip_normalize (Lanczos to
    `dims`, the centre crop) into its batch slot, the target resized once (resize_u8, Lanczos) -- that uint8 frame is
    image_prime's input, and image_trg is its crop_flip_normalize -- then the sample's photometric and composite draws; one
    WarpSupervision call for the batch.  Per epoch the draws are epoch_permutation(len) (`drop_last`), then for the samples in
    batch order coin, photometric.draw, draw_composite: the reference's __getitem__-then-transforms order for one loader
    without workers.  prime_trg_idx is a device int64 tensor of ones (the prime image is always made from the target).
    prefetch=0: files are decoded inside next() and the coin is on the global `random` stream.  prefetch=k > 0 (2 by default when
    the YAML's num_workers > 0): files are decoded k batches ahead within the epoch, in at most min(num_workers, 16) threads; the
    coins are then drawn ahead from a random.Random of the loader's own, seeded once from the global stream at the first next().
    Every draw and all device work happen on the thread that calls next().
    Not here: worker processes, several ranks (every rank would read the same batches), parity with the batch order of a
    Lightning run, `predict` (OutOfScopeError: the reference's matcher has no predict_step)."""

    def __init__(self, cfg, data_dir, device, prefetch=None):
        args = dict(((cfg or {}).get("data") or {}).get("init_args") or {})
        self.cfg, self.data_dir, self.device = cfg, str(data_dir), torch.device(device)
        self.load_config = args.get("load_config") or {}
        self.debug = bool(args.get("debug", False))
        self.num_workers = min(max(int(args.get("num_workers", 0)), 0), MAX_WORKERS)
        batch_size, divisor = int(args.get("batch_size", 8)), int(args.get("batch_size_divisor", 1))
        assert batch_size % divisor == 0, "batch_size must be divisible by batch_size_divisor"
        self.batch_size = batch_size // divisor
        self.pin_memory = bool(args.get("pin_memory", True))
        self._sec = {split: _sections(self.load_config, split) for split in _SPLITS}
        self.train_on, self.val_on = [n for n, _ in self._sec["train"]], [n for n, _ in self._sec["val"]]
        self.test_on, self.predict_on = [n for n, _ in self._sec["test"]], [n for n, _ in self._sec["predict"]]
        self.idx_to_name = {split: {i: n for i, (n, _) in enumerate(self._sec[split])} for split in _SPLITS}
        if self.train_on:
            assert self.batch_size % len(self.train_on) == 0, "batch size should be divisible by number of train datasets"
        self.val_batch_size = max(1, self.batch_size // max(len(self.train_on), 1) // 2)
        self.test_batch_size = 1
        self.prefetch = (2 if self.num_workers > 0 else 0) if prefetch is None else int(prefetch)
        if self.prefetch < 0:
            raise ValueError("MatchingDataModule: prefetch must not be negative")
        self._pool = None
        self._iters = []

    def _executor(self):
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max(1, self.num_workers), thread_name_prefix="refign-decode")
        return self._pool

    def root(self, name):
        return f"{self.data_dir}/{name}" + ("_debug" if self.debug and name == "MegaDepth" else "")

    def _reader(self, split, name, conf):
        from .datasets import MATCHING_READERS
        if name not in MATCHING_READERS:
            raise config.OutOfScopeError(f"MatchingDataModule: {name} ({split}) has no reader here ({' / '.join(MATCHING_READERS)}); "
                                         f"select the supported sections with datasets=")
        kwargs = {k: v for k, v in conf.items() if k != "transforms"}
        if name == "MegaDepth":
            kwargs["debug"] = self.debug
        return MATCHING_READERS[name](self.root(name), stage=split, **kwargs)

    def close(self):
        """ends the iterators' look-ahead and the decoding threads (waits for them); harmless when called again"""
        for it in self._iters:
            it.close()
        self._iters = []
        if self._pool is not None:
            self._pool.shutdown(wait=True, cancel_futures=True)
            self._pool = None

    # -- evaluation ----------------------------------------------------------------------------------------------------------
    def loaders(self, split, datasets=None):
        """{data set: iterable of batches} in idx_to_name[split]'s order.  A batch: resample.EvalIngest(**config.ingest_plan(cfg,
        split, name)) over the decoded pairs -- image, image_ref stacked to the split's batch size (val: val_batch_size; test:
        1), corr_pts / corr_pts_ref as lists of per-sample (n, 2) device tensors in the pixels of the batch's images -- plus
        `filename`.  MegaDepth's val samples throw their exchange coin, as the reference's do.  datasets: the names to keep."""
        if split == "predict":
            raise config.OutOfScopeError("MatchingDataModule: predict is outside this module: the reference's matcher "
                                         "(AlignmentModel) has no predict_step")
        if split not in ("val", "test"):
            raise ValueError(f"MatchingDataModule.loaders: split must be 'val' or 'test', got {split!r}")
        from .resample import EvalIngest
        out = {}
        for name, conf in self._sec[split]:
            if datasets is not None and name not in datasets:
                continue
            if name in out:
                raise config.OutOfScopeError(f"MatchingDataModule: two sections of {name} in {split}: the loaders and the metrics "
                                             f"are named by data set")
            reader = self._reader(split, name, conf)
            plan = config.ingest_plan(_one_section_cfg(split, name, conf), split, name)
            kw = {k: plan[k] for k in _EVAL_KEYS}
            if kw["dims"] is None and reader.dims is not None:
                kw["dims"] = tuple(reader.dims)                     # the reader's own default (RobotCarMatching: 1024 x 1024)
            ingest = EvalIngest(device=self.device, **kw)
            out[name] = _MatchingEvalLoader(reader, ingest, self.val_batch_size if split == "val" else self.test_batch_size,
                                            self._executor() if self.num_workers > 0 else None,
                                            coin=getattr(reader, "split", "test") != "test")
        return out

    # -- training ------------------------------------------------------------------------------------------------------------
    def train_batches(self):
        """An endless iterator of training batches.  One epoch_permutation per epoch, drawn when the epoch's first batch is asked
        for; the epoch has len // batch_size batches (`drop_last`).  A yielded batch consists of fresh tensors made on the current
        stream: nothing writes to it again."""
        secs = self._sec["train"]
        if len(secs) != 1:
            raise config.OutOfScopeError(f"MatchingDataModule: training sections {[n for n, _ in secs]}: one MegaDepth section is "
                                         f"what the matcher's configurations train on")
        name, conf = secs[0]
        plan = config.matching_train_plan(_one_section_cfg("train", name, conf), name)
        reader = self._reader("train", name, conf)
        if self.device.type != "cuda":
            raise RuntimeError("MatchingDataModule.train_batches: a HIP device is required (no CPU fallback)")
        it = _MatchingTrainIterator(self, reader, plan)
        self._iters.append(it)
        return it


class _MatchingTrainIterator:
    def __init__(self, dm, reader, plan):
        from .flowsynth import WarpSupervision, crop_origin
        self.dm, self.reader, self.plan = dm, reader, plan
        self.b = dm.batch_size
        self.n_batches = len(reader) // self.b
        if self.n_batches == 0:
            raise ValueError("MatchingDataModule: the training set holds fewer pairs than one batch")
        self.dims, self.crop = plan["dims"], plan["crop"]
        self.top, self.left = crop_origin(*self.dims, *self.crop)
        self.supervise = WarpSupervision(plan["warp"], photometric=plan["photometric"])
        self.proba = reader.exchange_images_with_proba
        self.arena = _PinnedArena(dm.pin_memory)
        self.k = dm.prefetch
        self.exe = dm._executor() if self.k > 0 else None
        self.private = None                                  # the coins' own stream (prefetch > 0)
        self.order, self.pos = [], 0
        self.pending = collections.deque()                   # planned batches: {"indices", "jobs": [(exchange, job)], "bufs"}
        self.sizes = {}
        self.ones = torch.ones(self.b, dtype=torch.int64, device=dm.device)
        # clocks for tools/matching_datamodule_bench.py: all of next(); the decoding itself (summed over the threads); next()
        # waiting for a file (prefetch=0: decoding it); the photometric and composite draws
        self.epoch, self.batches = 0, 0
        self.host_seconds, self.decode_seconds, self.wait_seconds, self.draw_seconds = 0.0, 0.0, 0.0, 0.0

    def __iter__(self):
        return self

    def _job(self, index, exchange, bufs):
        """start (or, without threads, do) the decoding of one pair into pinned buffers -> a future or the sample"""
        key = (index, exchange)
        if key not in self.sizes:
            self.sizes[key] = self.reader.sizes(index, exchange)
        out = {}
        for k, (h, w) in self.sizes[key].items():
            buf, out[k] = self.arena.take((h, w, 3))
            bufs.append(buf)
        views = {k: v.numpy() for k, v in out.items()}

        def work():
            import time
            t0 = time.perf_counter()
            s = self.reader.decode(index, exchange, views)
            s.update(out)                                    # the pinned tensors in place of their numpy views
            s["decode_seconds"] = time.perf_counter() - t0
            return s
        return work() if self.exe is None else self.exe.submit(work)

    def _new_epoch(self):
        self.order = epoch_permutation(len(self.reader))[:self.n_batches * self.b]
        self.pos = 0
        self.epoch += 1

    def _plan(self):
        """one more batch of the current epoch: its indices; with prefetch, its coins and its decoding jobs"""
        entry = {"indices": self.order[self.pos:self.pos + self.b], "jobs": collections.deque(), "bufs": []}
        self.pos += self.b
        if self.k > 0:
            for i in entry["indices"]:
                ex = _exchange_coin(self.private, self.proba)
                entry["jobs"].append((ex, self._job(i, ex, entry["bufs"])))
        self.pending.append(entry)

    def __next__(self):
        import time
        from .datastep import crop_flip_normalize
        from .resample import resize_crop_flip_normalize, resize_u8
        t0 = time.perf_counter()
        dev, plan = self.dm.device, self.plan
        if self.k > 0 and self.private is None:
            self.private = random.Random(random.getrandbits(64))
        if not self.pending:
            if self.pos >= len(self.order):
                self._new_epoch()
            self._plan()
        cur = self.pending.popleft()
        while self.k > 0 and len(self.pending) < self.k and self.pos < len(self.order):
            self._plan()
        (Hd, Wd), (ch, cw) = self.dims, self.crop
        ref = torch.empty((self.b, 3, ch, cw), dtype=torch.float32, device=dev)
        trg = torch.empty((self.b, 3, ch, cw), dtype=torch.float32, device=dev)
        prime = torch.empty((self.b, 3, Hd, Wd), dtype=torch.uint8, device=dev)
        draws, exchanged = [], []
        for j, index in enumerate(cur["indices"]):
            t1 = time.perf_counter()
            if cur["jobs"]:
                ex, job = cur["jobs"].popleft()
                s = job if isinstance(job, dict) else job.result()
            else:
                ex = _exchange_coin(random, self.proba)
                s = self._job(index, ex, cur["bufs"])
            self.wait_seconds += time.perf_counter() - t1
            self.decode_seconds += s["decode_seconds"]
            exchanged.append(ex)
            a = s["image_ref"].to(dev, non_blocking=True)
            t = s["image"].to(dev, non_blocking=True)
            resize_crop_flip_normalize(a, self.dims, self.top, self.left, ch, cw, False, ref[j], plan["mean"], plan["std"],
                                       filter="lanczos")
            if tuple(t.shape[:2]) == (Hd, Wd):               # Pillow's reader leaves a file of that size as it is
                prime[j].copy_(t.permute(2, 0, 1))
            else:
                prime[j].copy_(resize_u8(t, self.dims, filter="lanczos"))
            crop_flip_normalize(prime[j], None, self.top, self.left, ch, cw, False, trg[j], None, plan["mean"], plan["std"])
            t1 = time.perf_counter()
            draws.append(self.supervise.draw(Hd, Wd))
            self.draw_seconds += time.perf_counter() - t1
        self.arena.give(cur["bufs"], torch.cuda.current_stream(dev).record_event())
        batch = self.supervise({"image": trg, "image_ref": ref, "image_prime": prime}, draws=draws)
        batch["prime_trg_idx"] = self.ones
        self.exchanged = exchanged
        self.batches += 1
        self.host_seconds += time.perf_counter() - t0
        return batch

    def close(self):
        for entry in self.pending:
            for _, job in entry["jobs"]:
                if not isinstance(job, dict) and not job.cancel():
                    job.result()
        self.pending.clear()

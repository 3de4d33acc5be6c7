"""Minimal one-process-per-GPU trainer that stands where PyTorch-Lightning's Trainer stands in the reference
(SURVEY.md L4): it owns the optimiser/scheduler, drives `training_step`, and implements the data-parallel part.

Data parallelism: image pairs are independent, so ranks shard the batch; align / refine / teacher are
gradient-free replicas with ZERO communication.  The student's gradients of the three backward passes of a step are
accumulated into one flat fp32 buffer (every `p.grad` is a view into it) and all-reduced ONCE per step with RCCL,
averaged over ranks -- the reference's DDP does the same reduction three times per step (once per manual_backward).
On xGMI (7 point-to-point links per GPU) one 342 MB all-reduce is bandwidth-bound; the flat buffer is laid out in
gradient-readiness order (decode heads + MiT stage 4, stage 3, stage 2, stage 1) and, during the LAST backward pass of
the step, each finished range is put on the RCCL stream in `bucket_mb` pieces while the backward of the earlier stages
is still running (marks in seg.MixVisionTransformer.forward_features); the remainder follows when the pass ends.
BatchNorm layers become SyncBatchNorm when the config says `sync_batchnorm: True` (student AND teacher, D9).
"""
import os
from typing import List

import torch
import torch.distributed as dist
import torch.nn as nn

from .params import mark_grad_sink

LIGHTNING_VERSION = "1.5.10"        # the checkpoint layout of Trainer.save_checkpoint (the reference's requirements.txt)
_OWN_KEY = "refign_amd"             # what that layout has no slot for
_IMPL_FLAGS = ("fused", "foreach", "capturable", "differentiable")   # AdamW flags that pick an implementation


def _rng_state(dev):
    """This process's host RNG states and its device generator's (numpy's key as a list: the file stays plain data)."""
    import random

    import numpy as np
    kind, key, pos, has_gauss, gauss = np.random.get_state()
    return {"python": random.getstate(), "numpy": (kind, key.tolist(), int(pos), int(has_gauss), float(gauss)),
            "torch": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None}


def _set_rng_state(st, dev):
    import random

    import numpy as np
    random.setstate(st["python"])
    kind, key, pos, has_gauss, gauss = st["numpy"]
    np.random.set_state((kind, np.asarray(key, dtype=np.uint32), pos, has_gauss, gauss))
    torch.set_rng_state(st["torch"])
    if dev.type == "cuda" and st.get("cuda") is not None:
        torch.cuda.set_rng_state(st["cuda"], dev)


def _seed_rank(global_step, rank):
    """Resume without saved RNG states: python, numpy, torch CPU and device generators seeded from (global_step, rank)."""
    import random

    import numpy as np
    seed = (int(global_step) * 1000003 + int(rank)) % 2 ** 32
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def _write_file(obj, f):
    """The serialiser of save_checkpoint (a name of its own: the tests slow it down and make it fail part-way)."""
    torch.save(obj, f)


def _atomic_save(obj, filepath):
    """`obj` to a temporary file next to `filepath`, flushed to the disk, then renamed over it: a reader sees the old file
    or the complete new one, never a part."""
    os.makedirs(os.path.dirname(os.path.abspath(filepath)), exist_ok=True)
    tmp = f"{filepath}.tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            _write_file(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, filepath)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def parse_gradient_clip(val, algorithm="norm"):
    """Lightning's `gradient_clip_val` / `gradient_clip_algorithm` -> (threshold or None, algorithm): None and 0 mean off; a
    negative value, a NaN or a non-number and an algorithm other than "norm" / "value" raise ValueError."""
    if algorithm not in ("norm", "value"):
        raise ValueError(f"Trainer: gradient_clip_algorithm must be 'norm' or 'value' (got {algorithm!r})")
    if val is None:
        return None, algorithm
    if isinstance(val, bool) or not isinstance(val, (int, float)) or not val >= 0:
        raise ValueError(f"Trainer: gradient_clip_val must be None or a number >= 0 (got {val!r})")
    return (float(val) or None), algorithm


def parse_accumulate(k):
    """Lightning's `accumulate_grad_batches` -> int >= 1.  Its per-epoch schedule (a dict) has no meaning for a trainer that
    counts steps only: that, like anything else that is no positive int, raises ValueError."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        what = "a per-epoch schedule (dict): this trainer has no epochs" if isinstance(k, dict) else repr(k)
        raise ValueError(f"Trainer: accumulate_grad_batches must be an int >= 1 (got {what})")
    return k


class LinearWarmupPolynomialLR(torch.optim.lr_scheduler.LRScheduler):
    """helpers/lr_scheduler.py:10-57: linear warm-up from warmup_ratio*lr over warmup_iters, then polynomial decay to
    min_lr at max_steps."""

    def __init__(self, optimizer, max_steps: int = None, warmup_iters: int = 1500, warmup_ratio: float = 1e-6,
                 power=0.9, min_lr=0., last_epoch=-1):
        self.max_updates, self.warmup_iters, self.warmup_ratio = max_steps, warmup_iters, warmup_ratio
        self.power, self.min_lr = power, min_lr
        super().__init__(optimizer, last_epoch)

    def get_lr(self) -> List[float]:
        t = self.last_epoch
        if t < self.warmup_iters:
            k = (1 - t / self.warmup_iters) * (1 - self.warmup_ratio)
            return [lr * (1 - k) for lr in self.base_lrs]
        coeff = (1 - (t - self.warmup_iters) / float(self.max_updates - self.warmup_iters)) ** self.power
        return [(lr - self.min_lr) * coeff + self.min_lr for lr in self.base_lrs]


class ValEveryNSteps:
    """helpers/callbacks.py: validation every N steps.  Built from a config's callback list as in the reference; the rule
    itself (`should_validate`, helpers/callbacks.py:19) is what Trainer.fit(val_every_n_steps=) applies, and
    config.trainer_kwargs reads `every_n_steps` out of the YAML for it."""

    def __init__(self, every_n_steps):
        self.every_n_steps = every_n_steps

    def should_validate(self, global_step):
        return bool(self.every_n_steps) and global_step != 0 and global_step % self.every_n_steps == 0


class FlatGradBuffer:
    """All trainable parameters' gradients as views into one contiguous fp32 tensor.

    Limitation (vs. the reference, where a parameter that receives no gradient keeps `.grad = None` and is skipped by the
    optimizer): every view is persistent and zero-filled, so a trainable parameter that is never touched in a step still
    takes its AdamW weight-decay / moment update with a zero gradient.  No module of the hot path has such a parameter
    (every trainable tensor of MiT / DAFormer / SegFormer heads is on all three backward passes); a custom head with an
    unused branch should freeze it (`requires_grad_(False)`).

    `groups`: [(tag, [params])] in the order the gradients become FINAL during a backward pass
    (uda.grad_ready_groups): the buffer is laid out in that order, so `on_ready(tag)` -- called from the backward pass
    itself through seg._GradMark -- can put the range of a finished group on the wire (async all-reduce in `bucket_mb`
    pieces on the RCCL stream) while the backward of the earlier MiT stages is still running.  `all_reduce_mean()`
    reduces whatever has not been released, waits for everything and divides by the world size."""

    ALIGN = 64          # elements: every view starts on a 256-byte boundary (16-byte vector stores in csrc/reduce.hip)

    def __init__(self, params, groups=None, bucket_mb=64):
        self.params = [p for p in params if p.requires_grad]
        order, self.ranges = [], {}
        known = {id(p) for p in self.params}
        pad = lambda k: (k + self.ALIGN - 1) // self.ALIGN * self.ALIGN  # noqa: E731
        off, placed = 0, set()
        for tag, ps in (groups or []):
            start = off
            for p in ps:
                if id(p) in known and id(p) not in placed:
                    order.append(p)
                    placed.add(id(p))
                    off += pad(p.numel())
            if off > start:
                self.ranges[tag] = (start, off)
        rest = [p for p in self.params if id(p) not in placed]
        order += rest
        n = off + sum(pad(p.numel()) for p in rest)
        dev = self.params[0].device
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        off = 0
        for p in order:
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            mark_grad_sink(p)                       # backward kernels may accumulate into this view directly
            off += pad(p.numel())
        self.bucket_mb = bucket_mb
        self._works, self._released = [], []
        self._order, self.flat2 = order, None
        self._comm = self._comm2 = self._stream = None
        self._active = 0                                # which buffer the parameters' .grad views point into right now
        self._in_capture, self.captured_ranges, self._direct_pending = [], (), False
        self.overlapped_elements = 0

    def use_direct(self, comm, stream=None, comm2=None):
        """Reduce over `comm` (refign_amd/rccl.py DirectComm: ncclAllReduce on the stream WE choose) on `stream`, a stream of
        the reduce's own that waits for the producing stream at every release -- instead of torch's process group (whose
        collectives hop to the group's stream and back: 15 ms per step for the six 64 MB buckets of a 1-rank group, measured,
        profiles/r04_ddp_rehearsal.txt).  Event record / wait / ncclAllReduce are all capturable, so the SAME release works
        inside the hipGraph capture of the last backward pass: the all-reduce of the decode head / stage 4 / stage 3 ranges
        becomes a branch of the graph next to the backward of the earlier stages (`end_capture`, `replayed`).
        `comm2`: a second communicator for the SECOND buffer (the mixed pass running next to the source pass accumulates
        there): the sum over ranks is linear, so the two buffers are reduced separately -- the first one whole, as soon as the
        source pass is over and next to the mixed pass (`reduce_first_now`), the second one range by range from inside the
        mixed pass's backward -- and added afterwards.  Twice the bytes on the links, almost all of them hidden; two
        communicators because the two reduces run on unordered streams and one communicator's collectives must be issued in
        the same order on every rank."""
        self._comm, self._stream, self._comm2 = comm, stream, comm2

    def zero(self):
        self.flat.zero_()
        if self.flat2 is not None:
            self.flat2.zero_()
        self._in_capture = []

    def into_second(self):
        """Context manager: inside it every parameter's `.grad` is its view of a SECOND flat buffer.  Used around the
        hipGraph capture of a backward pass that is to run concurrently with another one (the captured kernels keep the
        addresses they saw): two passes accumulating into one buffer from two streams would race on every
        read-modify-write; `merge_second()` adds the second buffer to the first before the optimiser looks."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            if self.flat2 is None:
                self.flat2 = torch.zeros_like(self.flat)
            saved, off = [], 0
            pad = lambda k: (k + self.ALIGN - 1) // self.ALIGN * self.ALIGN  # noqa: E731
            for p in self._order:
                saved.append(p.grad)
                p.grad = self.flat2[off:off + p.numel()].view_as(p)
                off += pad(p.numel())
            self._active = 1
            try:
                yield
            finally:
                self._active = 0
                for p, g_ in zip(self._order, saved):
                    p.grad = g_
        return ctx()

    def merge_second(self):
        if self.flat2 is not None:
            self.flat.add_(self.flat2)

    def _buffer(self, k):
        return self.flat if k == 0 else self.flat2

    def _reduce_range(self, a, b, k=0):
        step = max(1, int(self.bucket_mb * 1024 * 1024 // 4))
        buf = self._buffer(k)
        comm = self._comm if k == 0 else self._comm2
        if comm is not None:
            import contextlib
            on = contextlib.nullcontext()
            if self._stream is not None:
                self._stream.wait_stream(torch.cuda.current_stream(buf.device))           # the gradients queued so far
                on = torch.cuda.stream(self._stream)
            with on:
                for i in range(a, b, step):
                    comm.all_reduce_(buf[i:min(i + step, b)])
            self._direct_pending = True
            return
        for i in range(a, b, step):
            self._works.append(dist.all_reduce(buf[i:min(i + step, b)], op=dist.ReduceOp.SUM, async_op=True))

    def on_ready(self, tag, capturing=None):
        """A group's gradients are final (called from inside the last backward pass into the buffer the views point to)."""
        r = self.ranges.get(tag)
        if r is None or not (dist.is_available() and dist.is_initialized()):
            return
        r = (self._active, *r)
        if r in self._released or r in self._in_capture:
            return
        if capturing is None:
            capturing = self.flat.is_cuda and torch.cuda.is_current_stream_capturing()
        if (self._comm if self._active == 0 else self._comm2) is None and (capturing or self._active == 1):
            # (a collective of torch's process group is not put into a capture here, and the second buffer is only reduced
            # on its own when it has a communicator of its own: the tail takes care of both)
            return
        # (torch's NCCL process group orders an async collective after the work queued so far on the CURRENT stream --
        # inside the autograd engine that is the stream of the backward kernels that produced these gradients)
        (self._in_capture if capturing else self._released).append(r)
        self._reduce_range(r[1], r[2], r[0])

    def reduce_first_now(self):
        """The FIRST buffer is final (the source pass is over; the rest of the step accumulates into the second one): put it on
        the wire whole, behind what is queued on the current stream.  Needs both communicators (see use_direct)."""
        if self._comm is None or self._comm2 is None or not (dist.is_available() and dist.is_initialized()):
            return False
        r = (0, 0, self.flat.numel())
        if r not in self._released:
            self._released.append(r)
            self._reduce_range(0, self.flat.numel(), 0)
        return True

    def end_capture(self):
        """INSIDE the capture, after the backward pass: join the reduce stream; `captured_ranges` <- the ranges the graph
        reduces on every replay (graphs.GraphedStep hands them back to `replayed` after each replay)."""
        if self._in_capture and self._stream is not None:
            torch.cuda.current_stream(self.flat.device).wait_stream(self._stream)
        self.captured_ranges, self._in_capture = tuple(self._in_capture), []
        return self.captured_ranges

    def replayed(self, ranges):
        """A graph that contains the all-reduce of `ranges` has just been replayed in this step."""
        for r in ranges or ():
            if r not in self._released:
                self._released.append(r)

    def _reduce_gaps(self, k):
        pos, n = 0, self.flat.numel()
        for _, a, b in sorted(r for r in self._released if r[0] == k):
            if a > pos:
                self._reduce_range(pos, a, k)
            pos = max(pos, b)
        if pos < n:
            self._reduce_range(pos, n, k)

    def all_reduce_mean(self, bucket_mb=None):
        """Everything the passes have not released, then: wait, add the second buffer, divide by the world size."""
        from .bn import data_parallel
        if not (dist.is_available() and dist.is_initialized()) or not data_parallel():
            # no group, or a group of ONE rank (torchrun --nproc-per-node 1): the sum over one rank is the identity and the
            # mean divides by 1 -- no collective is issued (round 4 sent the 343 MB buffer through six bucketed all-reduces of
            # the 1-rank group anyway: 144.9 -> 159.9 ms/step, the all-reduce kernels of torch's process group running on its
            # own stream next to the three busy compute streams).  RFN_DDP_REHEARSAL=1 makes a 1-rank group exchange for real.
            self.merge_second()
            self._released = []
            return
        if bucket_mb is not None:
            self.bucket_mb = bucket_mb
        world = dist.get_world_size()
        # the second buffer travels on its own as soon as ANY range has been released before this point: adding it into the first
        # buffer here would race with that range's all-reduce in flight -- and would add un-reduced values to reduced ones
        # (the whole-first-buffer and second-buffer releases were the cases round 4 handled)
        separate = self.flat2 is not None and len(self._released) > 0
        if not separate:
            self.merge_second()                       # one sum on the wire: what the second buffer holds goes with the first
        self._reduce_gaps(0)
        if separate:
            self._reduce_gaps(1)
        for w in self._works:
            w.wait()
        if self._direct_pending and self._stream is not None:
            torch.cuda.current_stream(self.flat.device).wait_stream(self._stream)
        self._direct_pending = False
        if separate:
            self.merge_second()
        self.overlapped_elements = sum(b - a for _, a, b in self._released)     # diagnostics / tests
        self.overlapped_fraction = self.overlapped_elements / (self.flat.numel() * (2 if separate else 1))
        self._works, self._released = [], []
        self.flat.div_(world)


class StallGuard:
    """A multi-rank run that makes no progress for `limit` seconds (RFN_STALL_S, default 600; RFN_BENCH_STALL_S is still read) says
    where it stopped on stderr and exits with code 17 instead of hanging the node in a collective.  `note(what)` is the heartbeat:
    Trainer.step calls it around every step; bench.py adds its own phases.  One daemon thread per process.
    `paused(what)`: a context in which the guard does not fire (checkpoint I/O, whose length depends on the disk, not on the
    other ranks); the clock restarts when it ends.  `stop()` ends the thread."""

    def __init__(self, rank, world, limit=None):
        import threading
        import time
        self.rank, self.world = rank, world
        self.limit = float(os.environ.get("RFN_STALL_S", os.environ.get("RFN_BENCH_STALL_S", "600"))) if limit is None else float(limit)
        self.progress = [time.monotonic(), "start"]
        self._paused, self._stop = 0, threading.Event()
        self._thread = threading.Thread(target=self._watch, daemon=True, name="refign-stall-guard")
        self._thread.start()

    def note(self, what):
        import time
        self.progress[0], self.progress[1] = time.monotonic(), what

    def pause(self, what):
        self._paused += 1
        self.note(what)

    def resume(self, what):
        self.note(what)                              # before the count drops: the guard never sees the time spent paused
        self._paused = max(0, self._paused - 1)

    def paused(self, what):
        import contextlib

        @contextlib.contextmanager
        def ctx():
            self.pause(what)
            try:
                yield
            finally:
                self.resume(f"{what} done")
        return ctx()

    def stop(self):
        self._stop.set()

    def _watch(self):
        import sys
        import time
        while not self._stop.wait(min(5.0, max(0.2, self.limit / 4))):
            idle = time.monotonic() - self.progress[0]
            if idle > self.limit and not self._paused:
                print(f"refign_amd rank {self.rank}/{self.world}: no progress for {idle:.0f} s after '{self.progress[1]}'; giving up",
                      file=sys.stderr, flush=True)
                os._exit(17)


# The inputs of the matcher's graphed training step (Trainer(graph_step=True)), in the order the graph takes them.
STEP_GRAPH_INPUTS = ("image_ref", "image_trg", "image_prime", "flow_prime", "mask_prime", "prime_trg_idx")


def prime_idx_tensor(idx, device):
    """`prime_trg_idx` as an int64 tensor on `device`.  A host list goes through pinned memory and a non-blocking copy, as
    AlignmentModel.training_step sends it: no synchronisation (the pinned block is the caching host allocator's, which keeps it
    until the copy has run).  A tensor is moved if it is elsewhere."""
    device = torch.device(device)
    if not torch.is_tensor(idx):
        idx = torch.tensor([int(v) for v in idx], dtype=torch.int64)
        if device.type == "cuda":
            idx = idx.pin_memory()
    return idx.to(device=device, dtype=torch.int64, non_blocking=True)


def step_graph_inputs(batch, device):
    """The tensors of a matcher batch in the order of STEP_GRAPH_INPUTS, `prime_trg_idx` as a device tensor."""
    missing = [k for k in STEP_GRAPH_INPUTS if k not in batch]
    if missing:
        raise KeyError(f"Trainer(graph_step=True): the batch has no {missing}")
    return tuple(prime_idx_tensor(batch[k], device) if k == "prime_trg_idx" else batch[k] for k in STEP_GRAPH_INPUTS)


class Trainer:
    """`step(batch)` = one reference training_step including EMA, three backward passes, the single gradient all-reduce and
    the optimiser/scheduler step (a model with automatic_optimization, the matcher: training_step, one backward pass, optimizer
    and scheduler step -- _automatic_step); `fit` / `validate` / `test` / `predict` = the loops of the Lightning entry points the
    reference is driven through (run.py fit | validate | test | predict); `save_checkpoint` / `load_checkpoint`."""

    def __init__(self, model, sync_batchnorm=False, bucket_mb=64, fused_optimizer=True, gc_interval=None, precision=None,
                 scaler_args=None, ckpt_path=None, deterministic=False, logger=None, log_every_n_steps=50, log_lr=True,
                 graph_step=False, gradient_clip_val=None, gradient_clip_algorithm="norm", accumulate_grad_batches=1):
        """`precision` (the reference's `--trainer.precision`): None -- step() runs under whatever autocast the caller
        entered, no loss scaling (what bench.py does); 16 / '16' / '16-mixed' -- step() enters fp16 autocast itself and
        scales the loss (`self.scaler`, amp.LossScaler; `scaler_args`: its init_scale / growth_factor / backoff_factor /
        growth_interval); 'bf16' / 'bf16-mixed' -- bf16 autocast; 32 -- no autocast.  Anything else: ValueError.
        `ckpt_path` (Lightning's `fit(ckpt_path=...)`): a file of save_checkpoint to continue from (load_checkpoint).
        `deterministic` (Lightning's `--trainer.deterministic true`): bit-reproducible steps -- same build, machine type, seeds
        and batches give the same bits in every loss, parameter, buffer and optimiser state.  Fixed for the life of the trainer
        (refign_amd/determinism.py: on here, off in close(); the kernels that add with floating-point atomics are replaced by
        their store-and-sum forms or refuse) and not available with precision=32.  One process, one GPU.  A model with
        automatic_optimization (the matcher) gets the mode with determinism.scatter_forms() -- its warp backward adds in 64-bit
        fixed point -- at any precision, with graph_step too (eager and replayed runs each repeat themselves, not each other).
        `logger` (a steplog.TensorBoardLogger, or anything with log_metrics(dict, step) / flush() / close(); None: nothing is
        recorded and nothing new runs), `log_every_n_steps`, `log_lr`: the record of the run.  The step that takes
        model.global_step from s to s + 1 is recorded when (s + 1) % log_every_n_steps == 0 and its row is labelled s (rows
        49, 99, ... at the default: this project's definition).  A row holds every entry of model.logged under its own
        name, `grad_norm/<optimizer group>` and `grad_norm/total` of the gradient the optimizer consumed (after the
        all-reduce and, under precision=16, the unscale; a skipped fp16 step shows its infinite or NaN norm),
        `grad_norm/nonfinite_chunks`, under precision=16 `amp/scale`, `amp/found_inf` (both this step's) and
        `amp/skipped_steps` (before this step), and with `log_lr` `lr-<optimizer class>/<optimizer group>` (`lr-AdamW/...`,
        `lr-Adam/...`), the rate this step used.
        The row is put together on the device between the unscale and AdamW (refign_amd/steplog.py) and reaches the host
        through a pinned mirror: the step does not wait for it.  step() hands finished rows to the logger and to
        `log_history`, a list of (step, {name: float}); validate() / test() log their results at the current global_step;
        fit() flushes before each validation, before each checkpoint and at its end, close() flushes and closes the file.
        Several ranks: rank 0 records and writes.  Nothing of the logger goes into a checkpoint.
        `graph_step` (a model with automatic_optimization, the matcher; one rank): training_step, loss scaling and backward
        replay from ONE hipGraph after two eager steps (_automatic_step, graphs.GraphedStep; `step_graph`); zeroing the
        gradients and the optimizer tail stay eager.  The graph is dropped, and captured again after two further eager steps,
        by load_checkpoint, validate / test / predict, model.train() / eval(), model.to() / half() and close().  With
        RFN_HIP_GRAPH=0 or off a GPU the step runs eagerly.  ValueError for a model that steps itself (the UDA model: its passes
        are graphed on their own).
        `gradient_clip_val`, `gradient_clip_algorithm` (Lightning's; None or 0: off): the gradient is clipped in
        _OptimizerProxy.step -- after the all-reduce and, under precision=16, the unscale (Lightning unscales before it clips),
        in front of the logged row and the optimizer -- in place in `self.grads.flat`, so every `p.grad` holds the clipped
        gradient afterwards.  That serves both kinds of model: for one that steps itself (the UDA model: manual optimization)
        it is the place where its training_step would call `self.clip_gradients(...)`.  "norm": clip_grad_norm_ over all
        optimizer parameters together (eps 1e-6, coefficient at most 1; a NaN norm multiplies NaN in, an infinite one gives
        0); "value": clip_grad_value_ (a NaN stays).  Decided and applied on the device (steplog.GradClip); a CPU buffer goes
        through torch's two functions.  Logged rows then hold the norms BEFORE clipping (computed once, shared with the
        clip) and, under "norm", `grad_clip/coef`.
        `accumulate_grad_batches` = k (an int; k > 1 needs a model with automatic_optimization, as in Lightning): step() call
        j = 1 .. k of a window zeroes the gradients for j = 1 only and backpropagates loss / k (divided in front of the loss
        scaling; model.logged keeps the undivided losses); call k alone all-reduces, unscales, clips, steps optimizer and
        scheduler, updates the loss scaler and adds 1 to global_step.  `optimizer_stepped` tells whether the last step() did.
        The window starts anew here and in load_checkpoint; save_checkpoint inside an open window raises.  With graph_step the
        division is part of the graph.  fit() counts optimizer steps."""
        from .amp import parse_precision
        clip_val, clip_alg = parse_gradient_clip(gradient_clip_val, gradient_clip_algorithm)
        self.accumulate_grad_batches = parse_accumulate(accumulate_grad_batches)
        if self.accumulate_grad_batches > 1 and not getattr(model, "automatic_optimization", False):
            raise ValueError("Trainer: accumulate_grad_batches > 1 needs a model with automatic_optimization (the matcher); a "
                             "model that steps itself (the UDA model) decides on its own when its optimizer steps")
        self._clip = None
        if clip_val is not None:
            from .steplog import GradClip
            self._clip = GradClip(clip_val, clip_alg)
        self._micro, self.optimizer_stepped = 0, False       # calls made in the open accumulation window
        self.step_graph = None
        if graph_step and not getattr(model, "automatic_optimization", False):
            raise ValueError("Trainer: graph_step=True is for a model with automatic_optimization (the matcher); the UDA "
                             "model's passes are graphed on their own (graphs.GraphedStep in refign_amd/uda.py)")
        self.log_every_n_steps, self.log_lr = int(log_every_n_steps), bool(log_lr)
        if logger is not None and self.log_every_n_steps < 1:
            raise ValueError("Trainer: log_every_n_steps must be positive")
        if logger is not None and dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
            logger = None                                    # rank 0 records and writes; no collective is involved
        self.logger, self.log_history = logger, []
        self._steplog = self._norm_plan = None
        self.log_stalls, self._eval_logged = 0, set()
        self.precision = parse_precision(precision)
        if scaler_args and self.precision != "16":
            raise ValueError("Trainer: scaler_args needs precision=16")
        self.deterministic = bool(deterministic)
        # a model with automatic_optimization (the matcher) takes the mode with its widening: the order-free warp backward and the
        # gather form of the generic correlation backward (determinism.scatter_forms).  It has no attention: any precision.
        self._det_scatter = self.deterministic and bool(getattr(model, "automatic_optimization", False))
        if self.deterministic and self.precision == "32" and not self._det_scatter:
            raise ValueError("Trainer: deterministic=True is not available with precision=32 (the fp32 parity attention adds its "
                             "dK / dV chunks with atomics)")
        self._det_held = False
        self.model = model
        if gc_interval is None:
            gc_interval = int(os.environ.get("RFN_GC_INTERVAL", "100"))
        self.gc_interval, self._steps_done = gc_interval, 0
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        from .bn import data_parallel
        self.data_parallel = data_parallel()                 # world > 1, or a 1-rank rehearsal of it
        from .bn import ddp_mode
        self.ddp_mode = ddp_mode() if self.data_parallel else None
        if sync_batchnorm and dist.is_available() and dist.is_initialized():
            nn.SyncBatchNorm.convert_sync_batchnorm(model)   # student AND teacher BNs (reference: sync_batchnorm: True)
            # The EMA teacher runs on a side stream next to the student (and next to hipGraph replays that contain the
            # student's statistics exchanges): its BatchNorm collectives get a communicator of their own, so that the
            # two streams never interleave collectives of ONE communicator in a rank-dependent order.
            teacher = [m for n, mod in model.named_children() if n.startswith("m_") for m in mod.modules()
                       if isinstance(m, nn.SyncBatchNorm)]
            if teacher and self.data_parallel:
                group = dist.new_group()
                for m in teacher:
                    m.process_group = group
        # RCCL called directly for the statistics exchanges (refign_amd/rccl.py; RFN_DDP_MODE=direct / direct3): a collective of torch's
        # process group hops to the group's own stream and back, and with three compute streams on four hardware queues
        # that stream shares a queue with a busy one -- in the 1-rank rehearsal the teacher branch takes 138 ms instead
        # of 116.  One communicator per stream that exchanges: the student's passes on the main stream, the teacher
        # (side stream), and -- with graphed student passes -- the mixed pass, which may then run next to the source
        # pass as it does on one GPU.
        from . import bn as _bn
        _bn._DIRECT["default"] = None
        if sync_batchnorm and self.data_parallel and next(model.parameters()).is_cuda and dist.get_backend() == "nccl":
            from . import rccl
            if rccl.enabled():
                dev = next(model.parameters()).device
                try:
                    _bn._DIRECT["default"] = rccl.DirectComm(dev)
                    if teacher:
                        teacher_comm = rccl.DirectComm(dev)
                        for m in teacher:
                            m._rfn_direct = teacher_comm
                    # A THIRD communicator (RFN_DDP_MODE=direct3 only): the mixed pass on its own stream next to the source pass, as
                    # on one GPU.  Every communicator's collectives are issued from one host thread in program order on a stream
                    # of its own, the same on every rank -- but three communicators' kernels on one device have never met a
                    # second rank (bn.ddp_mode), so this is opt-in.
                    if _bn.ddp_mode() == "direct3":
                        model._mixed_comm = rccl.DirectComm(dev)
                    # The gradient reduce.  Default: torch's process group, bucketed, after the passes (with the mixed pass
                    # next to the source pass there is no cheap way to start earlier: releases from inside a captured pass are
                    # cross-stream branches of its graph, and two graphs replaying side by side pay ~25 ms for those --
                    # profiles/r04_ddp_rehearsal.txt; the reduce itself is 343 MB: ~1-5 ms of link time on 8..2 GPUs).
                    # RFN_DDP_DIRECT_REDUCE=1: a communicator and a stream of its own (FlatGradBuffer.use_direct) -- the
                    # finished ranges then travel from inside the last backward pass, eagerly and inside the captured mixed
                    # pass alike (meant for RFN_DDP_MODE=direct: passes in stream order).
                    if os.environ.get("RFN_DDP_DIRECT_REDUCE", "0") == "1":
                        self._grad_comm = rccl.DirectComm(dev)
                        # (second buffer reduced on its own -- FlatGradBuffer.use_direct -- only on request: its in-graph
                        # releases are cross-stream branches of the mixed pass's graph, and two graphs replaying next to each
                        # other pay ~25 ms for those in the rehearsal: 172.7 against 147-159 ms with one reduce at the tail)
                        self._grad_comm2 = rccl.DirectComm(dev) if getattr(model, "_mixed_comm", None) is not None and \
                            os.environ.get("RFN_DDP_TWO_BUFFER", "0") == "1" else None
                except (OSError, RuntimeError, AttributeError) as e:   # no librccl / init failed: torch's process group
                    import warnings
                    warnings.warn(f"refign_amd.trainer: direct RCCL communicators unavailable ({type(e).__name__}: {e}); "
                                  f"statistics exchanges go through torch.distributed, student passes run eagerly")
                    _bn._DIRECT["default"] = None
                    for m in teacher:
                        m.__dict__.pop("_rfn_direct", None)
                    model.__dict__.pop("_mixed_comm", None)
                    self._grad_comm = self._grad_comm2 = None
        if fused_optimizer and model.optimizer_init["class_path"].endswith("AdamW") and \
                next(model.parameters()).is_cuda:
            model.optimizer_init = {**model.optimizer_init,
                                    "init_args": {**model.optimizer_init["init_args"], "fused": True}}
        (opt,), (sch,) = model.configure_optimizers()
        if isinstance(sch, dict):                            # Lightning's {'scheduler': ..., 'interval': 'step'} (AlignmentModel)
            if sch.get("interval", "step") != "step":
                raise ValueError(f"Trainer: lr scheduler interval {sch.get('interval')!r}: this trainer counts steps only")
            sch = sch["scheduler"]
        self.optimizer, self.scheduler = opt, sch
        self.fast_step = None
        if fused_optimizer and next(model.parameters()).is_cuda:
            from .optim import MultiTensorAdam, MultiTensorAdamW
            if type(opt) is torch.optim.AdamW:
                self.fast_step = MultiTensorAdamW(opt)        # one launch per step; torch's step() where it declines
            elif type(opt) is torch.optim.Adam:
                self.fast_step = MultiTensorAdam(opt)         # (the matcher's configs; the optimizer's arguments stay as given)
        groups = model.grad_ready_groups() if hasattr(model, "grad_ready_groups") else None
        self.grads = FlatGradBuffer([p for g in opt.param_groups for p in g["params"]], groups, bucket_mb)
        if getattr(self, "_grad_comm", None) is not None:
            self.grads.use_direct(self._grad_comm, torch.cuda.Stream(device=self._grad_comm.device),
                                  getattr(self, "_grad_comm2", None))
        self.bucket_mb = bucket_mb
        model._optimizer = _OptimizerProxy(self)
        model._grad_buffer = self.grads                      # uda: second buffer for the concurrently running mixed pass
        model._scheduler = sch
        model._backward = self._backward
        if graph_step:
            from .graphs import GraphedStep
            self._graph_logged = ()
            self.step_graph = GraphedStep(self._graphed_pass, "matcher training step", before_capture=self._before_capture)
            model.__dict__["_step_graph"] = self.step_graph   # AlignmentModel drops it with its own graphs (train / _apply / load)
        self.scaler = None
        if self.precision == "16":
            from .amp import LossScaler
            self.scaler = LossScaler(self.grads.flat.device, **(scaler_args or {}))
        self.guard = None
        if dist.is_available() and dist.is_initialized():
            self.broadcast_parameters()
            if dist.get_world_size() > 1:                    # a rank that never arrives must not hang the others for ever
                self.guard = StallGuard(dist.get_rank(), dist.get_world_size())
        # the last act before anything launches a kernel that has two forms: a constructor that raised further up holds nothing
        if self.deterministic:
            from . import determinism
            determinism.acquire(scatter_forms=self._det_scatter)
            self._det_held = True
        if ckpt_path is not None:
            self.load_checkpoint(ckpt_path)

    def _backward(self, loss, retain_graph=False, last=False):
        """What Lightning's manual_backward does, plus: during the LAST backward pass of a step under data parallelism
        the readiness marks of the MiT stages release finished ranges of the flat gradient buffer to the all-reduce."""
        from . import seg
        # (inside a hipGraph capture of the pass too when the buffer has a communicator of its own -- FlatGradBuffer.use_direct;
        # on_ready declines otherwise and the replayed pass is followed by one reduce of the whole buffer)
        capturing = loss.is_cuda and torch.cuda.is_current_stream_capturing()
        overlap = last and self.data_parallel and os.environ.get("RFN_DDP_OVERLAP", "1") != "0"
        seg._GRAD_READY_CB = self.grads.on_ready if overlap else None
        if self.scaler is not None:
            loss = self.scaler.scale(loss)
        from . import mfma
        try:
            with mfma.deferred_wgrads():                 # Linear weight gradients: queued, launched per block in groups
                loss.backward(retain_graph=retain_graph)
            if capturing and overlap:
                self.grads.end_capture()
        finally:
            seg._GRAD_READY_CB = None

    def broadcast_parameters(self):
        for t in list(self.model.parameters()) + list(self.model.buffers()):
            dist.broadcast(t.data, src=0)

    def step(self, batch, batch_idx=0, next_batch=None):
        """`next_batch` (optional): the batch of the following step, already on the device -- lets the model compute
        what depends on its inputs only (the frozen ImageNet encoder's features of the next source images) while this
        step's mixed pass runs (uda.prefetch_imnet_features)."""
        if self._steplog is not None:
            self._hand_over(self._steplog.poll())            # rows whose events have completed: no waiting
        if next_batch is not None and not getattr(self.model, "automatic_optimization", False):
            batch = dict(batch, image_src_next=next_batch["image_src"], semantic_src_next=next_batch.get("semantic_src"),
                         image_trg_next=next_batch.get("image_trg"), image_ref_next=next_batch.get("image_ref"))
        # Python's cyclic collector fires on allocation counts; a step allocates ~10^5 autograd / tensor wrapper objects
        # and a generation-2 pass in the middle of a step stalls the launch thread for ~100 ms (seen as one slow step in
        # ten).  Collect at a step boundary every `gc_interval` steps instead, with the automatic collector off.
        if self.gc_interval:
            import gc
            if self._steps_done == 0:
                gc.collect()
                gc.disable()
            elif self._steps_done % self.gc_interval == 0:
                gc.collect()
            self._steps_done += 1
        if self.guard is not None:
            self.guard.note(f"entering step {self._steps_done}")
        try:
            # (the step's main-stream work on a stream of its own / of another priority: neutral, profiles/r05_main_priority_ab.txt --
            # HIP offers two priority levels here, (0, -1), and the teacher's stream already has the high one)
            from . import determinism
            if getattr(self.model, "automatic_optimization", False):
                with determinism.torch_deterministic(self.deterministic):
                    self._automatic_step(batch, batch_idx)
            else:
                with determinism.torch_deterministic(self.deterministic), self._autocast():
                    self.model.training_step(batch, batch_idx)
                self.optimizer_stepped = True
            if self.guard is not None:
                self.guard.note(f"step {self._steps_done} queued")
        finally:
            # a crop pre-drawn for a forward that did not happen (exception, mode mismatch) must not leak into the next
            # unrelated extract_crop call
            from . import seg
            seg._PREDRAWN_CROPS.clear()
            seg._DEVICE_CROPS.clear()
        return {k: (float(v) if torch.is_tensor(v) else v) for k, v in self.model.logged.items()} \
            if os.environ.get("RFN_LOG_LOSSES") else None

    def _automatic_step(self, batch, batch_idx):
        """A model with automatic_optimization (AlignmentModel): training_step returns the loss and this trainer does what
        Lightning does around it -- zero the gradients, backward (scaled under precision=16), optimizer step through the
        proxy (all-reduce, unscale, clip, step-log row, Adam, scaler update), scheduler step, global_step + 1.  With
        accumulate_grad_batches = k the head (zeroing) belongs to the first call of a window and the tail (from the proxy on)
        to its last one, and every call backpropagates loss / k (Lightning's closure_loss / accumulate_grad_batches).  The
        gradient stays readable in `self.grads` until the next window.  Nothing here asks the host about device data after
        the first call of a shape: the head's warps skip their zero-flow check (matching.no_zero_flow_check)."""
        from . import matching
        model = self.model
        closes = self._closes_window()
        if self._micro == 0:
            self.grads.zero()
        if self.step_graph is not None:
            # training_step + loss scaling + backward as one replay; the outputs are copies the next replay does not touch, so
            # the step log (which reads model.logged later in stream order) and the caller see this step's values
            self._graph_batch_idx = batch_idx
            out = self.step_graph(*step_graph_inputs(batch, self.grads.flat.device))
            model.logged.update(zip(self._graph_logged, out))
        else:
            with self._autocast(), matching.no_zero_flow_check():
                loss = model.training_step(batch, batch_idx)
            self._backward(self._window_share(loss), last=closes)
        self._micro = 0 if closes else self._micro + 1
        self.optimizer_stepped = closes
        if not closes:
            return
        model._optimizer.step()
        self.scheduler.step()
        model.global_step += 1

    def _closes_window(self):
        """Whether the next step() call is the last of its accumulation window (always, without accumulation)."""
        return self._micro == self.accumulate_grad_batches - 1

    def _window_share(self, loss):
        k = self.accumulate_grad_batches
        return loss / k if k > 1 else loss

    def _graphed_pass(self, *tensors):
        """What `step_graph` runs eagerly, captures and replays: the eager branch of _automatic_step on the tensors of
        STEP_GRAPH_INPUTS (`prime_trg_idx` always a device tensor here: no pinned temporary inside a capture) -> the scalar
        tensors training_step logged, in the order it logged them (`_graph_logged`: their names).  One graph serves every call
        of an accumulation window (the division by k is in it), so under data parallelism no call releases ranges to the
        all-reduce from inside its backward: the window's last call reduces in the optimizer tail."""
        from . import matching
        model = self.model
        before = dict(model.logged)
        with self._autocast(), matching.no_zero_flow_check():
            loss = model.training_step(dict(zip(STEP_GRAPH_INPUTS, tensors)), self._graph_batch_idx)
        self._backward(self._window_share(loss), last=self.accumulate_grad_batches == 1)
        names = tuple(k for k, v in model.logged.items() if torch.is_tensor(v) and v is not before.get(k))
        self._graph_logged = names
        return tuple(model.logged[k] for k in names)

    def _before_capture(self):
        """The blocks the eager warm-up steps left in the caching allocator go back to the device before the step is captured
        into a pool of its own (the same activations a second time otherwise)."""
        torch.cuda.empty_cache()

    # -- the record of the run -----------------------------------------------------------------------------------------
    def _record_row(self):
        """Called by _OptimizerProxy.step between the unscale and AdamW: the losses are in model.logged and the current stream
        has joined the streams that made them, the gradients are final, the scaler has not been updated, and
        model.global_step is still the label of this step."""
        if not self._row_due():
            return
        label = int(self.model.global_step)
        from . import steplog
        flat = self.grads.flat
        if flat.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("Trainer: the optimizer step is being captured into a graph; a logged row (copy to the host mirror, "
                               "event record) cannot be part of a capture")
        groups = self.optimizer.param_groups
        gnames = [str(g.get("name", i)) for i, g in enumerate(groups)]
        scalars, host = {}, {}
        for k, v in self.model.logged.items():
            if k in self._eval_logged:                       # left there by validate() / test(), which log their own rows
                continue
            if torch.is_tensor(v):
                if v.numel() != 1:
                    continue                                 # (a row holds scalars)
                if v.device != flat.device:
                    raise TypeError(f"Trainer: model.logged[{k!r}] is on {v.device}, the step runs on {flat.device}")
                scalars[k] = v if v.dtype in steplog.DTYPE_CODES else v.double()
            else:
                host[k] = float(v)
        if self.scaler is not None:
            scalars.update({"amp/scale": self.scaler._scale, "amp/found_inf": self.scaler.found_inf,
                            "amp/skipped_steps": self.scaler._skipped})
        if self.log_lr:
            host.update({f"lr-{type(self.optimizer).__name__}/{n}": float(g["lr"]) for n, g in zip(gnames, groups)})
        clip = self._clip
        if clip is not None and clip.algorithm == "norm":
            scalars["grad_clip/coef"] = clip.coef[:1]
        log = self._steplog
        if log is None or log.names != list(scalars):
            if log is not None:                              # another set of logged names (a model stepped by hand): a new ring
                self._hand_over(log.flush())
                self.log_stalls += log.stalls
            log = self._steplog = steplog.StepLog(flat.device, list(scalars), group_names=gnames)
        if clip is not None:                                 # the norms the clip took before it changed the gradient
            log.record(label, scalars, sqnorms=clip.sqnorms, host=host)
        else:
            log.record(label, scalars, grads=(flat, self._grad_norm_plan()), host=host)

    def _row_due(self):
        """Whether the optimizer step in progress is one whose row is recorded."""
        return self.logger is not None and (int(self.model.global_step) + 1) % self.log_every_n_steps == 0

    def _grad_norm_plan(self):
        if self._norm_plan is None:
            from .steplog import GradNormPlan
            self._norm_plan = GradNormPlan.for_buffer(self.grads, self.optimizer.param_groups)
        return self._norm_plan

    def _unscale_and_clip(self):
        """Called by _OptimizerProxy.step after the all-reduce: the loss scaler's unscale (precision=16), then the clip."""
        if self._clip is not None:
            self._clip(self.grads, self._grad_norm_plan(), self.scaler, want_norms=self._row_due())
        elif self.scaler is not None:
            self.scaler.unscale_(self.grads.flat)

    def _hand_over(self, rows):
        for step, row in rows:
            self.log_history.append((step, row))
            self.logger.log_metrics(row, step)

    def _log_results(self, results):
        """validate / test results as scalars at the current global_step; a per-class list becomes <name>/<class index>."""
        if self.logger is None or not results:
            return
        row = {}
        for k, v in results.items():
            if isinstance(v, (list, tuple)):
                row.update({f"{k}/{i}": float(x) for i, x in enumerate(v)})
            else:
                row[k] = float(v)
        self.flush_log()
        self._hand_over([(int(self.model.global_step), row)])

    def flush_log(self):
        """Every recorded row to the logger and to log_history (waits for the rows' events, not for the device), and the
        logger's file flushed.  Returns the number of times record() had to wait for a free row so far."""
        if self.logger is None:
            return 0
        if self._steplog is not None:
            self._hand_over(self._steplog.flush())
        self.logger.flush()
        return self.log_stalls + (self._steplog.stalls if self._steplog is not None else 0)

    # -- loops ---------------------------------------------------------------------------------------------------------
    def _autocast(self):
        """The autocast of this trainer's `precision` for step() and the evaluation loops (None: whatever the caller entered)."""
        import contextlib
        if self.precision is None:
            return contextlib.nullcontext()
        dtype = {"16": torch.float16, "bf16": torch.bfloat16, "32": None}[self.precision]
        return torch.autocast("cuda", dtype=dtype or torch.float32, enabled=dtype is not None)

    @staticmethod
    def _named(loaders):
        """{dataset name: iterable} in the order of the reference's datamodule.idx_to_name[split], or one bare iterable ("")."""
        from collections.abc import Mapping
        return list(loaders.items()) if isinstance(loaders, Mapping) else [("", loaders)]

    def _to_device(self, batch):
        dev = self.grads.flat.device
        moved = {k: v.to(dev, non_blocking=True) for k, v in batch.items() if torch.is_tensor(v) and v.device != dev}
        return dict(batch, **moved) if moved else batch

    def _evaluation(self, what, loaders, per_batch, at_end=None, metrics=None):
        """The frame of validate / test / predict: model in eval(), no_grad, this trainer's autocast, `per_batch(batch,
        batch_idx, dataloader_idx, name)` over every loader, `at_end()` once; then every module back in the mode it was in
        (through model.train(), which drops captured graphs and mode-dependent caches: the student passes are captured again
        on the next steps) and what the last step prefetched for its successor dropped (made under the graphs of before; the
        next step computes it itself, the numbers are the same).  If a batch raises, the metrics are reset."""
        model = self.model
        modes = [(m, m.training) for m in model.modules()]
        model.eval()
        try:
            with torch.no_grad():
                with self._autocast():
                    for idx, (name, loader) in enumerate(self._named(loaders)):
                        for i, batch in enumerate(loader):
                            if self.guard is not None:
                                self.guard.note(f"{what}: dataset {idx} '{name}' batch {i}")
                            per_batch(self._to_device(batch), i, idx, name)
                out = at_end() if at_end is not None else None
            return out
        except BaseException:
            if metrics is not None:
                metrics.reset()
            raise
        finally:
            model.train(modes[0][1])
            for m, mode in modes:
                m.training = mode
            for k in ("_imnet_prefetch", "_class_prefetch", "_align_prefetch"):
                if k in model.__dict__:
                    model.__dict__[k] = None
            if self.guard is not None:
                self.guard.note(f"{what} done")

    def _metric_loop(self, split, loaders):
        from . import evaltail
        model = self.model
        metrics = getattr(model, "valid_metrics" if split == "validation" else "test_metrics", None)
        step, end = getattr(model, f"{split}_step"), getattr(model, f"{split}_epoch_end")

        def per_batch(batch, i, idx, name):
            if metrics is None or not evaltail.eval_step(model, metrics, batch, name):
                step(batch, i, idx, src_name=name)

        before = dict(model.logged) if self.logger is not None and hasattr(model, "logged") else None
        out = self._evaluation(split, loaders, per_batch, end, metrics)
        if before is not None:                               # what the epoch end logged is no part of a training step's row
            self._eval_logged |= {k for k, v in model.logged.items() if k not in before or before[k] is not v}
        out = {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in (out or {}).items()}
        self._log_results(out)
        return out

    def validate(self, loaders):
        """Lightning's `validate`: every batch of every loader through the model's validation step, then
        validation_epoch_end once -> {metric name: float, or list for per-class metrics}.  `loaders`: {dataset name: iterable
        of batches} in the order of the reference's datamodule.idx_to_name['val'] (the name is validation_step's `src_name`,
        the position its `dataloader_idx`), or one bare iterable (name "").  A batch is the reference's dict (`image`,
        `semantic`, ...); host tensors are moved to the model's device.  Runs in eval mode under no_grad and the autocast of
        this trainer's `precision`, and leaves every module in the mode it was in: nothing a later step() reads changes
        (parameters, EMA, BatchNorm statistics, optimizer, RNG streams).  A segmentation batch goes through the fused
        evaluation tail (refign_amd/evaltail.py: one kernel from the crop logits to the confusion counts) when its conditions
        hold -- evaltail.eval_step lists them; RFN_EVAL_FUSED=0 turns it off -- and through model.validation_step otherwise
        (any model with validation_step / validation_epoch_end works, AlignmentModel included).
        Multi-rank: each rank iterates its own loaders, of any length; the only collectives are the ones the metrics'
        compute() issues at the end, once per metric, so every rank must call validate() the same number of times."""
        return self._metric_loop("validation", loaders)

    def test(self, loaders):
        """Lightning's `test`: as validate(), through test_step / test_epoch_end and the model's test metrics."""
        return self._metric_loop("test", loaders)

    def predict(self, loaders, save_dir, orig_size=None, fused_resize=False):
        """Lightning's `predict`: arg-max label maps of every batch (`image`, `filename`) as PNGs under
        `<save_dir>/preds/<dataset>/<filename>` and `<save_dir>/color_preds/<dataset>/<filename>` (segmentation_model.py:
        283-302; no sub-directory for a bare iterable).  `orig_size`: the size the predictions are interpolated to (the
        reference's datamodule.predict_ds[i].orig_dims); None: the image size.  An `orig_size` other than the image size goes
        through model.predict_step, or with `fused_resize` through the fused evaluation tail as well (evaltail.labels_resized:
        the interpolation to `orig_size` inside the kernel; under 16-bit autocast it keeps fp32 where predict_step rounds its
        intermediate logits).  -> the number of files written."""
        from . import evaltail
        model, written = self.model, [0]

        def per_batch(batch, i, idx, name):
            preds = evaltail.predict_step(model, batch, save_dir, orig_size, name or None, resize=fused_resize)
            if preds is None:
                preds = model.predict_step(batch, i, idx, save_dir=save_dir, orig_size=orig_size, dataset_name=name or None)
            written[0] += 2 * len(preds) if save_dir is not None else 0

        self._evaluation("predict", loaders, per_batch)
        return written[0]

    def fit(self, train_batches, val_loaders=None, max_steps=None, val_every_n_steps=None, ckpt_dir=None, save_last=True):
        """Lightning's `fit`: step() until model.global_step == max_steps -- after `ckpt_path=` / load_checkpoint the run
        continues from the restored step count, it does not start over.  `train_batches` is iterated again when it is
        exhausted; WHERE in it a resumed run continues is the caller's to restore (hand in an iterable that starts at the
        batch the saved run would have taken next): the checkpoint holds no loader state.  The loop looks one batch ahead and
        hands it to step(..., next_batch=), which prefetches what depends on the next inputs only; the last step gets None.
        With accumulate_grad_batches = k, max_steps and val_every_n_steps count optimizer steps (k calls of step() each),
        step()'s batch_idx counts calls, and only the very last call gets None.
        After every step whose new global_step is a non-zero multiple of `val_every_n_steps` (helpers/callbacks.py:19) it
        runs validate(val_loaders); with `ckpt_dir` and `save_last` it writes `<ckpt_dir>/last.ckpt` (save_checkpoint) after
        each validation and at the end (ModelCheckpoint(save_last=True)).  max_steps=None: the scheduler's max_steps.
        -> [(global_step, metrics dict)], one entry per validation run."""
        model = self.model
        if max_steps is None:
            max_steps = getattr(self.scheduler, "max_updates", None)
        if max_steps is None:
            raise ValueError("Trainer.fit: max_steps is not given and the scheduler has none")
        rule = ValEveryNSteps(val_every_n_steps if val_loaders is not None else None)
        last = os.path.join(ckpt_dir, "last.ckpt") if ckpt_dir is not None and save_last else None
        history, saved_at = [], None
        if int(model.global_step) >= max_steps:
            return history

        def batches():
            while True:
                n = 0
                for b in train_batches:
                    n += 1
                    yield b
                if n == 0:
                    raise ValueError("Trainer.fit: train_batches is empty")

        it = batches()
        batch = self._to_device(next(it))
        while int(model.global_step) < max_steps:
            start = int(model.global_step)
            closes = self._closes_window()
            nxt = self._to_device(next(it)) if start + 1 < max_steps or not closes else None
            self.step(batch, start * self.accumulate_grad_batches + self._micro, next_batch=nxt)
            batch = nxt
            if not closes:
                continue                                     # inside a window: nothing has advanced, nothing is due
            if int(model.global_step) <= start:
                raise RuntimeError("Trainer.fit: the model's training_step did not advance global_step")
            if rule.should_validate(int(model.global_step)):
                self.flush_log()
                history.append((int(model.global_step), self.validate(val_loaders)))
                if last is not None:
                    self.flush_log()
                    self.save_checkpoint(last)
                    saved_at = int(model.global_step)
        if last is not None and saved_at != int(model.global_step):
            self.flush_log()
            self.save_checkpoint(last)
        self.flush_log()
        return history

    # -- checkpoints ---------------------------------------------------------------------------------------------------
    def _io(self, what):
        """Checkpoint I/O runs outside step(): the stall guard must not take a slow disk for a lost rank."""
        import contextlib
        return self.guard.paused(what) if self.guard is not None else contextlib.nullcontext()

    def save_checkpoint(self, filepath, weights_only=False):
        """Write the run's state to `filepath` in the dict layout of PyTorch-Lightning 1.5.10 (the reference's version):
        `epoch` (0: this trainer counts steps only), `global_step` (model.global_step, the steps done),
        `pytorch-lightning_version`, `state_dict` (model.state_dict(): the reference's key names), `loops` (the step count,
        for the layout's sake; not read back), `callbacks` ({}), `optimizer_states` ([the torch AdamW's state_dict()], step
        counts brought up from the device first), `lr_schedulers` ([scheduler.state_dict()]) and, under precision=16,
        `native_amp_scaling_state` (LossScaler.state_dict(), GradScaler's format).  What that layout has no slot for goes
        under `refign_amd`: every rank's RNG states (python `random`, numpy, torch CPU, the rank's device generator),
        the world size, the precision and the scaler's skipped-step count.  Whether Lightning itself resumes from this
        file is not tested (it is not a dependency); what is tested is the layout and that `state_dict` is what the
        reference's strict loader takes.
        `weights_only=True`: only epoch / global_step / version / state_dict (loads through `pretrained=` / load_weights).
        Call between steps, on every rank: the ranks' RNG states are gathered to rank 0, which alone writes -- to a
        temporary file in the same directory, moved into place when complete, so a save that fails part-way leaves the
        previous file as it was -- and every rank returns once the file is in place (an error on rank 0 raises on all).
        Not exact under precision=32 (parity mode): see DESIGN.md, Checkpoints.  RuntimeError inside an open accumulation
        window (accumulate_grad_batches > 1): neither this file nor Lightning's keeps a partial gradient."""
        if self._micro:
            raise RuntimeError(f"Trainer.save_checkpoint: {self._micro} of {self.accumulate_grad_batches} calls of an accumulation "
                               f"window are done; the file has no place for a partial gradient -- save after the window's last call")
        dist_on = dist.is_available() and dist.is_initialized()
        rank = dist.get_rank() if dist_on else 0
        dev = self.grads.flat.device
        with self._io(f"save_checkpoint {filepath}"):
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)           # everything the last step queued is in the tensors written below
            ckpt = {"epoch": 0, "global_step": int(self.model.global_step), "pytorch-lightning_version": LIGHTNING_VERSION,
                    "state_dict": self.model.state_dict()}
            if not weights_only:
                rng = [_rng_state(dev)]
                if dist_on:
                    rng = [None] * dist.get_world_size()
                    dist.all_gather_object(rng, _rng_state(dev))
                gs = ckpt["global_step"]
                progress = {"ready": gs, "started": gs, "processed": gs, "completed": gs}
                ckpt["loops"] = {"fit_loop": {"epoch_loop.batch_progress": {"total": dict(progress), "current": dict(progress)}}}
                ckpt["callbacks"] = {}
                ckpt["optimizer_states"] = [self.optimizer.state_dict()]   # (MultiTensorAdamW's pre-hook syncs `step`)
                ckpt["lr_schedulers"] = [self.scheduler.state_dict()]
                if self.scaler is not None:
                    ckpt["native_amp_scaling_state"] = self.scaler.state_dict()
                ckpt[_OWN_KEY] = {"world_size": len(rng), "precision": self.precision, "rng": rng,
                                  "scaler_skipped": self.scaler.skipped_steps() if self.scaler is not None else 0}
            err = None
            if rank == 0:
                try:
                    _atomic_save(ckpt, filepath)
                except Exception as e:
                    if not dist_on:
                        raise
                    err = e
            if dist_on:
                box = [None if err is None else f"{type(err).__name__}: {err}"]
                dist.broadcast_object_list(box, src=0)        # the others wait here until the file is in place
                if err is not None:
                    raise err
                if box[0] is not None:
                    raise RuntimeError(f"Trainer.save_checkpoint: rank 0 could not write {filepath}: {box[0]}")

    def load_checkpoint(self, filepath):
        """Continue the run saved in `filepath` (save_checkpoint, or a Lightning file of the reference): the next step()
        is the one the saved run would have taken next.  Model: state_dict loaded strictly, global_step restored, every
        cached copy of a parameter (16-bit / transposed copies, fp8 teacher weights) re-made from the loaded values, captured
        graphs, folded BatchNorm weights and packed frozen weights dropped (they are re-made on use).  Optimizer: the torch
        AdamW's state (the running trainer keeps its own implementation flags: fused / foreach / capturable); the fused step
        rebuilds its chunk table from it.  Scheduler, and the loss scaler under precision=16 (a file without a scaler state:
        fresh scaler, warning; a scaler state into a trainer without loss scaling: ignored, warning).  RNG: this rank's
        saved states; a file without them or written by another world size (a reference Lightning file) seeds rank r from
        (global_step, r) instead, with a warning -- the random draws then differ from the uninterrupted run's.
        Every rank calls it; each reads the file itself."""
        import warnings
        dist_on = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if dist_on else (0, 1)
        dev = self.grads.flat.device
        model = self.model
        self._micro = 0                                      # an accumulation window starts with the next step()
        with self._io(f"load_checkpoint {filepath}"):
            # (full pickle, as Lightning 1.5 loads: a reference file carries its hyper-parameters as python objects)
            ckpt = torch.load(filepath, map_location="cpu", weights_only=False)
            if "optimizer_states" not in ckpt or "lr_schedulers" not in ckpt:
                raise KeyError(f"Trainer.load_checkpoint: {filepath} holds the model only (save_checkpoint(weights_only=True)); "
                               f"load it through the model's `pretrained=` / load_weights to start a new run from it")
            model.load_state_dict(ckpt["state_dict"], strict=True)      # (uda: drops the captured graphs)
            model.global_step = int(ckpt.get("global_step", 0))
            for k in ("_imnet_prefetch", "_class_prefetch", "_align_prefetch"):   # made for a batch of the run before
                if k in model.__dict__:
                    model.__dict__[k] = None
            from .params import refresh
            refresh(model.parameters())               # cached 16-bit copies re-filled from the loaded values, others dropped
            if getattr(model, "teacher_f8", False):
                from . import f8
                f8.requantize()                       # K5: e4m3 teacher weights from the re-filled bf16 copies
            self._load_optimizer_state(ckpt["optimizer_states"][0])
            self.scheduler.load_state_dict(ckpt["lr_schedulers"][0])
            own = ckpt.get(_OWN_KEY) or {}
            amp = ckpt.get("native_amp_scaling_state")
            if self.scaler is not None:
                if amp:
                    self.scaler.load_state_dict(amp)
                    self.scaler._skipped.fill_(float(own.get("scaler_skipped", 0)))
                else:
                    warnings.warn(f"Trainer.load_checkpoint: {filepath} holds no loss-scaler state; the fp16 loss scaler "
                                  f"starts fresh")
            elif amp:
                warnings.warn(f"Trainer.load_checkpoint: {filepath} holds a loss-scaler state, this trainer does not scale "
                              f"(precision={self.precision}); ignored")
            rng = own.get("rng")
            if rng and int(own.get("world_size", -1)) == world and len(rng) == world:
                _set_rng_state(rng[rank], dev)
            else:
                why = "no RNG states" if not rng else f"RNG states of {own.get('world_size')} ranks, this run has {world}"
                warnings.warn(f"Trainer.load_checkpoint: {filepath} has {why}; rank {rank} is seeded from (global_step, rank) "
                              f"-- the resumed run's random draws differ from the uninterrupted run's")
                _seed_rank(model.global_step, rank)

    def _load_optimizer_state(self, state):
        """torch's Optimizer.load_state_dict with the param groups checked by name and the running optimizer's
        implementation flags kept (a file from a fused_optimizer=False trainer loads into a fused one and back; the `step`
        tensors then sit where these flags want them)."""
        mine = self.optimizer.param_groups
        names = [g.get("name") for g in state["param_groups"]]
        if names != [g.get("name") for g in mine]:
            raise ValueError(f"Trainer.load_checkpoint: optimizer param groups {names} != this model's "
                             f"{[g.get('name') for g in mine]}")
        state = dict(state, param_groups=[{**g, **{k: cur[k] for k in _IMPL_FLAGS if k in cur}}
                                          for g, cur in zip(state["param_groups"], mine)])
        self.optimizer.load_state_dict(state)         # (MultiTensorAdamW's post-hook drops its chunk table and device step)

    def close(self):
        """Give the process its cyclic garbage collector back (step() runs with it disabled between its own collections)
        and stop the stall guard; with a logger: hand over every recorded row and close its file; with graph_step: release
        the step's graph and its memory pool."""
        if getattr(self, "step_graph", None) is not None:
            self.step_graph.reset()
        if getattr(self, "logger", None) is not None:
            try:
                self.flush_log()
            finally:
                self.logger.close()
                self.logger = None
        if getattr(self, "guard", None) is not None:
            self.guard.stop()
            self.guard = None
        if getattr(self, "gc_interval", 0) and getattr(self, "_steps_done", 0):
            import gc
            gc.enable()
        if getattr(self, "_det_held", False):
            from . import determinism
            self._det_held = False
            determinism.release(scatter_forms=self._det_scatter)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _OptimizerProxy:
    """What `self.optimizers()` returns inside training_step: zero_grad() clears the flat buffer (keeping the views),
    step() all-reduces once, unscales (precision=16), clips (Trainer(gradient_clip_val=...): where a LightningModule under
    manual optimization calls self.clip_gradients) and then steps the real optimiser."""

    def __init__(self, trainer):
        self.t = trainer

    def zero_grad(self):
        self.t.grads.zero()

    def _record_row(self):
        """Trainer._record_row, looked up at call time (tests wrap it); whoever drives the proxy with a stand-in for the trainer
        that has no logging (no `_record_row`) records nothing."""
        record = getattr(self.t, "_record_row", None)
        if record is not None:
            record()

    def _unscale_and_clip(self):
        """Trainer._unscale_and_clip; a stand-in for the trainer without it gets the unscale alone."""
        both = getattr(self.t, "_unscale_and_clip", None)
        if both is not None:
            both()
        elif self.t.scaler is not None:
            self.t.scaler.unscale_(self.t.grads.flat)

    def step(self):
        self.t.grads.all_reduce_mean(self.t.bucket_mb)        # (and what a concurrently run pass accumulated on the side)
        sc = self.t.scaler
        self._unscale_and_clip()
        if sc is not None:
            # GradScaler.step + update: the reduced (scaled) gradients are unscaled in place -- an inf on any rank reached every
            # rank through the sum, so all ranks skip together -- then AdamW, skipped on the device when found_inf is set, then
            # the new scale.  torch's own step (first step, non-plain configurations) needs the flag on the host.
            self._record_row()                                # this step's scale and found_inf: the scaler is updated below
            if self.t.fast_step is not None and self.t.fast_step.step_amp(sc.found_inf):
                sc.update(self.t.fast_step.device_step)
                return
            if not bool(sc.found_inf.item()):
                self.t.optimizer.step()
            else:
                self.t.optimizer._opt_called = True       # a skipped step still lets the LR scheduler advance
            sc.update(None)
            return
        self._record_row()
        if self.t.fast_step is not None:
            self.t.fast_step.step()
        else:
            self.t.optimizer.step()

    def __getattr__(self, name):
        return getattr(self.t.optimizer, name)

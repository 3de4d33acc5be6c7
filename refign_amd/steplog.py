"""A record of the run without the step ever waiting for the device: `StepLog`, a device ring of fp64 rows with a pinned
host mirror and one event per row (csrc/steplog.hip fills a row: rfn_steplog_gather for the step's device scalars,
rfn_grad_sqnorm_groups for the gradient norms per optimizer group), `GradClip`, which decides on those norms whether and
how far the gradient is clipped, and `TensorBoardLogger`, which writes the rows as a TensorBoard event file with no
dependency on the `tensorboard` package.

What the reference gets from Lightning's TensorBoardLogger + LearningRateMonitor + `self.log(...)`; Trainer(logger=...)
drives both (refign_amd/trainer.py).  With CPU tensors (the CPU tests' stand-in models) StepLog has the same interface
and computes the row with plain torch in fp64 -- the form the GPU tests compare the kernels with."""
import collections
import ctypes
import os
import socket
import struct
import time

import torch

from . import _lib
from ._tensor import DTYPE_CODE

# dtype codes of rfn_steplog_gather
DTYPE_CODES = {**DTYPE_CODE, torch.float64: 3, torch.int32: 4}      # the record format's two additions
MAX_GATHER = 32                 # values per launch of rfn_steplog_gather
MAX_GROUPS = 32
CHUNK = 32768                   # elements per workgroup of the norm kernel's first stage (128 KB of fp32)
NONFINITE = "grad_norm/nonfinite_chunks"


def group_runs(order, param_groups, align=1):
    """Runs `(offset, length, group)` of a flat buffer that holds the tensors of `order` one after the other, each starting
    on a multiple of `align` elements (trainer.FlatGradBuffer._order / .ALIGN): `group` is the index of the optimizer
    group the tensor belongs to; neighbouring tensors of one group merge into one run (the zero-filled padding between
    them is inside it)."""
    which = {id(p): gi for gi, g in enumerate(param_groups) for p in g["params"]}
    pad = lambda k: (k + align - 1) // align * align  # noqa: E731
    runs, off = [], 0
    for p in order:
        gi = which.get(id(p))
        if gi is None:
            raise ValueError("steplog.group_runs: a tensor of the flat buffer is in no optimizer group")
        n = pad(p.numel())
        if runs and runs[-1][2] == gi and runs[-1][0] + runs[-1][1] == off:
            runs[-1][1] += n
        else:
            runs.append([off, n, gi])
        off += n
    return [tuple(r) for r in runs]


def chunk_runs(runs, chunk=CHUNK):
    """The runs cut into pieces of at most `chunk` elements: no piece crosses a run, hence a group, boundary."""
    out = []
    for off, n, gi in runs:
        for a in range(0, n, chunk):
            out.append((off + a, min(chunk, n - a), gi))
    return out


class GradNormPlan:
    """The chunk table of one flat gradient buffer, built once: `chunks` (host list and, for a device buffer, an int64
    device tensor of nchunks x 3) and the scratch for the per-chunk partial sums."""

    def __init__(self, runs, ngroups, numel, device, chunk=CHUNK):
        if not 0 < ngroups <= MAX_GROUPS:
            raise ValueError(f"GradNormPlan: {ngroups} groups (1 ... {MAX_GROUPS})")
        self.chunks = chunk_runs(runs, chunk)
        for off, n, gi in self.chunks:
            if not (0 <= off and 0 <= n and off + n <= numel and 0 <= gi < ngroups):
                raise ValueError(f"GradNormPlan: chunk ({off}, {n}, {gi}) is outside the buffer of {numel} elements / "
                                 f"{ngroups} groups")
        self.ngroups, self.numel, self.device = ngroups, int(numel), torch.device(device)
        self.table = self.partials = None
        if self.device.type == "cuda" and self.chunks:
            self.table = torch.tensor(self.chunks, dtype=torch.int64).to(self.device)
            self.partials = torch.zeros(len(self.chunks), dtype=torch.float64, device=self.device)

    @classmethod
    def for_buffer(cls, grads, param_groups, chunk=CHUNK):
        """From a trainer.FlatGradBuffer and the optimizer's param_groups."""
        return cls(group_runs(grads._order, param_groups, grads.ALIGN), len(param_groups), grads.flat.numel(),
                   grads.flat.device, chunk)


def grad_sqnorm_groups(flat, plan, out):
    """out[0 .. G-1] <- sum of squares of `flat` per group of `plan`, out[G] <- number of non-finite chunk partials; `out`:
    G + 1 contiguous fp64 values on flat's device.  Device tensors: two launches of csrc/steplog.hip on the current stream;
    CPU tensors: the same sums with torch in fp64."""
    G = plan.ngroups
    if flat.dtype != torch.float32 or not flat.is_contiguous() or flat.numel() != plan.numel or flat.device != plan.device:
        raise RuntimeError("grad_sqnorm_groups: a contiguous fp32 buffer of the plan's size and device is required")
    if out.dtype != torch.float64 or out.numel() != G + 1 or not out.is_contiguous() or out.device != flat.device:
        raise RuntimeError("grad_sqnorm_groups: out must hold G + 1 contiguous fp64 values on the buffer's device")
    if not flat.is_cuda:
        sums, bad = [0.0] * G, 0
        part = [float((flat[o:o + n].double() ** 2).sum()) for o, n, _ in plan.chunks]
        for (_, _, gi), v in zip(plan.chunks, part):
            sums[gi] += v
            bad += 0 if v - v == 0.0 else 1
        out.copy_(torch.tensor(sums + [float(bad)], dtype=torch.float64))
        return out
    if not plan.chunks:
        out.zero_()
        return out
    _lib.call("rfn_grad_sqnorm_groups", flat.device, flat.data_ptr(), flat.numel(), plan.table.data_ptr(), len(plan.chunks), G,
              plan.partials.data_ptr(), out.data_ptr())
    return out


class GradClip:
    """Lightning's `gradient_clip_val` / `gradient_clip_algorithm` on a flat fp32 gradient buffer (Trainer drives it from
    _OptimizerProxy.step, after the all-reduce and in front of the logged row and the optimizer).

    "norm": torch.nn.utils.clip_grad_norm_(params, value) -- the 2-norm over the whole buffer, eps 1e-6, the coefficient
    at most 1; a NaN norm multiplies NaN in, an infinite one gives coefficient 0.  "value": clip_grad_value_, every element
    into [-value, value], a NaN kept.  On a device buffer the decision and the scaling stay on the device (csrc/steplog.hip;
    no host synchronisation, no floating-point atomics):
      norm            rfn_grad_sqnorm_groups, rfn_grad_clip_coef, rfn_grad_scale_f32 (which returns at once at coefficient 1)
      norm under fp16 rfn_amp_unscale_sqnorm_groups_f32 (the scaler's unscale and the norm in one pass), coef, scale
      value           the scaler's unscale (under fp16), rfn_grad_clamp_f32
    On a CPU buffer it is torch's two functions themselves on the parameters whose `.grad` are the buffer's views.
    `sqnorms` (G + 1 fp64: rfn_grad_sqnorm_groups' out, the gradient BEFORE clipping; under "value" filled only when
    asked for) and `coef` (2 fp32: the coefficient and the total norm; "norm" only) are what the logged row takes."""

    ALGORITHMS = ("norm", "value")

    def __init__(self, value, algorithm="norm"):
        if algorithm not in self.ALGORITHMS:
            raise ValueError(f"GradClip: algorithm {algorithm!r} (one of {self.ALGORITHMS})")
        self.value, self.algorithm = float(value), algorithm
        self.sqnorms = self.coef = None

    def __call__(self, grads, plan, scaler=None, want_norms=False):
        """`grads`: a trainer.FlatGradBuffer; `plan`: its GradNormPlan; `scaler`: an amp.LossScaler whose unscale is still
        to be done (it is done here, in front of the clip), or None; `want_norms`: fill `sqnorms` under "value" too."""
        flat, G = grads.flat, plan.ngroups
        if self.sqnorms is None:
            self.sqnorms = torch.zeros(G + 1, dtype=torch.float64, device=flat.device)
            self.coef = torch.ones(2, dtype=torch.float32, device=flat.device)
        norm = self.algorithm == "norm"
        if not flat.is_cuda:
            if scaler is not None:
                scaler.unscale_(flat)                         # (raises: loss scaling has no CPU form)
            if norm or want_norms:
                grad_sqnorm_groups(flat, plan, self.sqnorms)
            if norm:
                total = torch.nn.utils.clip_grad_norm_(grads.params, self.value)
                self.coef.copy_(torch.stack([torch.clamp(self.value / (total + 1e-6), max=1.0), total]))
            else:
                torch.nn.utils.clip_grad_value_(grads.params, self.value)
            return
        if norm:
            if scaler is not None:
                scaler.unscale_sqnorm_(flat, plan, self.sqnorms)
            else:
                grad_sqnorm_groups(flat, plan, self.sqnorms)
            grad_clip_coef(self.sqnorms, G, self.value, self.coef)
            grad_scale_(flat, self.coef)
            return
        if scaler is not None:
            scaler.unscale_(flat)
        if want_norms:
            grad_sqnorm_groups(flat, plan, self.sqnorms)
        grad_clamp_(flat, self.value)


def _flat_f32(flat, what):
    if not (flat.is_cuda and flat.dtype == torch.float32 and flat.is_contiguous() and flat.data_ptr() % 16 == 0 and flat.numel()):
        raise RuntimeError(f"{what}: a non-empty contiguous, 16-byte aligned fp32 device buffer is required")


def grad_clip_coef(sqnorms, ngroups, max_norm, coef):
    """coef[0] <- min(1, max_norm / (sqrt(sqnorms[0] + ... + sqnorms[ngroups - 1]) + 1e-6)), coef[1] <- that norm: one launch,
    fp64 inside.  `sqnorms`: contiguous fp64 device values (grad_sqnorm_groups' out), `coef`: 2 contiguous fp32 next to them."""
    if sqnorms.dtype != torch.float64 or not sqnorms.is_contiguous() or sqnorms.numel() < ngroups or not sqnorms.is_cuda:
        raise RuntimeError("grad_clip_coef: sqnorms must hold `ngroups` contiguous fp64 device values")
    if coef.dtype != torch.float32 or not coef.is_contiguous() or coef.numel() != 2 or coef.device != sqnorms.device:
        raise RuntimeError("grad_clip_coef: coef must hold 2 contiguous fp32 values on the device of sqnorms")
    _lib.call("rfn_grad_clip_coef", coef.device, sqnorms.data_ptr(), int(ngroups), float(max_norm), coef.data_ptr())
    return coef


def grad_scale_(flat, coef):
    """flat *= coef[0] in place, the coefficient read on the device (nothing is written when it is exactly 1)."""
    _flat_f32(flat, "grad_scale_")
    if coef.dtype != torch.float32 or coef.device != flat.device or coef.numel() < 1:
        raise RuntimeError("grad_scale_: coef must be fp32 on the buffer's device")
    _lib.call("rfn_grad_scale_f32", flat.device, flat.data_ptr(), flat.numel(), coef.data_ptr())
    return flat


def grad_clamp_(flat, clip_value):
    """Every element of flat into [-clip_value, clip_value] in place; a NaN stays a NaN."""
    _flat_f32(flat, "grad_clamp_")
    _lib.call("rfn_grad_clamp_f32", flat.device, flat.data_ptr(), flat.numel(), float(clip_value))
    return flat


def gather_scalars(tensors, row):
    """row[i] <- double(tensors[i]) for one-element device tensors of mixed dtype (f32, bf16, f16, f64, i32), one launch per
    32 values on the current stream; CPU tensors: torch."""
    if row.dtype != torch.float64 or not row.is_contiguous() or row.numel() < len(tensors):
        raise RuntimeError("gather_scalars: row must be contiguous fp64 with room for every value")
    for t in tensors:
        if not torch.is_tensor(t) or t.numel() != 1 or t.dtype not in DTYPE_CODES or t.device != row.device:
            raise TypeError("gather_scalars: one-element f32 / bf16 / f16 / f64 / i32 tensors on the row's device are required "
                            f"(got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}, "
                            f"{getattr(t, 'dtype', None)}, {getattr(t, 'device', None)})")
    if not tensors:
        return row
    if not row.is_cuda:
        row[:len(tensors)] = torch.stack([t.detach().reshape(()).double() for t in tensors])
        return row
    for a in range(0, len(tensors), MAX_GATHER):
        part = tensors[a:a + MAX_GATHER]
        ptrs = (ctypes.c_void_p * len(part))(*[t.data_ptr() for t in part])
        codes = (ctypes.c_int * len(part))(*[DTYPE_CODES[t.dtype] for t in part])
        _lib.call("rfn_steplog_gather", row.device, ptrs, codes, len(part), row.data_ptr() + 8 * a)
    return row


class _Done:
    """The event of a row on the CPU: complete as soon as it is recorded."""

    def record(self, stream=None):
        pass

    def query(self):
        return True

    def synchronize(self):
        pass


class StepLog:
    """A ring of `rows` fp64 rows on `device`, a pinned host mirror and one event per row.

    `names`: the device scalars of a row, in column order; `group_names` (optional): the optimizer groups whose gradient
    norms follow them (`grad_norm/<group>`, `grad_norm/total`, and the number of non-finite chunk partials).
    record() enqueues everything on the current stream and returns; poll() / flush() hand back the rows whose events
    have completed as `(step, {name: float})`, in step order.  The mirror is read only after the row's event reports
    complete.  `stalls` counts how often record() had to wait because every row was pending."""

    def __init__(self, device, names, rows=64, group_names=None, event_factory=None):
        self.device = torch.device(device)
        self.names, self.group_names = list(names), list(group_names) if group_names is not None else None
        if len(set(self.names)) != len(self.names):
            raise ValueError("StepLog: duplicate names")
        self.rows = int(rows)
        if self.rows < 1:
            raise ValueError("StepLog: rows must be positive")
        ng = len(self.group_names) + 1 if self.group_names is not None else 0
        self.width = max(1, len(self.names) + ng)
        self.ring = torch.zeros(self.rows, self.width, dtype=torch.float64, device=self.device)
        cuda = self.device.type == "cuda"
        self.mirror = torch.zeros(self.rows, self.width, dtype=torch.float64, pin_memory=True) if cuda else self.ring
        make = event_factory or (torch.cuda.Event if cuda else _Done)
        self.events = [make() for _ in range(self.rows)]
        self._pending = collections.deque()        # (slot, step, host values, with norms, tensors kept alive), oldest first
        self._ready = []
        self._next = 0
        self.stalls = 0

    def record(self, step, scalars, grads=None, host=None, sqnorms=None):
        """`scalars`: {name: one-element tensor on the device} for every name of the log; `grads`: (flat buffer, GradNormPlan)
        or None; `sqnorms`: instead of `grads`, the G + 1 values grad_sqnorm_groups has already computed (GradClip.sqnorms: the
        norms the clip decided on; they are copied, not computed again); `host`: {name: python number} that goes with the row
        as it is.  Never waits for the device, unless all rows are pending: then for the oldest row's event (counted in
        `stalls`)."""
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("StepLog.record: the current stream is capturing a graph; the copy to the host mirror and the "
                               "row's event would be replayed with every replay of that graph")
        if set(scalars) != set(self.names):
            raise KeyError(f"StepLog.record: got {sorted(scalars)}, the log was made for {sorted(self.names)}")
        if (grads is not None or sqnorms is not None) and self.group_names is None:
            raise ValueError("StepLog.record: this log was made without group names")
        if grads is not None and sqnorms is not None:
            raise ValueError("StepLog.record: grads or sqnorms, not both")
        if len(self._pending) == self.rows:
            while self._pending and self.events[self._pending[0][0]].query():
                self._take()                                  # rows that are complete but were not polled yet
        if len(self._pending) == self.rows:
            self.stalls += 1
            self.events[self._pending[0][0]].synchronize()
            self._take()
        slot = self._next
        row = self.ring[slot]
        tensors = [scalars[k] for k in self.names]
        gather_scalars(tensors, row)
        if grads is not None:
            flat, plan = grads
            if plan.ngroups != len(self.group_names):
                raise ValueError("StepLog.record: the plan's group count differs from the log's")
            grad_sqnorm_groups(flat, plan, row[len(self.names):len(self.names) + plan.ngroups + 1])
        if sqnorms is not None:
            if sqnorms.numel() != len(self.group_names) + 1:
                raise ValueError("StepLog.record: sqnorms must hold one value per group and the non-finite count")
            row[len(self.names):len(self.names) + sqnorms.numel()].copy_(sqnorms)
        if self.mirror is not self.ring:
            self.mirror[slot].copy_(row, non_blocking=True)
        self.events[slot].record()
        self._next = (slot + 1) % self.rows
        self._pending.append((slot, int(step), dict(host or {}), grads is not None or sqnorms is not None, tensors))

    def _take(self):
        """The oldest pending row (its event has completed) from the mirror into the ready list."""
        slot, step, host, normed, _ = self._pending.popleft()
        vals = self.mirror[slot].tolist()
        out = dict(zip(self.names, vals))
        if normed:
            n0, G = len(self.names), len(self.group_names)
            sq = vals[n0:n0 + G]
            for name, v in zip(self.group_names, sq):
                out[f"grad_norm/{name}"] = _sqrt(v)
            out["grad_norm/total"] = _sqrt(sum(sq))
            out[NONFINITE] = vals[n0 + G]
        out.update(host)
        self._ready.append((step, out))

    def poll(self):
        while self._pending and self.events[self._pending[0][0]].query():
            self._take()
        out, self._ready = self._ready, []
        return out

    def flush(self):
        """Waits for the outstanding rows' events (not for the device) and returns every row not yet handed out."""
        while self._pending:
            self.events[self._pending[0][0]].synchronize()
            self._take()
        out, self._ready = self._ready, []
        return out

    @property
    def pending(self):
        return len(self._pending)


def _sqrt(v):
    return v ** 0.5 if v >= 0.0 else float("nan")       # (inf -> inf, NaN -> NaN: a skipped fp16 step shows as it is)


# -- TensorBoard event files ---------------------------------------------------------------------------------------------
def _crc_table():
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        table.append(c)
    return table


_CRC = _crc_table()


def crc32c(data):
    """CRC-32C (Castagnoli), the checksum of TFRecord framing."""
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def _masked_crc(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def _varint(n):
    n &= (1 << 64) - 1
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def _field_bytes(number, payload):
    return _varint(number << 3 | 2) + _varint(len(payload)) + payload


def encode_event(wall_time, step=None, file_version=None, scalars=None):
    """One tensorflow Event message: wall_time (1, double), step (2, int64), file_version (3, string) or summary (5) with one
    Value{tag (1, string), simple_value (2, float)} per entry of `scalars`."""
    out = b"\x09" + struct.pack("<d", wall_time)
    if step is not None:
        out += b"\x10" + _varint(int(step))
    if file_version is not None:
        out += _field_bytes(3, file_version.encode())
    if scalars is not None:
        summary = b"".join(_field_bytes(1, _field_bytes(1, tag.encode()) + b"\x15" + struct.pack("<f", _f32(v)))
                           for tag, v in scalars)
        out += _field_bytes(5, summary)
    return out


def _f32(v):
    try:
        return struct.unpack("<f", struct.pack("<f", v))[0]
    except OverflowError:                                  # finite in fp64, beyond fp32: what a cast gives
        return float("inf") if v > 0 else float("-inf")


def tfrecord(payload):
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", _masked_crc(head)) + payload + struct.pack("<I", _masked_crc(payload))


class TensorBoardLogger:
    """Scalars as a TensorBoard event file `events.out.tfevents.<time>.<host>.<pid>` under
    `<save_dir>/<name>/version_<n>` (the next free n when `version` is None), written by hand: TFRecord framing, a first
    record with file_version "brain.Event:2", then one Event per log_metrics call.  The directory and the file are made on
    the first write; writes are buffered appends, flush() / close() push them to the disk.  A second logger on the same
    version directory (a resumed run) writes a second file next to the first, which is how TensorBoard reads a continued
    run."""

    def __init__(self, save_dir, name="default", version=None):
        self.save_dir, self.name = str(save_dir), "" if name is None else str(name)
        root = os.path.join(self.save_dir, self.name)
        if version is None:
            taken = []
            if os.path.isdir(root):
                for d in os.listdir(root):
                    if d.startswith("version_") and d[8:].isdigit() and os.path.isdir(os.path.join(root, d)):
                        taken.append(int(d[8:]))
            version = max(taken) + 1 if taken else 0
        self.version = version
        self.log_dir = os.path.join(root, version if isinstance(version, str) else f"version_{int(version)}")
        self.path = None
        self._file = None

    def _open(self):
        os.makedirs(self.log_dir, exist_ok=True)
        base = f"events.out.tfevents.{int(time.time()):010d}.{socket.gethostname()}.{os.getpid()}"
        path, k = os.path.join(self.log_dir, base), 0
        while os.path.exists(path):                       # two loggers of one process within one second
            k += 1
            path = os.path.join(self.log_dir, f"{base}.{k}")
        self.path = path
        self._file = open(path, "ab", buffering=1 << 20)
        self._file.write(tfrecord(encode_event(time.time(), file_version="brain.Event:2")))

    def log_metrics(self, metrics, step):
        """One Event at `step` with every entry of `metrics` ({tag: number}) as a scalar."""
        if not metrics:
            return
        if self._file is None:
            if self.path is not None:
                raise RuntimeError("TensorBoardLogger: closed")
            self._open()
        self._file.write(tfrecord(encode_event(time.time(), step=step, scalars=[(k, float(v)) for k, v in metrics.items()])))

    def flush(self):
        if self._file is not None:
            self._file.flush()

    def close(self):
        if self._file is not None:
            self._file.close()
            self._file = None

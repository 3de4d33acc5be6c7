"""Trainer logging on the CPU: the TensorBoard event file read back by a reader of this file's own (framing, both CRCs,
the three message types), version_<n> numbering and a resumed run's second file, config.trainer_logging on the
reference's configs, a stand-in model through Trainer.fit with a logger, the ring logic of StepLog with rows made to stay
pending, two ranks over gloo, and the bindings of the two new entry points."""
import glob
import math
import os
import struct

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml
from test_config_cpu import _REF_CONFIG_NAMES, _REF_CONFIGS
from test_ddp_cpu import _free_port
from test_fit_cpu import TRAINER_YAML, _batches, _stub_validation, _val_batch
from test_resume_cpu import GROUPS, _trainer


# ---------------------------------------------------------------------------------------------------------------------
# a reader of event files that shares no code with the writer
# ---------------------------------------------------------------------------------------------------------------------
def crc32c(data):
    crc = 0xFFFFFFFF
    for byte in data:
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 & -(crc & 1))
    return crc ^ 0xFFFFFFFF


def _masked(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def _read_varint(buf, pos):
    out, shift = 0, 0
    while True:
        b = buf[pos]
        pos += 1
        out |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return out, pos


def _fields(buf):
    """[(field number, wire type, value)] of one protobuf message (varint, 64-bit, length-delimited, 32-bit)."""
    pos, out = 0, []
    while pos < len(buf):
        key, pos = _read_varint(buf, pos)
        num, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = _read_varint(buf, pos)
        elif wt == 1:
            v, pos = buf[pos:pos + 8], pos + 8
        elif wt == 2:
            n, pos = _read_varint(buf, pos)
            v, pos = buf[pos:pos + n], pos + n
        elif wt == 5:
            v, pos = buf[pos:pos + 4], pos + 4
        else:
            raise AssertionError(f"wire type {wt}")
        out.append((num, wt, v))
    return out


def read_events(path):
    """-> [{"wall_time", "step", "file_version", "scalars": [(tag, value)]}], every record's two CRCs verified."""
    assert crc32c(b"123456789") == 0xE3069283
    data, pos, events = open(path, "rb").read(), 0, []
    while pos < len(data):
        head = data[pos:pos + 8]
        (n,) = struct.unpack("<Q", head)
        assert struct.unpack("<I", data[pos + 8:pos + 12])[0] == _masked(head), "length CRC"
        payload = data[pos + 12:pos + 12 + n]
        assert len(payload) == n
        assert struct.unpack("<I", data[pos + 12 + n:pos + 16 + n])[0] == _masked(payload), "payload CRC"
        pos += 16 + n
        ev = {"wall_time": None, "step": 0, "file_version": None, "scalars": []}
        for num, wt, v in _fields(payload):                                  # Event
            if (num, wt) == (1, 1):
                ev["wall_time"] = struct.unpack("<d", v)[0]
            elif (num, wt) == (2, 0):
                ev["step"] = v
            elif (num, wt) == (3, 2):
                ev["file_version"] = v.decode()
            elif (num, wt) == (5, 2):
                for n2, w2, val in _fields(v):                               # Summary
                    assert (n2, w2) == (1, 2)
                    tag = simple = None
                    for n3, w3, x in _fields(val):                           # Summary.Value
                        if (n3, w3) == (1, 2):
                            tag = x.decode()
                        elif (n3, w3) == (2, 5):
                            simple = struct.unpack("<f", x)[0]
                        else:
                            raise AssertionError(f"Value field {n3} / wire type {w3}")
                    ev["scalars"].append((tag, simple))
            else:
                raise AssertionError(f"Event field {num} / wire type {wt}")
        events.append(ev)
    return events


def _f32(v):
    return torch.tensor(v, dtype=torch.float64).float().item()


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _rows_of(path):
    evs = read_events(path)
    assert evs[0]["file_version"] == "brain.Event:2" and not evs[0]["scalars"] and evs[0]["wall_time"] > 1.5e9
    assert all(e["file_version"] is None and e["wall_time"] > 1.5e9 for e in evs[1:])
    return [(e["step"], dict(e["scalars"])) for e in evs[1:]]


def _event_files(log_dir):
    return sorted(glob.glob(os.path.join(log_dir, "events.out.tfevents.*")))


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the file
# ---------------------------------------------------------------------------------------------------------------------
def test_event_file_reads_back(tmp_path):
    from refign_amd.steplog import TensorBoardLogger
    lg = TensorBoardLogger(str(tmp_path), name="run")
    assert lg.log_dir == str(tmp_path / "run" / "version_0") and not os.path.exists(lg.log_dir)     # nothing before a write
    logged = [(0, {"train_loss_src": 2.944438934326172, "lr-AdamW/head_weight": 6e-11}),
              (49, {"a/b": 1 / 3, "neg": -1e-30, "big": 1e300, "tiny": 1e-60}),
              (2 ** 40 + 7, {"amp/found_inf": 1.0, "grad_norm/total": float("inf"), "grad_norm/head_bias": float("nan")}),
              (50, {"unicode/é": 0.0})]
    for step, row in logged:
        lg.log_metrics(row, step)
    lg.log_metrics({}, 51)                                                    # nothing to say: no record
    lg.close()
    files = _event_files(lg.log_dir)
    assert len(files) == 1 and files[0] == lg.path
    parts = os.path.basename(files[0]).split(".")
    assert parts[:3] == ["events", "out", "tfevents"] and parts[3].isdigit() and parts[-1] == str(os.getpid())
    rows = _rows_of(files[0])
    assert [s for s, _ in rows] == [s for s, _ in logged]
    for (_, got), (_, want) in zip(rows, logged):
        assert list(got) == list(want)
        assert all(_same(got[k], _f32(want[k])) for k in want), (got, want)
    with pytest.raises(RuntimeError, match="closed"):
        lg.log_metrics({"x": 1.0}, 52)


def test_version_numbering_and_a_resumed_runs_second_file(tmp_path):
    from refign_amd.steplog import TensorBoardLogger
    a = TensorBoardLogger(str(tmp_path), name="run")
    a.log_metrics({"x": 0.0}, 0)
    a.log_metrics({"x": 1.0}, 1)
    a.close()
    b = TensorBoardLogger(str(tmp_path), name="run")                          # the next free n
    assert b.version == 1 and b.log_dir.endswith("version_1")
    b.log_metrics({"x": 5.0}, 0)
    b.close()
    os.makedirs(tmp_path / "run" / "version_7")
    assert TensorBoardLogger(str(tmp_path), name="run").version == 8
    assert TensorBoardLogger(str(tmp_path), name="other").version == 0
    assert TensorBoardLogger(str(tmp_path)).log_dir == str(tmp_path / "default" / "version_0")
    # the resumed run: the same version directory, a second file, labels that continue
    c = TensorBoardLogger(str(tmp_path), name="run", version=0)
    assert c.log_dir == a.log_dir
    c.log_metrics({"x": 2.0}, 2)
    c.flush()
    files = _event_files(a.log_dir)
    assert len(files) == 2 and set(files) == {a.path, c.path}
    assert [s for s, _ in _rows_of(a.path)] + [s for s, _ in _rows_of(c.path)] == [0, 1, 2]   # (flush() made it readable)
    c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3: configs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _REF_CONFIG_NAMES)
def test_trainer_logging_on_the_reference_configs(name, tmp_path, monkeypatch):
    path = next((p for p in _REF_CONFIGS if p.endswith("/configs/" + name)), None)
    if path is None:
        pytest.skip(f"reference checkout not present (configs/{name})")
    from refign_amd import config
    from refign_amd.steplog import TensorBoardLogger
    monkeypatch.chdir(tmp_path)                                               # (save_dir is relative in every one of them)
    cfg = config.load_config(path)
    spec = cfg["trainer"]["logger"]
    spec = spec[0] if isinstance(spec, list) else spec
    got = config.trainer_logging(cfg)
    assert set(got) == {"logger", "log_every_n_steps", "log_lr"}
    assert isinstance(got["logger"], TensorBoardLogger)
    assert got["logger"].save_dir == spec["init_args"]["save_dir"] and got["logger"].name == spec["init_args"]["name"]
    assert got["log_every_n_steps"] == cfg["trainer"].get("log_every_n_steps", 50)
    assert got["log_lr"] is any(c["class_path"].endswith("LearningRateMonitor") for c in cfg["trainer"]["callbacks"])
    assert got["log_lr"] is True
    assert os.listdir(tmp_path) == []                                         # reading a config writes nothing
    assert set(config.trainer_kwargs(cfg)) == {"max_steps", "val_every_n_steps", "save_last", "sync_batchnorm", "precision"}


def test_trainer_logging_from_yaml_text(tmp_path):
    from refign_amd import config
    from refign_amd.steplog import TensorBoardLogger
    got = config.trainer_logging(yaml.safe_load(TRAINER_YAML))
    assert isinstance(got["logger"], TensorBoardLogger) and (got["logger"].save_dir, got["logger"].name) == \
        ("lightning_logs", "some_run")
    assert got["log_every_n_steps"] == 50 and got["log_lr"] is True
    bare = config.trainer_logging(yaml.safe_load("trainer:\n  max_steps: 100\n"))
    assert bare == {"logger": None, "log_every_n_steps": 50, "log_lr": False}
    assert config.trainer_logging({}) == bare and config.trainer_logging(None) == bare
    one = config.trainer_logging(yaml.safe_load(
        "trainer:\n  log_every_n_steps: 7\n  logger:\n    class_path: pytorch_lightning.loggers.TensorBoardLogger\n"
        f"    init_args:\n      save_dir: {tmp_path}\n      name: r\n      version: 3\n"))
    assert one["log_every_n_steps"] == 7 and one["logger"].log_dir == str(tmp_path / "r" / "version_3")
    other = config.trainer_logging(yaml.safe_load(
        "trainer:\n  logger:\n    class_path: pytorch_lightning.loggers.CSVLogger\n    init_args:\n      save_dir: x\n"))
    assert other["logger"] is None


# ---------------------------------------------------------------------------------------------------------------------
# 4: a stand-in model through fit
# ---------------------------------------------------------------------------------------------------------------------
def _stub_logged_training(trainer, seen, seed=11):
    """A training_step in the shape of the real one: zero_grad, losses through model.log (mixed dtypes), gradients into the
    flat buffer, optimizer and scheduler step, global_step.  `seen[label]` <- what a row of that step should hold."""
    model, gen = trainer.model, torch.Generator().manual_seed(seed)

    def training_step(batch, batch_idx):
        opt, sch = model.optimizers(), model.lr_schedulers()
        opt.zero_grad()
        v = float(batch["image_src"])
        model.log("train_loss_src", torch.tensor(1.5 + v / 3))
        model.log("train_loss_featdist_src", torch.tensor(0.1 * v, dtype=torch.bfloat16))
        model.log("train_loss_uda_trg", torch.tensor(2.0 - v / 7, dtype=torch.float16))
        for p in trainer.grads.params:                   # through the views: the padding between them stays zero
            p.grad.copy_(torch.randn(p.shape, generator=gen) * 10.0 ** (model.global_step % 5 - 2))
        want = {k: float(t.double()) for k, t in model.logged.items() if k.startswith("train_")}
        sq = [float(sum((p.grad.double() ** 2).sum() for p in g["params"])) for g in trainer.optimizer.param_groups]
        want.update({f"grad_norm/{g['name']}": s ** 0.5 for g, s in zip(trainer.optimizer.param_groups, sq)})
        want["grad_norm/total"] = sum(sq) ** 0.5
        want.update({f"lr-AdamW/{g['name']}": float(g["lr"]) for g in trainer.optimizer.param_groups})
        seen[int(model.global_step)] = want
        opt.step()
        sch.step()
        model.global_step += 1

    model.training_step = training_step


def test_fit_with_a_logger_on_a_stand_in_model(tmp_path):
    from refign_amd.steplog import TensorBoardLogger
    lg = TensorBoardLogger(str(tmp_path / "logs"), name="cpu")
    tr = _trainer(logger=lg, log_every_n_steps=3)
    seen = {}
    _stub_logged_training(tr, seen)
    _stub_validation(tr, [])
    tr.model.train()
    hist = tr.fit(_batches(4), val_loaders={"ACDC": [_val_batch(1)]}, max_steps=10, val_every_n_steps=4,
                  ckpt_dir=str(tmp_path / "ck"))
    assert [s for s, _ in hist] == [4, 8]
    train_rows = [(s, r) for s, r in tr.log_history if "train_loss_src" in r]
    val_rows = [(s, r) for s, r in tr.log_history if "train_loss_src" not in r]
    assert [s for s, _ in train_rows] == [2, 5, 8]                             # (s + 1) % 3 == 0, labelled s
    names = {"train_loss_src", "train_loss_featdist_src", "train_loss_uda_trg", "grad_norm/total",
             "grad_norm/nonfinite_chunks"} | {f"grad_norm/{g}" for g in GROUPS} | {f"lr-AdamW/{g}" for g in GROUPS}
    for s, row in train_rows:
        assert set(row) == names and row["grad_norm/nonfinite_chunks"] == 0.0
        for k, want in seen[s].items():
            if k.startswith("grad_norm/"):
                assert abs(row[k] - want) <= 1e-12 * want, (s, k, row[k], want)
            else:
                assert row[k] == want, (s, k, row[k], want)              # losses and rates: exact, in fp64
    assert len({row["lr-AdamW/head_weight"] for _, row in train_rows}) == 3   # the warm-up moves: each step its own rate
    assert [(s, r) for s, r in val_rows] == [(s, m) for s, m in hist]
    assert [s for s, _ in tr.log_history] == [2, 4, 5, 8, 8]                   # in the order things happened
    # the checkpoint holds nothing of the logger: the parent's key set
    ck = torch.load(str(tmp_path / "ck" / "last.ckpt"), map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "global_step", "pytorch-lightning_version", "state_dict", "loops", "callbacks",
                       "optimizer_states", "lr_schedulers", "refign_amd"}
    assert set(ck["refign_amd"]) == {"world_size", "precision", "rng", "scaler_skipped"} and ck["callbacks"] == {}
    assert tr.flush_log() == 0                                                # no stall
    tr.close()
    # the file holds log_history after fp32 rounding
    files = _event_files(lg.log_dir)
    assert len(files) == 1
    rows = _rows_of(files[0])
    assert [s for s, _ in rows] == [s for s, _ in tr.log_history]
    for (_, got), (_, want) in zip(rows, tr.log_history):
        assert list(got) == list(want) and all(_same(got[k], _f32(want[k])) for k in want)
    # a resumed run on the same directory: a second file, labels that continue
    lg2 = TensorBoardLogger(str(tmp_path / "logs"), name="cpu", version=0)
    tr2 = _trainer(logger=lg2, log_every_n_steps=3, ckpt_path=str(tmp_path / "ck" / "last.ckpt"))
    _stub_logged_training(tr2, {})
    tr2.fit(_batches(4), max_steps=15)
    tr2.close()
    files = _event_files(lg.log_dir)
    assert len(files) == 2
    assert [s for s, _ in _rows_of(lg2.path)] == [11, 14]


def test_logger_none_changes_nothing():
    tr = _trainer()
    seen = {}
    _stub_logged_training(tr, seen)
    tr.fit(_batches(4), max_steps=4)
    assert tr.logger is None and tr._steplog is None and tr.log_history == [] and tr.flush_log() == 0
    tr.close()
    with pytest.raises(ValueError, match="log_every_n_steps"):
        _trainer(logger=object(), log_every_n_steps=0)


def test_per_class_results_become_one_scalar_per_class():
    """test(): a per-class list becomes <name>/<class index> at the current global_step; any object with log_metrics / flush /
    close serves as a logger; close() closes it."""
    from refign_amd.metrics import IoU, MyMetricCollection
    rows = []

    class Memory:
        def log_metrics(self, metrics, step):
            rows.append((step, dict(metrics)))

        def flush(self):
            pass

        def close(self):
            rows.append("closed")

    tr = _trainer(logger=Memory(), log_every_n_steps=1)
    model = tr.model
    model.test_metrics = MyMetricCollection({"test_ACDC_IoU": IoU(num_classes=4, ignore_index=255, average="none")})
    model.test_step = lambda batch, batch_idx=0, dataloader_idx=0, src_name="": \
        model.test_metrics["test_ACDC_IoU"](batch["pred"], batch["semantic"])
    model.global_step = 6
    out = tr.test({"ACDC": [_val_batch(4)]})
    assert rows == [(6, {f"test_ACDC_IoU/{i}": v for i, v in enumerate(out["test_ACDC_IoU"])})]
    tr.close()
    assert rows[-1] == "closed"


# ---------------------------------------------------------------------------------------------------------------------
# 5: the ring
# ---------------------------------------------------------------------------------------------------------------------
class _FakeEvent:
    """Pending until the test says otherwise; a wait completes it (and is counted)."""
    waits = 0

    def __init__(self):
        self.done = True

    def record(self, stream=None):
        self.done = False

    def query(self):
        return self.done

    def synchronize(self):
        if not self.done:
            _FakeEvent.waits += 1
        self.done = True


def test_ring_keeps_order_loses_nothing_and_counts_stalls():
    from refign_amd.steplog import StepLog
    _FakeEvent.waits = 0
    log = StepLog("cpu", ["a", "b"], rows=4, event_factory=_FakeEvent)
    rec = lambda s: log.record(s, {"a": torch.tensor(float(s)), "b": torch.tensor(s, dtype=torch.int32)},  # noqa: E731
                               host={"h": s * 0.5})
    for s in range(4):
        rec(s)
    assert log.pending == 4 and log.poll() == [] and log.stalls == 0           # nothing complete: nothing handed out
    log.events[0].done = log.events[1].done = True
    log.events[3].done = True                                                  # (2 is not: 3 must wait behind it)
    assert [s for s, _ in log.poll()] == [0, 1] and log.pending == 2
    rec(4)
    rec(5)                                                                     # into the two free rows
    assert log.pending == 4 and log.stalls == 0
    rec(6)                                                                     # full: waits for the oldest (2), once
    assert log.stalls == 1 and _FakeEvent.waits == 1 and log.pending == 4
    rec(7)                                                                     # full again, but row 3's event had completed:
    assert log.stalls == 1 and _FakeEvent.waits == 1 and log.pending == 4      # read out without a wait, no stall
    got = log.poll()                                                           # 2 and 3 were read out when their rows were needed
    assert [s for s, _ in got] == [2, 3]
    rest = log.flush()
    assert [s for s, _ in rest] == [4, 5, 6, 7] and log.pending == 0 and log.poll() == [] and log.flush() == []
    for s, row in got + rest:
        assert row == {"a": float(s), "b": float(s), "h": s * 0.5}             # each row its own values: none overwritten
    with pytest.raises(KeyError):
        log.record(8, {"a": torch.tensor(1.0)})
    with pytest.raises(TypeError):
        log.record(8, {"a": torch.tensor(1.0), "b": torch.tensor([1, 2], dtype=torch.int32)})
    with pytest.raises(TypeError):
        log.record(8, {"a": torch.tensor(1.0), "b": torch.tensor(1, dtype=torch.int64)})


def test_group_runs_and_cpu_norms():
    """Neighbours of one group merge, chunks do not cross a group boundary, a group without parameters sums to zero, an
    infinity shows in its group and in the count."""
    from refign_amd.steplog import GradNormPlan, StepLog, chunk_runs, group_runs
    ps = [torch.zeros(n) for n in (5, 64, 1, 130, 7)]
    groups = [{"params": [ps[0], ps[1]]}, {"params": [ps[2], ps[4]]}, {"params": []}, {"params": [ps[3]]}]
    runs = group_runs(ps, groups, align=64)
    assert runs == [(0, 128, 0), (128, 64, 1), (192, 192, 3), (384, 64, 1)]
    assert chunk_runs(runs, 100) == [(0, 100, 0), (100, 28, 0), (128, 64, 1), (192, 100, 3), (292, 92, 3), (384, 64, 1)]
    with pytest.raises(ValueError):
        group_runs(ps + [torch.zeros(1)], groups)
    flat = torch.randn(448, generator=torch.Generator().manual_seed(2))
    plan = GradNormPlan(runs, 4, 448, "cpu", chunk=100)
    with pytest.raises(ValueError):
        GradNormPlan(runs, 4, 447, "cpu")
    log = StepLog("cpu", [], group_names=["g0", "g1", "empty", "g3"])
    log.record(0, {}, grads=(flat, plan))
    flat2 = flat.clone()
    flat2[200] = float("inf")
    log.record(1, {}, grads=(flat2, plan))
    (_, r0), (_, r1) = log.flush()
    sq = lambda a, b: float((flat[a:b].double() ** 2).sum())  # noqa: E731
    want = [sq(0, 128) ** 0.5, (sq(128, 192) + sq(384, 448)) ** 0.5, 0.0, sq(192, 384) ** 0.5]
    for name, w in zip(["g0", "g1", "empty", "g3"], want):
        assert abs(r0[f"grad_norm/{name}"] - w) <= 1e-12 * max(w, 1.0)
    assert abs(r0["grad_norm/total"] - float((flat.double() ** 2).sum()) ** 0.5) <= 1e-12 * r0["grad_norm/total"]
    assert r0["grad_norm/nonfinite_chunks"] == 0.0
    assert r1["grad_norm/g3"] == float("inf") and r1["grad_norm/total"] == float("inf")
    assert r1["grad_norm/nonfinite_chunks"] == 1.0 and r1["grad_norm/g0"] == r0["grad_norm/g0"]


# ---------------------------------------------------------------------------------------------------------------------
# 6: two ranks
# ---------------------------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, world, port, out):
    from refign_amd.steplog import TensorBoardLogger
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RFN_STALL_S="120")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    lg = TensorBoardLogger(out, name="ddp")
    tr = _trainer(logger=lg, log_every_n_steps=2)
    _stub_logged_training(tr, {}, seed=20 + rank)
    tr.fit(_batches(3), max_steps=4)
    torch.save({"rows": tr.log_history, "has_logger": tr.logger is not None, "path": lg.path}, f"{out}/r{rank}.pt")
    tr.close()
    dist.destroy_process_group()


def test_two_ranks_one_event_file(tmp_path):
    port, out = _free_port(), str(tmp_path)
    mp.spawn(_two_rank_worker, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = (torch.load(f"{out}/r{k}.pt", weights_only=False) for k in range(2))
    assert r0["has_logger"] and not r1["has_logger"] and r1["rows"] == [] and r1["path"] is None
    files = glob.glob(os.path.join(out, "ddp", "*", "events.out.tfevents.*"))
    assert files == [r0["path"]]
    rows = _rows_of(files[0])
    assert [s for s, _ in rows] == [s for s, _ in r0["rows"]] == [1, 3]
    assert all(_same(got[k], _f32(want[k])) for (_, got), (_, want) in zip(rows, r0["rows"]) for k in want)


# ---------------------------------------------------------------------------------------------------------------------
# 7: bindings
# ---------------------------------------------------------------------------------------------------------------------
def test_bindings():
    import ctypes

    import refign_amd
    from refign_amd import _lib
    lib = ctypes.CDLL(refign_amd.library_path())
    for name in ("rfn_steplog_gather", "rfn_grad_sqnorm_groups"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert refign_amd.abi_version() == 5
    # argument errors are decided on the host: nothing is launched, so they can be seen without a GPU
    bound = _lib.load_library()
    one = (ctypes.c_void_p * 1)(64)
    code = (ctypes.c_int * 1)(0)
    assert bound.rfn_steplog_gather(one, code, 0, 64, None) == -1
    assert bound.rfn_steplog_gather(one, code, 33, 64, None) == -1
    assert bound.rfn_steplog_gather(one, code, 1, None, None) == -1
    assert bound.rfn_steplog_gather(one, (ctypes.c_int * 1)(5), 1, 64, None) == -1
    assert bound.rfn_steplog_gather((ctypes.c_void_p * 1)(None), code, 1, 64, None) == -1
    assert b"dtype code 5" in bound.rfn_last_error() or b"null" in bound.rfn_last_error()
    assert bound.rfn_grad_sqnorm_groups(None, 4, 64, 1, 1, 64, 64, None) == -1
    assert bound.rfn_grad_sqnorm_groups(64, 4, 64, 1, 33, 64, 64, None) == -1
    assert bound.rfn_grad_sqnorm_groups(64, 4, 64, 0, 1, 64, 64, None) == -1
    assert bound.rfn_grad_sqnorm_groups(68, 4, 64, 1, 1, 64, 64, None) == -1           # not 16-byte aligned

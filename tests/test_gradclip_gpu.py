"""GPU: gradient clipping and accumulation -- the four entry points on raw buffers (rfn_grad_clip_coef, rfn_grad_scale_f32,
rfn_grad_clamp_f32, rfn_amp_unscale_sqnorm_groups_f32) and Trainer(gradient_clip_val=, gradient_clip_algorithm=,
accumulate_grad_batches=) on the matcher's 128 x 160 golden and the small UDA model."""
import math

import numpy as np
import pytest
import torch
from conftest import golden
from test_matcher_gpu import matcher_batch
from test_matcher_trainer_gpu import FP16_SCALE, LOSSES, Memory, build

pytestmark = pytest.mark.gpu

NEW_ENTRY_POINTS = ("rfn_grad_clip_coef", "rfn_grad_scale_f32", "rfn_grad_clamp_f32", "rfn_amp_unscale_sqnorm_groups_f32")
SIZES = (1, 3, 4, 5, 255, 1024, 2 * 16384 + 7)
CONTENTS = ("normal", "zero", "1e30", "denormal", "inf", "nan")
CLIP = 1.0                               # far below the matcher's recorded gradient norm of 7.3e4 on this batch


@pytest.fixture(scope="module")
def z():
    return golden("matcher_step_128x160")


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _content(kind, n, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + n)
    x = torch.randn(n, generator=g)
    if kind == "zero":
        x.zero_()
    elif kind == "1e30":
        x = torch.where(x >= 0, 1.0, -1.0) * 1e30         # squares overflow fp32, not fp64
    elif kind == "denormal":
        x = x * 1e-42
    elif kind == "inf":
        x[n // 2] = float("inf")
    elif kind == "nan":
        x[n // 2] = float("nan")
    return x.to(dev)


def _plan(chunks, G, n, dev):
    """A GradNormPlan with exactly these chunks (a zero-length one included, which chunk_runs would drop)."""
    from refign_amd.steplog import GradNormPlan
    plan = GradNormPlan([], G, n, dev)
    plan.chunks = list(chunks)
    plan.table = torch.tensor(plan.chunks, dtype=torch.int64).reshape(-1, 3).to(dev)
    plan.partials = torch.zeros(len(plan.chunks), dtype=torch.float64, device=dev)
    return plan


def _whole(n, dev, chunk=16384):
    from refign_amd.steplog import GradNormPlan
    return GradNormPlan([(0, n, 0)], 1, n, dev, chunk)


def _bits(t):
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def _ordered(t):
    """fp32 -> integers whose difference counts the representable values in between."""
    i = t.detach().contiguous().view(torch.int32).to(torch.int64).cpu()
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps(a, b):
    return (_ordered(a) - _ordered(b)).abs()


def _same_bits_or_both_nan(a, b):
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(a)
    return bool((nan == torch.isnan(b)).all()) and torch.equal(_bits(a[~nan]), _bits(b[~nan]))


# ---------------------------------------------------------------------------------------------------------------------
# kernels: norm -> coefficient -> scale
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("n", SIZES)
def test_coef_and_scale_on_raw_buffers(dev, n, kind):
    """coef within 1 ulp of the fp64 host value; the scaled buffer is the fp32 product with the coefficient read back, bit for
    bit; every element within 2 ulp (one rounding of the coefficient, one of the product) of clip_grad_norm_ on fp64 copies."""
    from refign_amd.steplog import grad_clip_coef, grad_scale_, grad_sqnorm_groups
    max_norm = 0.25
    flat = _content(kind, n, dev)
    before = flat.clone()
    plan = _whole(n, dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    coef = torch.full((2,), -7.0, dtype=torch.float32, device=dev)
    grad_sqnorm_groups(flat, plan, out)
    grad_clip_coef(out, 1, max_norm, coef)
    grad_scale_(flat, coef)
    host = before.cpu()
    total = math.sqrt(float((host.double() ** 2).sum())) if kind not in ("inf", "nan") else float(kind)
    got_c, got_t = coef.cpu()[0], coef.cpu()[1]
    print(f"\nn={n} {kind}: coef {float(got_c)!r} total {float(got_t)!r} (host {total!r})")
    if kind == "nan":
        assert math.isnan(float(got_c)) and math.isnan(float(got_t))
        assert bool(torch.isnan(flat).all())                                   # NaN throughout, as torch multiplies it in
        return
    if kind == "inf":
        assert float(got_c) == 0.0 and math.isinf(float(got_t))
    else:
        c = max_norm / (total + 1e-6)
        want_c = torch.tensor(min(1.0, c), dtype=torch.float64).to(torch.float32)
        want_t = torch.tensor(total, dtype=torch.float64).to(torch.float32)
        assert int(_ulps(got_c, want_c)) <= 1 and int(_ulps(got_t, want_t)) <= 1
    if kind in ("zero", "denormal"):
        assert float(got_c) == 1.0
        assert torch.equal(_bits(flat), _bits(before))                          # (all-zero gradients stay zero)
    product = host * got_c                                                      # fp32 on the host: one rounding, as the kernel's
    assert _same_bits_or_both_nan(flat, product)
    if kind == "inf":
        return                                                                  # (0 * inf = NaN at the one element, 0 elsewhere)
    ref = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
    ref.grad = host.double()
    torch.nn.utils.clip_grad_norm_([ref], max_norm)
    assert int(_ulps(flat, ref.grad.to(torch.float32)).max()) <= 2


def test_coefficient_one_leaves_every_bit(dev):
    """NaN payloads, infinities, denormals and negative zero survive a coefficient of exactly 1; with 3 groups the coefficient
    is taken of all groups together."""
    from refign_amd.steplog import grad_clip_coef, grad_scale_, grad_sqnorm_groups
    n = 2 * 16384 + 7
    flat = _content("normal", n, dev, seed=2)
    raw = flat.view(torch.int32)
    raw[5], raw[6], raw[n - 1], raw[n - 2] = 0x7FC12345, -4194303, -2147483648, 1          # NaNs with payloads, -0.0, a denormal
    flat[9] = float("-inf")
    before = _bits(flat)
    one = torch.tensor([1.0, 0.0], device=dev)
    grad_scale_(flat, one)
    assert torch.equal(_bits(flat), before)
    # three groups: 1 / (sqrt(4 * 1 + 4 * 4 + 4 * 16) + 1e-6)
    flat = torch.cat([torch.full((4,), 1.0), torch.full((4,), 2.0), torch.full((4,), 4.0)]).to(dev)
    plan = _plan([(0, 4, 0), (4, 4, 1), (8, 4, 2)], 3, 12, dev)
    out = torch.zeros(4, dtype=torch.float64, device=dev)
    coef = torch.zeros(2, device=dev)
    grad_sqnorm_groups(flat, plan, out)
    grad_clip_coef(out, 3, 1.0, coef)
    assert out.tolist() == [4.0, 16.0, 64.0, 0.0]
    want = torch.tensor([1.0 / (math.sqrt(84.0) + 1e-6), math.sqrt(84.0)], dtype=torch.float64).to(torch.float32)
    assert int(_ulps(coef, want).max()) <= 1


@pytest.mark.parametrize("v", [0.5, 1e-3])
@pytest.mark.parametrize("n", SIZES)
def test_clamp_is_torch_clamp_bit_for_bit(dev, n, v):
    from refign_amd.steplog import grad_clamp_
    flat = _content("normal", n, dev, seed=3)
    flat[0] = float("nan")
    if n > 2:
        flat[1], flat[n - 1] = float("inf"), float("-inf")
    if n > 4:
        flat[3] = -0.0
    want = torch.clamp(flat, -v, v)
    grad_clamp_(flat, v)
    assert torch.equal(_bits(flat), _bits(want))
    assert math.isnan(float(flat[0])) and int(torch.isnan(flat).sum()) == 1
    assert float(torch.nan_to_num(flat, nan=0.0).abs().max()) <= float(torch.tensor(v, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# kernels: the fused unscale-and-norm
# ---------------------------------------------------------------------------------------------------------------------
N_RAGGED = 2 * 16384 + 7
# offsets with off & 3 = 0, 1, 2, 3; lengths 16384, 5, 1, 0 and a ragged rest; gaps at 16384, 16390 .. 16393, 16395 .. 16398
RAGGED = ((0, 16384, 0), (16385, 5, 1), (16394, 1, 2), (16399, 16376, 1), (20000, 0, 0))


def _chunk_mask(chunks, n):
    m = torch.zeros(n, dtype=torch.bool)
    for off, ln, _ in chunks:
        m[off:off + ln] = True
    return m


@pytest.mark.parametrize("bad", [None, "inf", "nan"])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** 4, 2.0 ** 16])
@pytest.mark.parametrize("G", [1, 3])
def test_fused_unscale_and_norm_equals_the_two_calls(dev, G, scale, bad):
    """Buffer, found_inf and all G + 1 values of out, bit for bit, against rfn_amp_unscale_f32 followed by
    rfn_grad_sqnorm_groups on a copy (gaps zero, as FlatGradBuffer.zero() leaves them)."""
    from refign_amd.amp import LossScaler
    from refign_amd.steplog import grad_sqnorm_groups
    n = N_RAGGED
    chunks = [(o, ln, g % G) for o, ln, g in RAGGED]
    plan = _plan(chunks, G, n, dev)
    flat = _content("normal", n, dev, seed=4) * scale
    flat[~_chunk_mask(chunks, n).to(dev)] = 0.0
    if bad is not None:
        flat[16387] = float(bad)                                                # inside the 5-element chunk at off & 3 = 1
    copy = flat.clone()
    a, b = LossScaler(dev, init_scale=scale), LossScaler(dev, init_scale=scale)
    out_a = torch.full((G + 1,), -1.0, dtype=torch.float64, device=dev)
    out_b = torch.full((G + 1,), -1.0, dtype=torch.float64, device=dev)
    a.unscale_sqnorm_(flat, plan, out_a)
    b.unscale_(copy)
    grad_sqnorm_groups(copy, _plan(chunks, G, n, dev), out_b)
    assert torch.equal(_bits(flat), _bits(copy))
    assert torch.equal(_bits(a.found_inf), _bits(b.found_inf)) and float(a.found_inf) == (0.0 if bad is None else 1.0)
    assert torch.equal(_bits(out_a), _bits(out_b)), (out_a.tolist(), out_b.tolist())
    assert float(out_a[G]) == (0.0 if bad is None else 1.0)
    if bad is None:
        want = sum(float((copy[o:o + ln].double() ** 2).sum()) for o, ln, _ in chunks)
        assert float(out_a[:G].sum()) == pytest.approx(want, rel=1e-12)


def test_fused_unscale_touches_nothing_between_the_chunks(dev):
    from refign_amd.amp import LossScaler
    n = N_RAGGED
    plan = _plan(RAGGED, 3, n, dev)
    inside = _chunk_mask(RAGGED, n).to(dev)
    flat = _content("normal", n, dev, seed=5)
    flat[~inside] = float("nan")                                                # would raise found_inf if it were read
    before = flat.clone()
    sc = LossScaler(dev, init_scale=8.0)
    out = torch.zeros(4, dtype=torch.float64, device=dev)
    sc.unscale_sqnorm_(flat, plan, out)
    assert float(sc.found_inf) == 0.0 and float(out[3]) == 0.0
    assert bool(torch.isnan(flat[~inside]).all()) and int((~inside).sum()) == 9
    assert torch.equal(_bits(flat[inside]), _bits(before[inside] * 0.125))


# ---------------------------------------------------------------------------------------------------------------------
# Trainer: the matcher
# ---------------------------------------------------------------------------------------------------------------------
def _mirror(batch):
    """The batch seen in a mirror: images, mask and flow flipped along W, the flow's x component negated."""
    out = dict(batch)
    for k in ("image_ref", "image_trg", "image_prime", "mask_prime", "flow_prime"):
        out[k] = batch[k].flip(-1).contiguous()
    out["flow_prime"][:, 0].neg_()
    return out


def _norm64(flat):
    return float(flat.detach().double().cpu().norm())


def _adam_state(trainer):
    sd = trainer.optimizer.state_dict()
    return {(i, k): (v.detach().cpu().clone() if torch.is_tensor(v) else v) for i, st in sd["state"].items() for k, v in st.items()}


def _params(model):
    return {k: v.detach().cpu().clone() for k, v in model.named_parameters()}


def _equal_dicts(a, b):
    return a.keys() == b.keys() and all(torch.equal(_bits(a[k]), _bits(b[k])) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


def test_norm_clipping_of_one_matcher_step(dev, z):
    """The buffer's norm afterwards is the threshold to 1e-6 relative (eps / total = 1e-6 / 7e4, plus the coefficient's fp32
    rounding of 6e-8 and the products' roundings, which do not add up); the row holds the norm BEFORE clipping."""
    from refign_amd.trainer import Trainer
    model = build(dev)
    trainer = Trainer(model, gradient_clip_val=CLIP, logger=Memory(), log_every_n_steps=1)
    trainer.step(matcher_batch(z, dev), 0)
    trainer.flush_log()
    norm = _norm64(trainer.grads.flat)
    (step, row), = trainer.log_history
    print(f"\nnorm after clipping {norm!r}; row coef {row['grad_clip/coef']!r} total {row['grad_norm/total']!r}")
    assert abs(norm - CLIP) <= 1e-6 * CLIP
    assert step == 0 and 0.0 < row["grad_clip/coef"] < 1.0
    assert row["grad_norm/total"] > 1e3 * CLIP                                 # 7.3e4 on this batch: the unclipped norm,
    assert row["grad_norm/total"] * row["grad_clip/coef"] == pytest.approx(CLIP, rel=1e-6)    # the one the decision used
    assert all(p.grad.data_ptr() >= trainer.grads.flat.data_ptr() for p in trainer.grads.params)
    assert model.global_step == 1 and trainer.optimizer_stepped is True
    trainer.close()


def test_value_clipping_of_one_matcher_step(dev, z):
    from refign_amd.trainer import Trainer
    v = 1e-2
    model = build(dev)
    trainer = Trainer(model, gradient_clip_val=v, gradient_clip_algorithm="value")
    trainer.step(matcher_batch(z, dev), 0)
    flat = trainer.grads.flat
    lim = float(torch.tensor(v, dtype=torch.float32))
    assert float(flat.abs().max()) == lim and int((flat.abs() == lim).sum()) > 10      # something was clamped, nothing exceeds
    assert bool(torch.isfinite(flat).all()) and model.global_step == 1
    trainer.close()


def test_a_threshold_that_never_clips_changes_no_bit(dev, z):
    """deterministic=True with gradient_clip_val=1e30 against deterministic=True alone (the step as it was): parameters and
    Adam's moments after 2 steps, bit for bit."""
    from refign_amd.trainer import Trainer
    got = []
    for clip in (1e30, None):
        torch.manual_seed(0)
        np.random.seed(0)
        model = build(dev)
        trainer = Trainer(model, deterministic=True, gradient_clip_val=clip)
        batch = matcher_batch(z, dev)
        for it in range(2):
            trainer.step(batch, it)
        if clip is not None:
            assert float(trainer._clip.coef[0]) == 1.0 and float(trainer._clip.coef[1]) > 1e3
        got.append((_params(model), _adam_state(trainer)))
        trainer.close()
    assert any(k[1] == "exp_avg_sq" for k in got[0][1])
    assert _equal_dicts(got[0][0], got[1][0]) and _equal_dicts(got[0][1], got[1][1])


def _hand_windows(dev, batches, windows=2):
    """zero_grad, one (loss / k).backward() per micro-batch, Adam and scheduler step -> the gradient after the FIRST window
    (before anything steps on it) by parameter name, and the logged losses of every call."""
    model = build(dev)
    (opt,), (sch,) = model.configure_optimizers()
    rows, first = [], None
    for _ in range(windows):
        opt.zero_grad()
        for b in batches:
            loss = model.training_step(b, 0)
            (loss / len(batches)).backward()
            rows.append([float(model.logged[k]) for k in LOSSES])
        if first is None:
            first = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        opt.step()
        sch["scheduler"].step()
    return first, np.asarray(rows)


def _rel_l2(a, b):
    num = math.sqrt(sum(float(((a[k].double() - b[k].double()) ** 2).sum()) for k in a))
    return num / math.sqrt(sum(float((b[k].double() ** 2).sum()) for k in a))


def test_accumulation_over_two_different_micro_batches(dev, z):
    """k = 2 over the golden batch and its mirror image.  The gradient after the window against the hand loop's: relative L2
    difference at most max(4 s, 1e-4), s the same difference between two fresh hand-loop runs (the backward adds with
    atomics), 1e-4 the floor test_three_trainer_steps_follow_the_hand_driven_loop uses.  After 2 windows the losses lie
    within that test's bound of the hand loop's."""
    from refign_amd.trainer import Trainer
    batch = matcher_batch(z, dev)
    batches = [batch, _mirror(batch)]
    (ga, rows_a), (gb, rows_b) = _hand_windows(dev, batches), _hand_windows(dev, batches)
    s, spread = _rel_l2(ga, gb), np.abs(rows_a - rows_b)
    model = build(dev)
    trainer = Trainer(model, accumulate_grad_batches=2)
    rows, stepped, grad = [], [], None
    for call in range(4):
        trainer.step(batches[call % 2], call)
        rows.append([float(model.logged[k]) for k in LOSSES])
        stepped.append((trainer.optimizer_stepped, model.global_step))
        if call == 1:
            grad = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
    rows = np.asarray(rows)
    assert grad.keys() == ga.keys()
    d = _rel_l2(grad, ga)
    single = _rel_l2({k: v * 2 for k, v in grad.items()}, ga)                   # what a missing division would give
    bound = np.maximum(4 * spread, 1e-4 * np.abs(rows_a))
    print(f"\ngradient: |trainer - hand| / |hand| = {d:.3e}, between two hand loops s = {s:.3e}, bound {max(4 * s, 1e-4):.3e} "
          f"(an undivided gradient: {single:.3e})\nlosses hand\n{rows_a}\ntrainer\n{rows}\nspread\n{spread}\nbound\n{bound}")
    assert d <= max(4 * s, 1e-4)
    assert not np.allclose(rows_a[0], rows_a[1], rtol=1e-3), "the two micro-batches are one"
    assert np.isfinite(rows).all() and (np.abs(rows - rows_a) <= bound).all()
    assert stepped == [(False, 0), (True, 1), (False, 1), (True, 2)]
    assert trainer.scheduler.last_epoch == 2 and trainer.fast_step.launches == 1     # torch's own first step, then one launch
    trainer.close()


@pytest.mark.parametrize("graph", [False, True])
def test_fp16_accumulated_clipped_window_does_not_synchronise(dev, z, graph):
    """precision=16, k = 2, norm clipping: a whole window under set_sync_debug_mode("error") -- eagerly the second one (calls 3
    and 4), with graph_step the first one after the capture (calls 5 and 6: call 3 captures, which synchronises)."""
    from refign_amd.trainer import Trainer
    model = build(dev)
    trainer = Trainer(model, precision=16, scaler_args={"init_scale": FP16_SCALE}, gradient_clip_val=CLIP,
                      accumulate_grad_batches=2, graph_step=graph)
    batch = matcher_batch(z, dev)
    batch["prime_trg_idx"] = torch.tensor(batch["prime_trg_idx"], device=dev)
    batches = [batch, _mirror(batch)]
    warm = 4 if graph else 2
    for call in range(warm):
        trainer.step(batches[call % 2], call)
    if graph:
        assert trainer.step_graph.captured()
    torch.cuda.synchronize(dev)
    before = {k: v.detach().clone() for k, v in model.alignment_head.named_parameters()}
    launches = trainer.fast_step.launches
    torch.cuda.set_sync_debug_mode("error")
    try:
        trainer.step(batches[0], warm)
        trainer.step(batches[1], warm + 1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert model.global_step == warm // 2 + 1 and trainer.fast_step.launches == launches + 1
    assert trainer.scaler.skipped_steps() == 0
    assert any(not torch.equal(v, before[k]) for k, v in model.alignment_head.named_parameters())
    assert abs(_norm64(trainer.grads.flat) - CLIP) <= 1e-6 * CLIP
    assert all(np.isfinite(float(model.logged[k])) for k in LOSSES)
    trainer.close()


def test_fp16_overflow_skips_the_whole_window_once(dev, z):
    from refign_amd.trainer import Trainer
    model = build(dev, milestones=(1, 100))
    huge = 2.0 ** 100
    trainer = Trainer(model, precision=16, scaler_args={"init_scale": huge}, gradient_clip_val=CLIP, accumulate_grad_batches=2)
    batch = matcher_batch(z, dev)
    batches = [batch, _mirror(batch)]
    p0 = {k: v.detach().clone() for k, v in model.alignment_head.named_parameters()}
    trainer.step(batches[0], 0)
    assert trainer.scaler.get_scale() == huge and model.global_step == 0          # nothing is decided inside the window
    trainer.step(batches[1], 1)
    assert all(torch.equal(v, p0[k]) for k, v in model.alignment_head.named_parameters())
    assert trainer.scaler.get_scale() == huge / 2 and trainer.scaler.skipped_steps() == 1
    assert model.global_step == 1 and trainer.scheduler.last_epoch == 1
    trainer.scaler._scale.fill_(FP16_SCALE)
    for call in (2, 3):
        trainer.step(batches[call % 2], call)
    assert trainer.scaler.skipped_steps() == 1 and model.global_step == 2
    assert any(not torch.equal(v, p0[k]) for k, v in model.alignment_head.named_parameters())
    trainer.close()


def test_deterministic_fp16_accumulated_clipped_runs_repeat(dev, z):
    """deterministic=True, k = 2, norm clipping, precision=16: two fresh runs of 2 windows give the same bits in every loss,
    parameter, moment and the scaler's state; nothing refuses (a refusal raises RuntimeError with RFN_ENONDET's code)."""
    from test_matcher_deterministic_gpu import _assert_same_state, _state
    from refign_amd.trainer import Trainer
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        np.random.seed(0)
        model = build(dev)
        trainer = Trainer(model, deterministic=True, precision=16, scaler_args={"init_scale": FP16_SCALE},
                          gradient_clip_val=CLIP, accumulate_grad_batches=2)
        batch = matcher_batch(z, dev)
        batches, rows = [batch, _mirror(batch)], []
        for call in range(4):
            trainer.step(batches[call % 2], call)
            rows.append([float(model.logged[k]) for k in LOSSES])
        assert float(trainer._clip.coef[0]) < 1.0
        runs.append((rows, _state(model, trainer)))
        trainer.close()
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    _assert_same_state(runs[0][1], runs[1][1], "two deterministic fp16 runs of 2 clipped windows")
    assert runs[0][1]["global_step"] == 2 and float(runs[0][1]["scaler/skipped"]) == 0
    assert np.isfinite(runs[0][0]).all() and runs[0][0][0] != runs[0][0][2]


# ---------------------------------------------------------------------------------------------------------------------
# Trainer: the UDA model, and the defaults
# ---------------------------------------------------------------------------------------------------------------------
def test_uda_step_is_clipped_in_the_proxy(dev):
    from test_resume_gpu import _seed
    from test_step_gpu import build as build_uda
    from test_step_gpu import make_batch
    from refign_amd.trainer import Trainer
    c = 1e-3
    _seed(5)
    uda = build_uda(False, dev)
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        Trainer(uda, precision="bf16", accumulate_grad_batches=2)
    t = Trainer(uda, precision="bf16", gradient_clip_val=c)
    t.step(make_batch(2, 128, 128, 64, dev), 0)
    norm, coef, total = _norm64(t.grads.flat), float(t._clip.coef[0]), float(t._clip.coef[1])
    print(f"\nuda: norm before {total!r}, coefficient {coef!r}, norm after {norm!r}")
    assert coef < 1.0 and total > c
    assert abs(norm - c) <= 1e-6 * c
    assert t.optimizer_stepped is True
    t.close()


def test_defaults_call_none_of_the_new_entry_points(dev, z, monkeypatch):
    from test_resume_gpu import _seed
    from test_step_gpu import build as build_uda
    from test_step_gpu import make_batch
    from refign_amd import _lib
    from refign_amd.trainer import Trainer
    lib = _lib.load_library()
    calls = {}
    for name in NEW_ENTRY_POINTS:
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    _seed(5)
    t = Trainer(build_uda(False, dev), precision="bf16")
    t.step(make_batch(2, 128, 128, 64, dev), 0)
    t.close()
    t = Trainer(build(dev), precision=16, scaler_args={"init_scale": FP16_SCALE}, logger=Memory(), log_every_n_steps=1)
    t.step(matcher_batch(z, dev), 0)
    torch.cuda.synchronize(dev)
    t.close()
    assert calls == {}, calls
    # ... and the wrapping does see them
    t = Trainer(build(dev), precision=16, scaler_args={"init_scale": FP16_SCALE}, gradient_clip_val=CLIP)
    t.step(matcher_batch(z, dev), 0)
    torch.cuda.synchronize(dev)
    t.close()
    assert calls == {"rfn_amp_unscale_sqnorm_groups_f32": 1, "rfn_grad_clip_coef": 1, "rfn_grad_scale_f32": 1}, calls

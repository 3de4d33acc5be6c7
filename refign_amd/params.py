"""Parameter plumbing of the training step, laid out for the flat gradient buffer (trainer.FlatGradBuffer).

Two things autograd + autocast do per parameter per pass, which on a MiT-B5 (1 000 parameters, 4 forward and 3 backward
passes per Refign step) add up to ~7 000 launches of tiny kernels (profiles/r01_step_shapes_elem.txt):
  * autocast re-casts every fp32 weight/bias to bf16 at every use              -> `derived()`: one versioned bf16 copy
    per parameter, re-made only after the parameter changed in place (optimizer step, EMA update, load_state_dict);
  * every weight gradient is materialised, cast to fp32 and added to `.grad`   -> `grad_sink()`: the hand-written
    backward kernels (sum_rows, layernorm_bwd, dwconv3x3_bwd_weight) ACCUMULATE straight into the parameter's view of
    the flat fp32 gradient buffer and return None to autograd.
"""
import numpy as np
import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

from . import _lib
from ._tensor import DTYPE_CODE, ptr, workspace


class _Entry:
    """One cached copy of a parameter: `value` goes to callers, refresh() copies `refill(p)` into `fill` (the value, or the
    parameter-shaped view of a padded value); `epoch`: the parameter's epoch cell when the copy was made (no refill only)."""
    __slots__ = ("value", "fill", "refill", "version", "ptr", "epoch")

    def __init__(self, value, fill, refill, version, ptr, epoch):
        self.value, self.fill, self.refill, self.version, self.ptr, self.epoch = value, fill, refill, version, ptr, epoch


def _epoch(d):
    cell = d.get("_rfn_epoch")
    return None if cell is None else cell[0]


def _capturing(t):
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def derived(p, key, fn, refill=None):
    """fn(p.detach()) cached on the parameter, recomputed when p was modified in place or re-allocated.  Two kinds of entry:
      * `refill(p.detach())` given -- a VIEW of the parameter with the cached tensor's shape: refresh() updates the cached
        tensor in place with one multi-tensor copy (dtype / layout conversions), so captured graphs keep pointing at live
        values.  fn may return (value, fill_target) where callers get a padded buffer and refresh() fills a view of it.
      * no refill -- valid until the next refresh() of a set that holds the parameter, then re-made on use; in no plan.
        Inside a stream capture it is computed but not kept (a tensor allocated there holds no data until the first
        replay), and a kept one of a refreshed set is not used (the next refresh gives up the tensor the graph points at)."""
    d = p.__dict__
    cache = d.setdefault("_rfn_derived", {})
    ent = cache.get(key)
    if ent is not None and ent.version == p._version and ent.ptr == p.data_ptr():
        if ent.refill is not None:
            return ent.value
        epoch = _epoch(d)
        if ent.epoch == epoch and (epoch is None or not _capturing(ent.value)):
            return ent.value
    with torch.no_grad():
        value = fn(p.detach())
    value, fill = value if isinstance(value, tuple) else (value, value)
    if refill is not None:
        _GENERATION[0] += 1                            # cached refresh plans are stale
    elif _capturing(value):
        return value
    cache[key] = _Entry(value, fill, refill, p._version, p.data_ptr(), _epoch(d))
    return value


def entries(p):
    """(key, tensor, refill) of every cached copy of `p` that stands: `tensor` is the one refresh() fills (refill given), or
    the cached value (refill None)."""
    d = p.__dict__
    for key, ent in d.get("_rfn_derived", {}).items():
        if ent.refill is not None or (ent.version == p._version and ent.ptr == p.data_ptr() and ent.epoch == _epoch(d)):
            yield key, ent.fill, ent.refill


def forget(plan_key):
    """Drop what refresh() and ema_update() keep for one named parameter set."""
    _PLANS.pop(plan_key, None)
    _EMA_TABLES.pop(plan_key, None)


_GENERATION = [0]        # bumped whenever an entry WITH a refill view is created, replaced or dropped
_PLANS = {}              # plan key -> what refresh() does for one fixed parameter set (see refresh)
_EMA_TABLES = {}         # plan key -> chunk table of ema_update


def _table(rows, dev):
    return torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev), len(rows)


def chunk_rows(n, chunk):
    """(offset, count) of every `chunk`-element piece of an n-element tensor: one row each in the multi-tensor kernels' tables."""
    return [(off, min(chunk, n - off)) for off in range(0, n, chunk)]


def _identity(t):
    return t


def _build_plan(params):
    """One pass over the parameters' caches: which cached tensors are re-filled from which views of their parameter; entries
    without a refill view are dropped.  The views alias the parameters' storage, so the same (dst, src) lists serve every later
    refresh of this parameter set for as long as no refillable entry is created or dropped and no parameter is re-allocated."""
    entries, dst, src = [], [], []
    for p in params:
        cache = p.__dict__.get("_rfn_derived", {})
        for key in list(cache):
            ent = cache[key]
            if ent.refill is None:
                del cache[key]
                continue
            if ent.ptr == p.data_ptr():
                v = ent.refill(p.detach())
                if v.shape == ent.fill.shape:
                    dst.append(ent.fill)
                    src.append(v)
                    ent.version = p._version
                    entries.append((cache, key, p))
                    continue
            del cache[key]
            _GENERATION[0] += 1
    skip = set()

    def launches(idx, make_table, by_dtype=True):
        """One table per device (and copy dtype) over the pairs `idx`, from 4 pairs on; fewer stay with the per-tensor copies.
        (The tensors are kept next to the table: they own the memory the table points into.)"""
        if len(idx) < 4:
            return []
        skip.update(idx)
        groups = {}
        for i in idx:
            groups.setdefault((dst[i].device, dst[i].dtype if by_dtype else None), []).append(i)
        return [make_table([dst[i] for i in g], [src[i] for i in g], dev) + (dev, [dst[i] for i in g], [src[i] for i in g])
                for (dev, _), g in groups.items()]

    # plain fp32 -> bf16 / fp16 casts of contiguous tensors: ONE launch of the multi-tensor cast kernel per device and dtype
    # (csrc/reduce.hip); torch._foreach_copy_ with a dtype change is one tiny kernel per tensor
    casts = launches([i for i, (d, s_) in enumerate(zip(dst, src))
                      if d.is_cuda and d.dtype in _CAST16 and s_.dtype == torch.float32 and d.is_contiguous()
                      and s_.is_contiguous() and d.numel() == s_.numel() and d.numel() > 0], _cast_table)
    # transposed 16-bit copies (W^T of the Linear weights): one launch of the tile-transpose kernel instead of one strided
    # copy per tensor
    transposes = launches([i for i, (d, s_) in enumerate(zip(dst, src))
                           if i not in skip and d.is_cuda and d.dtype in _CAST16 and s_.dtype == torch.float32 and d.dim() == 2
                           and d.is_contiguous() and s_.dim() == 2 and s_.t().is_contiguous() and s_.numel() > 0], _transpose_table)
    # every other layout-changing copy of an fp32 parameter view into a contiguous <= 4-D tensor: one launch
    # (csrc/reduce.hip multi_permute_cast_kernel) instead of one strided-copy kernel per tensor
    permutes = launches([i for i, (d, s_) in enumerate(zip(dst, src))
                         if i not in skip and d.is_cuda and d.is_contiguous() and d.dtype in DTYPE_CODE and s_.dtype == torch.float32
                         and 1 <= d.dim() <= 4 and d.numel() > 0 and s_.shape == d.shape], _permute_table, by_dtype=False)
    return {"entries": entries, "casts": casts, "transposes": transposes, "permutes": permutes,
            "rest": ([d for i, d in enumerate(dst) if i not in skip], [s_ for i, s_ in enumerate(src) if i not in skip]),
            "gen": _GENERATION[0]}


# 16-bit copy dtype -> (multi-tensor cast, multi-tensor transpose + cast) entry points of csrc/reduce.hip
_CAST16 = {torch.bfloat16: ("rfn_multi_cast_f32_bf16", "rfn_multi_transpose_cast_f32_bf16"),
           torch.float16: ("rfn_multi_cast_f32_f16", "rfn_multi_transpose_cast_f32_f16")}


def _permute_table(dst, src, dev):
    """Chunk table of the multi-tensor layout-changing copy: 12 int64 per chunk (csrc/reduce.hip PermChunk), built once."""
    chunk = _lib.load_library().rfn_multi_permute_chunk_elems()
    rows = []
    for d, s_ in zip(dst, src):
        shape = [1] * (4 - d.dim()) + list(d.shape)
        strides = [0] * (4 - d.dim()) + list(s_.stride())
        n = d.numel()
        assert n < 2 ** 31, "the permute kernel indexes one tensor with 32 bits"
        rows += [(s_.data_ptr(), d.data_ptr(), shape[1], shape[2], shape[3], strides[0], strides[1], strides[2], strides[3],
                  off, cnt, DTYPE_CODE[d.dtype]) for off, cnt in chunk_rows(n, chunk)]
    return _table(rows, dev)


def _cast_table(dst, src, dev):
    """Chunk table of the multi-tensor fp32 -> bf16 / fp16 cast kernel (one dst dtype per table): {src*, dst*, n}, 24 bytes per chunk, built once."""
    chunk = _lib.load_library().rfn_multi_cast_chunk_elems()
    rows = []
    for s_, d in zip(src, dst):
        sp, dp = s_.data_ptr(), d.data_ptr()
        rows += [(sp + 4 * off, dp + 2 * off, cnt) for off, cnt in chunk_rows(s_.numel(), chunk)]
    return _table(rows, dev)


def _transpose_table(dst, src, dev):
    """Tile table of the multi-tensor transpose + cast kernel: src views are (K, N) transposes of contiguous (N, K)
    fp32 parameters, dst the contiguous (K, N) bf16 or fp16 copies (one dtype per table)."""
    rows = []
    T = _lib.load_library().rfn_multi_transpose_tile()
    for s_, d in zip(src, dst):
        K, N = s_.shape                                   # view (K, N) of a parameter stored (N, K)
        sp, dp = s_.data_ptr(), d.data_ptr()
        for n0 in range(0, N, T):
            for k0 in range(0, K, T):
                rows.append((sp, dp, N | (K << 32), n0 | (k0 << 32)))
    return _table(rows, dev)


def _multi_cast(table, nrows, dev, dtype=torch.bfloat16):
    _lib.call(_CAST16[dtype][0], dev, ptr(table), nrows)


def _optimizer_step_post_hook(optimizer, args, kwargs):
    refresh((p for g in optimizer.param_groups for p in g["params"]), plan_key=("optimizer", id(optimizer)))


register_optimizer_step_post_hook(_optimizer_step_post_hook)


def refresh(params, plan_key=None):
    """Bring the cached copies of `params` up to date after the parameters were updated in place by something that
    does not bump their version counters (fused / foreach optimizers, EMA updates through `.data`): copies with a
    refill view are re-filled with ONE multi-tensor cast launch + one multi-tensor copy, every other derived tensor is
    invalid from here on and re-made on next use.  Called by an optimizer-step post hook (every torch optimizer) and by
    the EMA update.  `plan_key`: callers that refresh the SAME parameter set every step name it; the (dst, src) lists are
    then built once (walking 1 000 parameters and building their views costs ~3 ms of host time per call) and reused
    until a refillable entry is created / dropped or a parameter moves.  The parameters of a planned set share an epoch
    cell (`_rfn_epoch`; one from another set is kept): bumping the set's cells ends its entries without a refill."""
    plan = _PLANS.get(plan_key) if plan_key is not None else None
    if plan is not None and plan["gen"] == _GENERATION[0]:
        ents = plan["entries"]
        # the parameters of a set are updated (and moved) together: the first and the last entry tell whether the
        # version stamps need a pass and whether the storage is still where the plan's views point
        probe = [(c.get(k), p) for c, k, p in ((ents[0], ents[-1]) if ents else ())]
        if any(e is None or e.ptr != p.data_ptr() for e, p in probe):
            plan = None                                # parameter re-allocated or entry gone: rebuild
        elif any(e.version != p._version for e, p in probe):
            for cache, key, p in ents:
                ent = cache.get(key)
                if ent is not None:
                    ent.version = p._version
    else:
        plan = None
    if plan is None:
        params = list(params)
        plan = _build_plan(params)                     # (drops the entries without a refill itself)
        if plan_key is not None:
            shared = [0]                                # (a parameter that has a cell from another set keeps it)
            cells = [p.__dict__.setdefault("_rfn_epoch", shared) for p in params]
            plan["cells"] = list({id(c): c for c in cells}.values())
            if len(_PLANS) >= 8:
                _PLANS.clear()
            _PLANS[plan_key] = plan
    else:
        for cell in plan["cells"]:
            cell[0] += 1
    with torch.no_grad():
        for table, nrows, dev, dsts, _ in plan["casts"]:
            _multi_cast(table, nrows, dev, dsts[0].dtype)
        for table, ntiles, dev, dsts, _ in plan["transposes"]:
            _lib.call(_CAST16[dsts[0].dtype][1], dev, ptr(table), ntiles)
        for table, nrows, dev, _, _ in plan["permutes"]:
            _lib.call("rfn_multi_permute_cast_f32", dev, ptr(table), nrows)
        if plan["rest"][0]:
            torch._foreach_copy_(*plan["rest"])


def ema_update(ema_params, live_params, momentum, plan_key):
    """ema <- momentum * ema + (1 - momentum) * live over two aligned parameter lists (segmentation_model.py:676-689) as
    ONE kernel launch (csrc/reduce.hip: rfn_multi_ema_f32) from a chunk table that is built once per parameter set,
    then refresh() of the teacher's cached copies.  Falls back to two multi-tensor torch ops off the GPU.
    The kernel's second coefficient is float32(1) - float32(momentum); the reference and the torch branch below multiply by
    float32(1 - momentum) -- for momentum 0.999 the two are 1.29e-5 apart relatively."""
    ema_params, live_params = list(ema_params), list(live_params)
    if not ema_params:
        return
    dev = ema_params[0].device
    if dev.type == "cuda" and all(p.dtype == torch.float32 and p.is_contiguous() for p in ema_params + live_params):
        sig = (len(ema_params), ema_params[0].data_ptr(), ema_params[-1].data_ptr(), live_params[0].data_ptr(),
               live_params[-1].data_ptr())
        ent = _EMA_TABLES.get(plan_key)
        lib = _lib.load_library()
        if ent is None or ent[0] != sig:
            chunk = lib.rfn_multi_cast_chunk_elems()
            rows = []
            for e, l_ in zip(ema_params, live_params):
                ep, lp = e.data_ptr(), l_.data_ptr()
                rows += [(ep + 4 * off, lp + 4 * off, 0, cnt) for off, cnt in chunk_rows(e.numel(), chunk)]
            ent = _EMA_TABLES[plan_key] = (sig,) + _table(rows, dev)
        _lib.call("rfn_multi_ema_f32", dev, ptr(ent[1]), ent[2], float(momentum))
    else:
        ema, live = [p.data for p in ema_params], [p.data for p in live_params]
        torch._foreach_mul_(ema, momentum)
        torch._foreach_add_(ema, live, alpha=1.0 - momentum)
    refresh(ema_params, plan_key=plan_key)


def as_dtype(p, dtype):
    """`p` in the compute dtype (None stays None): the parameter itself if it already has it, else the cached copy."""
    if p is None or p.dtype == dtype:
        return p
    return derived(p, dtype, lambda t: t.to(dtype), _identity)


def _t_view(t):
    return t.reshape(t.shape[0], -1).t()              # (N, K) or (N, K, 1, 1) -> (K, N) view


def transposed(p, dtype):
    """Contiguous transposed copy W^T (K, N) of a Linear weight (N, K) in the compute dtype: the B operand of the
    input-gradient GEMM dx = dy W run as an NT product (csrc/mfma_gemm.hip).  Cached like the plain 16-bit copy and
    re-filled in place after optimizer / EMA updates."""
    return derived(p, ("T", dtype), lambda t: t.reshape(t.shape[0], -1).to(dtype).t().contiguous(), _t_view)


# Named layouts of a convolution weight (N, C, KH, KW).  Each function owns its key and its build / refill pair, so every
# user of a layout shares one entry per parameter and dtype.
def nhwc_view(t):
    return t.permute(0, 2, 3, 1)


def _krsc_view(t):
    return t.permute(2, 3, 1, 0)


def patch_linear(p, dtype):
    """(Co, ry, rx, c) copy: the weight of a kernel == stride convolution as a Linear over (ry, rx, c) patch rows."""
    return derived(p, (dtype, "patch_linear"), lambda t: nhwc_view(t.to(dtype)).contiguous(), nhwc_view)


def patch_linear_t(p, dtype):
    """(ry, rx, c, Co) copy: the transpose of patch_linear, the B operand of the patch Linear's input-gradient GEMM."""
    return derived(p, (dtype, "patch_linear_T"), lambda t: _krsc_view(t.to(dtype)).contiguous(), _krsc_view)


def channels_last(p, dtype):
    """The weight in the compute dtype with channels-last strides: what the library wants next to channels-last activations."""
    return derived(p, (dtype, "channels_last"), lambda t: t.to(dtype).contiguous(memory_format=torch.channels_last), _identity)


def _tap_view(t):
    return t.reshape(t.shape[0], 9).t()


def tap_major_f32(p):
    """(9, C) tap-major fp32 copy of a depthwise 3x3 weight (C, 1, 3, 3)."""
    return derived(p, "tap_major_f32", lambda t: _tap_view(t.float()).contiguous(), _tap_view)


def _stacked(params, key, alloc, slot, views):
    """ONE buffer shared by the cached copies of several parameters: entry `key` of params[i] hands out the buffer and is
    re-filled, by refresh() like every other entry with a refill view, through slot(buffer, i) <- views[i](params[i]).  The first
    parameter's entry owns the allocation (alloc(p)); an entry that points at an older buffer is re-made into the current one."""
    base = None
    for i, p in enumerate(params):
        def make(t, i=i):
            buf = alloc(t) if base is None else base
            fill = slot(buf, i)
            fill.copy_(views[i](t))
            return buf, fill
        got = derived(p, key, make, views[i])
        if base is not None and got is not base:
            p.__dict__["_rfn_derived"].pop(key, None)
            _GENERATION[0] += 1
            got = derived(p, key, make, views[i])
        if base is None:
            base = got
    return base


def _tap_block_view(box, transpose):
    y0, y1, x0, x1 = box

    def view(t):                                       # (K, C, 3, 3) -> (ny, nx, K, C), or (C, ny, nx, K)
        s = t[:, :, y0:y1, x0:x1]
        return s.permute(1, 2, 3, 0) if transpose else s.permute(2, 3, 0, 1)
    return view


def tap_stack(weights, dtype, live, n_pad, rows, transpose=False):
    """The live taps of several 3x3 convolution weights (K, C, 3, 3) stacked into one zero-padded matrix in `dtype`: `live`
    gives per weight the (y0, y1, x0, x1) box of its taps that are kept, tap-major in (weight, ky, kx) order, K padded to
    `n_pad` per tap, `rows` rows in all -> (rows, C), the W operand of the DeepLabV2 tap-GEMM (csrc/aspp.hip); `transpose`:
    its (C, rows) transpose, the W operand of the data-gradient GEMM.  One buffer, one refill view per weight."""
    C = weights[0].shape[1]
    starts, t = [], 0
    for y0, y1, x0, x1 in live:
        starts.append(t)
        t += (y1 - y0) * (x1 - x0)

    def slot(buf, i):
        y0, y1, x0, x1 = live[i]
        ny, nx, K = y1 - y0, x1 - x0, weights[i].shape[0]
        a, b = starts[i] * n_pad, (starts[i] + ny * nx) * n_pad
        if transpose:
            return buf[:, a:b].view(C, ny, nx, n_pad)[..., :K]
        return buf[a:b].view(ny, nx, n_pad, C)[:, :, :K]

    return _stacked(weights, ("tap_stack_T" if transpose else "tap_stack", dtype, tuple(live), n_pad, rows),
                    lambda p: torch.zeros((C, rows) if transpose else (rows, C), dtype=dtype, device=p.device), slot,
                    [_tap_block_view(box, transpose) for box in live])


def bias_stack(biases, n_pad):
    """(R, n_pad) fp32 rows of R bias vectors, zero padded: what rfn_aspp_tapsum adds in row order."""
    return _stacked(biases, ("bias_stack", len(biases), n_pad),
                    lambda p: torch.zeros((len(biases), n_pad), dtype=torch.float32, device=p.device),
                    lambda buf, i: buf[i, :biases[i].shape[0]], [_identity] * len(biases))


def compute_dtype(x):
    """dtype the dense ops run in: the autocast dtype inside an autocast region, else x's."""
    if x.is_cuda and torch.is_autocast_enabled("cuda"):
        return torch.get_autocast_dtype("cuda")
    return x.dtype


def mark_grad_sink(p):
    """FlatGradBuffer: `p.grad` is a persistent, contiguous fp32 view that kernels may accumulate into directly."""
    p._rfn_grad_sink = True


def grad_sink(p):
    if p is None or not getattr(p, "_rfn_grad_sink", False):
        return None
    g = p.grad                 # looked up every time: zero_grad(set_to_none=True) or a foreign p.grad must be seen
    if g is None or g.dtype != torch.float32 or not g.is_cuda:
        return None
    return g


def sum_rows(x, out=None, accumulate=False):
    """out[n] (+)= sum over the leading dim of a contiguous (S, n) fp32 / bf16 / fp16 matrix, fp32 result (csrc/reduce.hip)."""
    S, n = x.shape
    if not x.is_cuda or n % 8 != 0 or x.dtype not in DTYPE_CODE or not x.is_contiguous():
        r = x.sum(0, dtype=torch.float32)
        if out is None:
            return r
        return out.add_(r) if accumulate else out.copy_(r)
    if out is None:
        out, accumulate = torch.empty(n, dtype=torch.float32, device=x.device), False
    lib = _lib.load_library()
    nb = lib.rfn_sum_rows_workspace_bytes(S, n)
    ws = workspace(nb, x.device)
    _lib.call("rfn_sum_rows", x.device, ptr(x), ptr(out), ptr(ws), S, n, DTYPE_CODE[x.dtype], 1 if accumulate else 0)
    return out


def linear_param_grads(g2, part, gb_out, gw_out):
    """One Linear's parameter gradients, accumulated in place: gb_out (N) += column sum of g2 (T, N);
    gw_out (N*K) += sum over the leading dim of part (S, N*K).  Two launches (csrc/reduce.hip).  Returns False when
    the shapes are outside the fused kernel's domain (caller falls back to two sum_rows calls)."""
    T, N = g2.shape
    S, NK = part.shape
    if not (g2.is_cuda and g2.dtype == part.dtype and g2.dtype in DTYPE_CODE and T > 64 and S <= 64 and N % 8 == 0
            and NK % 8 == 0 and g2.is_contiguous() and part.is_contiguous()):
        return False
    lib = _lib.load_library()
    ws = workspace(lib.rfn_sum_rows_workspace_bytes(T, N), g2.device)
    _lib.call("rfn_linear_param_grads", g2.device, ptr(g2), ptr(gb_out), ptr(ws), T, N, 1, ptr(part), ptr(gw_out), S, NK, 1,
              DTYPE_CODE[g2.dtype])
    return True

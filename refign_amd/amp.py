"""Loss scaling of the fp16 recipe: what `--trainer.precision 16` gives the reference (Lightning's native AMP, a
torch.amp.GradScaler around a non-fused torch.optim.AdamW), with every decision taken on the device.

torch's GradScaler reads `found_inf` on the host in every `step()` to decide whether to call the optimizer.  Here the
scale, the found-inf flag and the growth tracker are device tensors, and the three kernels of csrc/reduce.hip run in
stream order with no host synchronisation:
  unscale_   g *= 1 / scale over the flat gradient buffer, found_inf = 1 if any gradient is inf / NaN
             (unscale_sqnorm_: the same with the squared norms per optimizer group from the same pass, csrc/steplog.hip);
  (AdamW)    optim.MultiTensorAdamW.step_amp: the update is a no-op when found_inf is set (step count on the device);
  update     backoff on inf, growth after `growth_interval` clean steps (torch._amp_update_scale_).
`state_dict()` / `load_state_dict()` speak GradScaler's format, so a Lightning checkpoint's `native_amp_scaling_state`
round-trips."""
import torch

from . import _lib
from ._tensor import ptr


class LossScaler:
    def __init__(self, device, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        if not (growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and int(growth_interval) > 0 and init_scale > 0):
            raise ValueError("LossScaler: need growth_factor > 1, 0 < backoff_factor < 1, growth_interval > 0, init_scale > 0")
        self.device = torch.device(device)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), \
            int(growth_interval)
        self._scale = torch.full((1,), float(init_scale), dtype=torch.float32, device=self.device)
        self._growth_tracker = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.found_inf = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._skipped = torch.zeros(1, dtype=torch.float32, device=self.device)     # diagnostics: steps skipped so far

    def scale(self, loss):
        """loss * scale, read from the device buffer when the pass runs (a replayed capture sees the current scale)."""
        return loss * self._scale

    def unscale_(self, grads):
        """In place on a flat fp32 gradient buffer: grads *= 1 / scale; found_inf <- any gradient inf or NaN."""
        if not (grads.is_cuda and grads.dtype == torch.float32 and grads.is_contiguous() and grads.data_ptr() % 16 == 0):
            raise RuntimeError("LossScaler.unscale_: a contiguous, 16-byte aligned fp32 CUDA buffer is required")
        self.found_inf.zero_()
        _lib.call("rfn_amp_unscale_f32", grads.device, ptr(grads), grads.numel(), ptr(self._scale), ptr(self.found_inf))

    def unscale_sqnorm_(self, grads, plan, out):
        """unscale_ and steplog.grad_sqnorm_groups(grads, plan, out) in ONE pass over the buffer, bit-equal to the two calls one
        after the other (norm clipping decides on the unscaled gradient's norm: steplog.GradClip).  Only the chunks of `plan`
        are touched: what lies between them must be the zero-filled alignment gaps of a trainer.FlatGradBuffer."""
        if not (grads.is_cuda and grads.dtype == torch.float32 and grads.is_contiguous() and grads.data_ptr() % 16 == 0):
            raise RuntimeError("LossScaler.unscale_sqnorm_: a contiguous, 16-byte aligned fp32 CUDA buffer is required")
        if grads.numel() != plan.numel or grads.device != plan.device or not plan.chunks:
            raise RuntimeError("LossScaler.unscale_sqnorm_: the plan was made for another buffer, or is empty")
        if out.dtype != torch.float64 or out.numel() != plan.ngroups + 1 or not out.is_contiguous() or out.device != grads.device:
            raise RuntimeError("LossScaler.unscale_sqnorm_: out must hold G + 1 contiguous fp64 values on the buffer's device")
        self.found_inf.zero_()
        _lib.call("rfn_amp_unscale_sqnorm_groups_f32", grads.device, ptr(grads), grads.numel(), ptr(plan.table), len(plan.chunks),
                  plan.ngroups, ptr(self._scale), ptr(self.found_inf), ptr(plan.partials), ptr(out))

    def update(self, optimizer_step=None):
        """After the optimizer: new scale from found_inf; `optimizer_step` (a device float tensor of the optimizer's step
        count, or None) is advanced by one when the step was taken."""
        with torch.no_grad():
            self._skipped.add_(self.found_inf)
        _lib.call("rfn_amp_update_scale", self.device, ptr(self._scale), ptr(self._growth_tracker), ptr(self.found_inf),
                  ptr(optimizer_step), self.growth_factor, self.backoff_factor, self.growth_interval)

    # --- host-side reads (each synchronises) ---------------------------------------------------------------------------
    def get_scale(self):
        return float(self._scale.item())

    def skipped_steps(self):
        return int(self._skipped.item())

    def state_dict(self):
        return {"scale": self.get_scale(), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(self._growth_tracker.item())}

    def load_state_dict(self, state_dict):
        if not state_dict:
            raise RuntimeError("LossScaler.load_state_dict: empty state (a checkpoint saved without loss scaling)")
        self._scale.fill_(float(state_dict["scale"]))
        self.growth_factor = float(state_dict["growth_factor"])
        self.backoff_factor = float(state_dict["backoff_factor"])
        self.growth_interval = int(state_dict["growth_interval"])
        self._growth_tracker.fill_(int(state_dict["_growth_tracker"]))


# Trainer(precision=...): accepted values -> autocast dtype name ("32": no autocast; None: the caller's autocast)
PRECISIONS = {16: "16", "16": "16", "16-mixed": "16", "bf16": "bf16", "bf16-mixed": "bf16", 32: "32", "32": "32"}


def parse_precision(precision):
    if precision is None:
        return None
    if isinstance(precision, bool) or not isinstance(precision, (int, str)) or precision not in PRECISIONS:
        raise ValueError(f"Trainer: precision must be None, 16, '16', '16-mixed', 'bf16', 'bf16-mixed' or 32 "
                         f"(got {precision!r})")
    return PRECISIONS[precision]

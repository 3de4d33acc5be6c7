"""AdamW step of the whole model as ONE kernel launch (csrc/reduce.hip: rfn_multi_adamw_f32).

The reference instantiates `torch.optim.AdamW` from its YAML (`optimizer:` section) and Lightning steps it; here the
torch optimizer object stays the owner of everything a checkpoint holds -- param_groups, `state[p]['exp_avg' |
'exp_avg_sq' | 'step']`, the LR scheduler writes `group['lr']` as always -- and only the arithmetic of `step()` moves:
torch's fused implementation needs ~4 ms of host time per step to regroup 1 090 tensors into 33 multi-tensor launches
(measured, profiles/r02_step_phases_events.txt); a chunk table built once makes it one launch.  torch performs the FIRST
step itself (it creates the state exactly as it would), and any configuration outside plain AdamW (amsgrad, maximize,
non-fp32 / non-CUDA parameters, gradients that are not where the table expects them) stays on torch's step."""
import math

import numpy as np
import torch

from . import _lib
from ._tensor import ptr
from .params import chunk_rows, refresh


class MultiTensorAdamW:
    TORCH_CLASS = torch.optim.AdamW                        # exactly this class, no subclass
    ENTRY, ENTRY_AMP = "rfn_multi_adamw_f32", "rfn_multi_adamw_amp_f32"
    DECOUPLED = True                                       # p -= lr wd p

    def __init__(self, optimizer):
        self.opt = optimizer
        self._table = None
        self._sig = None
        self._steps = None
        self._t = 0
        self._synced_t = 0
        self._params = None
        self._dev_step = None                              # step count on the device (step_amp: the host does not know it)
        self.launches = 0                                  # diagnostics / tests
        # state['step'] of the 1 000 parameters is brought up to date when somebody looks (checkpoint, torch's own step)
        optimizer.register_state_dict_pre_hook(lambda opt: self._sync_steps())
        # load_state_dict REPLACES every state tensor (mid-run resume / rollback): the chunk table would keep pointing at
        # the freed moment buffers and the kernel's own step counter would ignore the loaded one -- drop everything, the
        # next step() rebuilds from the loaded state
        optimizer.register_load_state_dict_post_hook(lambda opt: self._reset())

    def _reset(self):
        self._table = self._sig = self._steps = self._params = self._dev_step = None
        self._t = self._synced_t = 0

    def _sync_steps(self):
        if self._dev_step is not None:
            if self._steps is not None:
                with torch.no_grad():
                    for s in self._steps:
                        s.copy_(self._dev_step[0])
            return
        if self._steps is not None and self._synced_t != self._t:
            with torch.no_grad():
                torch._foreach_add_(self._steps, float(self._t - self._synced_t))
            self._synced_t = self._t

    def _plain(self):
        if type(self.opt) is not self.TORCH_CLASS or len(self.opt.param_groups) > 8:
            return False
        for g in self.opt.param_groups:
            if g.get("amsgrad") or g.get("maximize") or g.get("differentiable") or torch.is_tensor(g["lr"]):
                return False
            if bool(g.get("decoupled_weight_decay", self.DECOUPLED)) != self.DECOUPLED:
                return False                                # (torch.optim.Adam(decoupled_weight_decay=True) is AdamW's arithmetic)
            for p in g["params"]:
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad is not None
                        and p.grad.dtype == torch.float32 and p.grad.is_contiguous()):
                    return False
        return True

    def _signature(self):
        ps = self._params
        if ps is None or len(ps) != sum(len(g["params"]) for g in self.opt.param_groups):
            ps = self._params = [p for g in self.opt.param_groups for p in g["params"]]
        g0, g1 = ps[0].grad, ps[-1].grad
        # ... and where the first and the last parameter's first moments live: replaced state is seen even without the hook
        m0, m1 = (self.opt.state.get(p, {}).get("exp_avg") for p in (ps[0], ps[-1]))
        return (len(ps), ps[0].data_ptr(), ps[-1].data_ptr(), None if g0 is None else g0.data_ptr(),
                None if g1 is None else g1.data_ptr(), None if m0 is None else m0.data_ptr(),
                None if m1 is None else m1.data_ptr(),
                tuple((g.get("amsgrad"), g.get("maximize"), torch.is_tensor(g["lr"])) for g in self.opt.param_groups))

    def _build(self):
        lib = _lib.load_library()
        chunk = lib.rfn_multi_cast_chunk_elems()
        rows, steps, t = [], [], None
        for gi, g in enumerate(self.opt.param_groups):
            for p in g["params"]:
                st = self.opt.state.get(p)
                if not st or "exp_avg" not in st or not torch.is_tensor(st.get("step")):
                    return False                            # state not created yet (or a foreign layout): torch steps
                m, v = st["exp_avg"], st["exp_avg_sq"]
                if not (m.dtype == torch.float32 and v.dtype == torch.float32 and m.is_contiguous() and v.is_contiguous()):
                    return False
                steps.append(st["step"])
                pp, gp, mp, vp = p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr()
                rows += [(pp + 4 * o, gp + 4 * o, mp + 4 * o, vp + 4 * o, cnt | (gi << 56))
                         for o, cnt in chunk_rows(p.numel(), chunk)]
        ts = {float(s) for s in steps[:1] + steps[-1:]}
        if len(ts) != 1:
            return False
        self._t = self._synced_t = int(ts.pop())
        dev = self.opt.param_groups[0]["params"][0].device
        self._table = (self._upload(torch.from_numpy(np.asarray(rows, dtype=np.int64)), dev), len(rows), dev)
        self._steps = steps
        self._sig = self._signature()
        return True

    @staticmethod
    def _upload(host, dev):
        return host.to(dev)

    def _updated(self):
        """The parameters changed under torch's feet (no version counter moved): cached copies follow."""
        refresh((p for g in self.opt.param_groups for p in g["params"]), plan_key=("optimizer", id(self.opt)))

    def step(self):
        sig = self._signature()
        if self._table is None or sig != self._sig:         # first call, or parameters / gradients / flags changed
            self._sync_steps()
            self._table = None
            if not (self._plain() and self._build()):
                return self.opt.step()                      # torch's own step (it also creates the state on step 1)
        self._t += 1
        t = self._t
        args = []
        for g in self.opt.param_groups:
            b1, b2 = g["betas"]
            args += [float(g["lr"]), b1, b2, float(g["eps"]), float(g["weight_decay"]), 1.0 - b1 ** t,
                     math.sqrt(1.0 - b2 ** t), 1.0 - b1, 1.0 - b2]
        host = np.asarray(args, dtype=np.float32)
        table, n, dev = self._table
        with torch.no_grad():
            _lib.call(self.ENTRY, dev, ptr(table), n, host.ctypes.data, len(self.opt.param_groups))
        self.launches += 1
        self.opt._opt_called = True                        # what Optimizer.step's wrapper tells the LR scheduler
        self._updated()

    def step_amp(self, found_inf):
        """The step under loss scaling (amp.LossScaler): the same update, skipped on the device when `found_inf` is set.
        The step count lives on the device (`device_step`, advanced by LossScaler.update when the step was taken); the
        torch state's `step` tensors are brought up to date from it when somebody looks.  Returns False where it declines
        (first step, configuration outside the plain optimizer): the caller then steps torch's optimizer itself."""
        sig = self._signature()
        if self._table is None or sig != self._sig:
            self._sync_steps()
            self._table = self._dev_step = None
            if not (self._plain() and self._build()):
                return False
        if self._dev_step is None:
            self._dev_step = torch.full((1,), float(self._t), dtype=torch.float32, device=self._table[2])
        args = []
        for g in self.opt.param_groups:
            b1, b2 = g["betas"]
            args += [float(g["lr"]), b1, b2, float(g["eps"]), float(g["weight_decay"]), 1.0 - b1, 1.0 - b2]
        host = np.asarray(args, dtype=np.float64)
        table, n, dev = self._table
        with torch.no_grad():
            _lib.call(self.ENTRY_AMP, dev, ptr(table), n, host.ctypes.data, len(self.opt.param_groups),
                      ptr(found_inf), ptr(self._dev_step))
        self.launches += 1
        self.opt._opt_called = True
        self._updated()
        return True

    @property
    def device_step(self):
        return self._dev_step


class MultiTensorAdam(MultiTensorAdamW):
    """torch.optim.Adam -- weight decay as an L2 term of the gradient, `g += wd p`, the optimizer of the matcher's configs --
    as one launch (rfn_multi_adam_f32 / rfn_multi_adam_amp_f32: the same kernels, templated on the decay form).  Same chunk
    table, same hand-over rules, same step() / step_amp(found_inf) / device_step as MultiTensorAdamW."""
    TORCH_CLASS = torch.optim.Adam
    ENTRY, ENTRY_AMP = "rfn_multi_adam_f32", "rfn_multi_adam_amp_f32"
    DECOUPLED = False                                      # g += wd p

    @staticmethod
    def _upload(host, dev):
        """Through pinned memory, without waiting: the table is built in the SECOND step of a run (torch takes the first),
        and the matcher's step asks the host nothing after its first call."""
        return host.pin_memory().to(dev, non_blocking=True)

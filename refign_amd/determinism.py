"""Deterministic mode: the one switch the Python wrappers consult when they choose a kernel form.

`Trainer(deterministic=True)` holds it for the life of the trainer (`acquire()` at the end of the constructor, `release()` in
`close()`); tests use the `deterministic()` context manager.  Both kinds of request meet in one place (`_apply`): the mode is what
the innermost open `with deterministic(on):` block says, and outside any block it is on while at least one holder remains.  So a
trainer closed inside a `with deterministic():` block leaves the block's mode alone, and `with deterministic(False):` around code
of a live deterministic trainer switches the mode off for that block -- a test's tool, not something a training loop does.
The state proper is the library's process-wide flag (`rfn_set_deterministic` / `rfn_get_deterministic`, include/refign_hip.h):
while it is set, every entry point that adds with floating-point atomics returns RFN_ENONDET, so a wrapper that forgot to ask
`enabled()` raises instead of drifting.  A Python mirror of the flag keeps `enabled()` off the ctypes path (it sits in front of
~1 000 launches per step).

`scatter_forms` widens the mode (`acquire(scatter_forms=True)`, `deterministic(scatter_forms=True)`, `scatter_forms()`): see there.
It follows the same rule: what the innermost block says, and outside blocks on while a holder that asked for it remains.

`torch_deterministic()` is the span of one training step: torch's own switch on (ATen ops without a deterministic form raise),
MIOpen's deterministic algorithms, and `fill_uninitialized_memory` off -- that one is a debugging aid which puts a fill launch
behind every `torch.empty`.
"""
import contextlib

import torch

from . import _lib

_ENABLED = False
_SCATTER = False


def enabled():
    return _ENABLED


def scatter_forms():
    """The widening of the mode: with it, the two scatter backwards the plain mode refuses (matching.warp, the generic fp32
    correlation) take their order-free forms (rfn_warp_bwd_det_f32, rfn_corr_bwd_gather_f32).  A deterministic Trainer of the
    matcher asks for it; the plain mode keeps refusing them -- the UDA step never differentiates through a warp, and the refusal
    is the tripwire of its audit."""
    return _ENABLED and _SCATTER


_HOLDERS = 0            # open deterministic trainers
_SCATTER_HOLDERS = 0    # ... of them, those that asked for the scatter forms
_BLOCKS = []            # (on, scatter_forms) of every open `with deterministic(...):` block, innermost last


def _apply():
    """Bring the library's flag and its mirror to what the requests say."""
    global _ENABLED, _SCATTER
    on, _SCATTER = _BLOCKS[-1] if _BLOCKS else (_HOLDERS > 0, _SCATTER_HOLDERS > 0)
    if on != _ENABLED:
        _lib.check(_lib.load_library().rfn_set_deterministic(1 if on else 0), "set_deterministic")
        _ENABLED = on


def acquire(scatter_forms=False):
    """A long-lived holder of the mode (a Trainer): on until the last holder has released it.  `scatter_forms`: the holder asks
    for the widening too (release it with the same argument)."""
    global _HOLDERS, _SCATTER_HOLDERS
    _HOLDERS += 1
    _SCATTER_HOLDERS += 1 if scatter_forms else 0
    _apply()


def release(scatter_forms=False):
    global _HOLDERS, _SCATTER_HOLDERS
    _HOLDERS = max(0, _HOLDERS - 1)
    _SCATTER_HOLDERS = min(_HOLDERS, max(0, _SCATTER_HOLDERS - (1 if scatter_forms else 0)))
    _apply()


@contextlib.contextmanager
def deterministic(on=True, scatter_forms=False):
    """`with deterministic():` -- nests, and restores the state it found.  The widening is what the innermost block says."""
    _BLOCKS.append((bool(on), bool(on) and bool(scatter_forms)))
    try:
        _apply()
        yield
    finally:
        _BLOCKS.pop()
        _apply()


@contextlib.contextmanager
def torch_switch_suspended():
    """torch's switch off around ONE op that torch refuses wholesale although the call at hand cannot depend on order (the
    caller says why).  No-op when the switch is off."""
    if not torch.are_deterministic_algorithms_enabled():
        yield
        return
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(False)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(True, warn_only=warn)


@contextlib.contextmanager
def torch_deterministic(on=True):
    """torch's side of the mode for the duration of a block (no-op with on=False)."""
    if not on:
        yield
        return
    prev_algo = torch.are_deterministic_algorithms_enabled()
    prev_warn = torch.is_deterministic_algorithms_warn_only_enabled()
    prev_cudnn = torch.backends.cudnn.deterministic
    prev_fill = torch.utils.deterministic.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True)
    torch.backends.cudnn.deterministic = True
    torch.utils.deterministic.fill_uninitialized_memory = False
    try:
        yield
    finally:
        torch.utils.deterministic.fill_uninitialized_memory = prev_fill
        torch.backends.cudnn.deterministic = prev_cudnn
        torch.use_deterministic_algorithms(prev_algo, warn_only=prev_warn)

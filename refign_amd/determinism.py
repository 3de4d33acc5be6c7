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

`torch_deterministic()` is the span of one training step: torch's own switch on (ATen ops without a deterministic form raise),
MIOpen's deterministic algorithms, and `fill_uninitialized_memory` off -- that one is a debugging aid which puts a fill launch
behind every `torch.empty`.
"""
import contextlib

import torch

from . import _lib

_ENABLED = False


def enabled():
    return _ENABLED


_HOLDERS = 0            # open deterministic trainers
_BLOCKS = []            # the `on` of every open `with deterministic(on):` block, innermost last


def _apply():
    """Bring the library's flag and its mirror to what the requests say."""
    global _ENABLED
    on = _BLOCKS[-1] if _BLOCKS else _HOLDERS > 0
    if on != _ENABLED:
        _lib.check(_lib.load_library().rfn_set_deterministic(1 if on else 0), "set_deterministic")
        _ENABLED = on


def acquire():
    """A long-lived holder of the mode (a Trainer): on until the last holder has released it."""
    global _HOLDERS
    _HOLDERS += 1
    _apply()


def release():
    global _HOLDERS
    _HOLDERS = max(0, _HOLDERS - 1)
    _apply()


@contextlib.contextmanager
def deterministic(on=True):
    """`with deterministic():` -- nests, and restores the state it found."""
    _BLOCKS.append(bool(on))
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

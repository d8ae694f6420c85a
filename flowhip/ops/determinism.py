"""Deterministic mode: an opt-in switch under which one training step
(forward, backward, optimizer update) repeats bit for bit on one GPU.

The default kernels sum in a few places with float atomics, whose order the
hardware picks (csrc/col_sum.hip, csrc/instance_norm.hip at column widths
below 32, the flow gradient of csrc/convex_upsample.hip). With the mode on,
the autograd Functions and `nn/norm.py` pass `deterministic=True` to those
bindings, which then run atomics-free kernels whose summation order is fixed
by indices alone. Paths without such a kernel step aside to torch (PAC) or
raise (the `fmap2` gradient of the on-demand correlation lookup).

The convolutions that stay on torch (the baseline's mask head among them)
need torch's own switch: MIOpen's backward-weights solvers sum with atomics
unless `torch.backends.cudnn.deterministic` is set, so the mode sets it and
puts the earlier value back when it is turned off.

The mode is read where an op is dispatched, never inside csrc/.
FLOWHIP_DETERMINISTIC=1 sets the initial value, so scripts run in the mode
without being edited.
"""

import contextlib
import os

import torch

_DETERMINISTIC = False
_TORCH_CONV_PREV = None  # torch.backends.cudnn.deterministic before the mode


def set_deterministic(flag):
    global _DETERMINISTIC, _TORCH_CONV_PREV
    _DETERMINISTIC = bool(flag)
    if _DETERMINISTIC:
        if _TORCH_CONV_PREV is None:
            _TORCH_CONV_PREV = bool(torch.backends.cudnn.deterministic)
        torch.backends.cudnn.deterministic = True
    elif _TORCH_CONV_PREV is not None:
        torch.backends.cudnn.deterministic = _TORCH_CONV_PREV
        _TORCH_CONV_PREV = None


def deterministic_enabled():
    return _DETERMINISTIC


@contextlib.contextmanager
def deterministic(flag=True):
    """Run the body with the mode set to `flag`; the previous value comes
    back on exit, also when the body raises."""
    prev = deterministic_enabled()
    set_deterministic(flag)
    try:
        yield
    finally:
        set_deterministic(prev)


set_deterministic(os.environ.get("FLOWHIP_DETERMINISTIC", "0") == "1")

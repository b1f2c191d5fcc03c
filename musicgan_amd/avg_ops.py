"""Tensor-level wrapper over mg_adam_step_dev_ema of the C ABI (include/musicgan_hip.h, csrc/elementwise.hip): the fused Adam
step that keeps an exponential running average of the weights in the same pass.  The call is asynchronous on the caller's current
stream and allocates nothing on the device.  No fallback path exists: non-GPU tensors raise."""
from __future__ import annotations

import ctypes
from typing import Sequence

import torch

from . import _lib
from ._lib import AdamTensorDevEma, check
from .ops import _chk_typed, _s


def ema_weight(decay: float) -> float:
    """host arithmetic: 1 - decay, formed in float64 and rounded once to float32 -- the scalar the kernel receives"""
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"0 <= decay < 1 expected, got {decay!r}")
    return ctypes.c_float(1.0 - float(decay)).value


def adam_step_ema(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], exp_avg: Sequence[torch.Tensor],
                  exp_avg_sq: Sequence[torch.Tensor], steps: Sequence[torch.Tensor], ema: Sequence[torch.Tensor], *, lr: float,
                  beta1: float, beta2: float, eps: float, grad_scale: float = 1.0, decay: float) -> None:
    """One Adam update (torch.optim.Adam's arithmetic, as mg_adam_step_dev) of every params[i] from grads[i] * grad_scale, and
    ema[i] += (params[i] - ema[i]) * (1 - decay) on the new values, in one launch per 48 tensors plus its counter tick.  Writes all of
    params[i], exp_avg[i], exp_avg_sq[i], ema[i] (float32, one size per i) and steps[i] (one int32 on the device: the number of
    updates so far, advanced by one); reads grads[i]."""
    lists = (params, grads, exp_avg, exp_avg_sq, steps, ema)
    if len(params) < 1 or any(len(x) != len(params) for x in lists):
        raise ValueError(f"six non-empty lists of one length expected, got lengths {[len(x) for x in lists]}")
    for x in (params, grads, exp_avg, exp_avg_sq, ema):
        _chk_typed("adam_step_ema", *x)
    _chk_typed("adam_step_ema", *steps, dtype=torch.int32)
    for i, p in enumerate(params):
        if any(x[i].numel() != p.numel() for x in (grads, exp_avg, exp_avg_sq, ema)) or steps[i].numel() != 1:
            raise ValueError(f"adam_step_ema: tensor {i}: {p.numel()} elements expected in grad, moments and average, one in the step")
        if any(x[i].device != p.device for x in lists):
            raise ValueError(f"adam_step_ema: tensor {i}: all six tensors must be on one device")
    weight = ema_weight(decay)
    recs = (AdamTensorDevEma * len(params))(*[
        AdamTensorDevEma(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), s.data_ptr(), e.data_ptr())
        for p, g, m, v, s, e in zip(*lists)])   # host records; the library hands them to the kernel by value
    with torch.cuda.device(params[0].device):
        check(_lib.load().mg_adam_step_dev_ema(ctypes.cast(recs, ctypes.c_void_p), len(params), lr, beta1, beta2, eps,
                                               float(grad_scale), weight, _s()), "mg_adam_step_dev_ema")

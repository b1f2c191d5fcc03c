"""Tensor-level wrapper over the mg_pyramid_l2 entries of the C ABI (include/musicgan_hip.h, csrc/pyrloss.hip): the multi-scale L2
loss between two (N, C, H, W) float32 batches with its gradient (definition: DESIGN.md 4.16).  Two launches, asynchronous on the
caller's current stream; nothing is read back, so a call can be captured.  No fallback path exists: non-GPU tensors raise."""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check
from .ops import _chk_typed, _p, _s, workspace

MAX_LEVELS = 7   # PL_MAX_LEVELS of csrc/pyrloss_plan.h


def default_levels(h: int, w: int) -> int:
    """min(7, 1 + log2 of the largest power of two dividing both sides): the deepest pyramid the image takes"""
    g = math.gcd(int(h), int(w))
    return min(MAX_LEVELS, (g & -g).bit_length())


def check_weights(h: int, w: int, weights=None, levels: Optional[int] = None) -> Tuple[float, ...]:
    """The level weights lambda_0 .. lambda_{L-1} as a tuple of floats.  weights=None: 1 / L each, over `levels` levels (None: the
    default depth of an h x w image).  ValueError for no level or more than 7, a side that is no multiple of 2^(L-1), a count that
    disagrees with `levels`, or a weight that is not a finite number >= 0."""
    if weights is None:
        n = default_levels(h, w) if levels is None else levels
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_LEVELS:
            raise ValueError(f"pyramid_l2: levels must be an integer in 1 .. {MAX_LEVELS}, got {levels!r}")
        lam = (1.0 / n,) * n
    else:
        try:
            lam = tuple(float(v) for v in weights)
        except (TypeError, ValueError):
            raise ValueError(f"pyramid_l2: weights must be a sequence of numbers, got {weights!r}")
        if not 1 <= len(lam) <= MAX_LEVELS or (levels is not None and levels != len(lam)):
            raise ValueError(f"pyramid_l2: 1 .. {MAX_LEVELS} weights expected"
                             + (f" ({levels} levels asked for)" if levels is not None else "") + f", got {len(lam)}")
        if any(not (math.isfinite(v) and v >= 0.0) for v in lam):
            raise ValueError(f"pyramid_l2: weights must be finite and >= 0, got {lam}")
    g = 1 << (len(lam) - 1)
    if h % g or w % g:
        raise ValueError(f"pyramid_l2: {len(lam)} levels need sides that are multiples of {g}, got {h} x {w}")
    return lam


def pyramid_l2_ws_bytes(n: int, c: int, h: int, w: int, levels: int) -> int:
    """bytes of workspace one call takes (0: the library refuses the shape)"""
    return int(_lib.load().mg_pyramid_l2_ws_bytes(int(n), int(c), int(h), int(w), int(levels)))


def pyramid_l2(x: torch.Tensor, t: torch.Tensor, weights: Optional[Sequence[float]] = None, *, need_grad: bool = True,
               out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """x, t (N, C, H, W) -> (loss (N,) float64, grad (N, C, H, W) float32 = d loss[n] / d x, or None with need_grad=False).
    weights: lambda_0 .. lambda_{L-1} (None: the deepest pyramid the sides take, 1 / L each).  `out` (optional) receives all of the
    gradient; it must not overlap x or t, which may be one tensor."""
    what = "pyramid_l2"
    if not isinstance(x, torch.Tensor) or not isinstance(t, torch.Tensor):
        raise _lib.MusicGanHipError(f"{what}: tensors on a ROCm GPU expected (no CPU fallback)")
    _chk_typed(what, x, t)
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{what}: a non-empty (N, C, H, W) batch expected, got {tuple(x.shape)}")
    if t.shape != x.shape or t.device != x.device:
        raise ValueError(f"{what}: t must be {tuple(x.shape)} on {x.device}, got {tuple(t.shape)} on {t.device}")
    n, c, h, w = x.shape
    lam = check_weights(h, w, weights)
    grad = None
    if need_grad:
        grad = torch.empty_like(x) if out is None else out
        _chk_typed(what, grad)
        if grad.shape != x.shape or grad.device != x.device:
            raise ValueError(f"{what}: out must be {tuple(x.shape)} on {x.device}, got {tuple(grad.shape)} on {grad.device}")
    elif out is not None:
        raise ValueError(f"{what}: out given with need_grad=False")
    nbytes = pyramid_l2_ws_bytes(n, c, h, w, len(lam))
    if nbytes == 0:
        raise ValueError(f"{what}: {tuple(x.shape)} with {len(lam)} levels is more than one launch takes")
    loss = torch.empty(n, dtype=torch.float64, device=x.device)
    ws = workspace(nbytes, x.device)
    lam_c = (ctypes.c_float * len(lam))(*lam)
    check(_lib.load().mg_pyramid_l2(_p(x), _p(t), n, c, h, w, len(lam), lam_c, _p(loss), _p(grad), _p(ws), nbytes, _s()),
          "mg_pyramid_l2")
    return loss, grad

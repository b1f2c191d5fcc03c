"""Multi-scale L2 reconstruction loss as a module: the per-sample loss of musicgan_amd/proj_ops.py (definition: DESIGN.md 4.16; kernels:
csrc/pyrloss.hip), differentiable with respect to its first argument."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import ops, proj_ops


class _PyramidL2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, weights):
        need = ctx.needs_input_grad[0]
        loss, g = proj_ops.pyramid_l2(x.detach().contiguous(), t.detach().contiguous(), weights, need_grad=need)
        ctx.g = g   # the gradient comes out of the launch that reads x and t: nothing else is kept
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss):
        if ctx.g is None:
            return None, None, None
        # d loss[n] / d x scaled by the upstream value of sample n, rounded to float32 once (ctx.g stays: a retained graph may come back)
        return ops.scale_per_sample(ctx.g, g_loss.to(torch.float32).contiguous()), None, None


class PyramidL2(nn.Module):
    """`weights`: lambda_0 .. lambda_{L-1}; None: 1 / L each over `levels` levels (None: the deepest pyramid the images take, at most
    7).  forward(x, t) -> (N,) float64; the gradient flows to x alone."""

    def __init__(self, levels: Optional[int] = None, weights: Optional[Sequence[float]] = None):
        super().__init__()
        side = 1 << (proj_ops.MAX_LEVELS - 1)   # a side every depth takes: the values are checked here, an image's sides per call
        lam = proj_ops.check_weights(side, side, weights, levels) if weights is not None or levels is not None else None
        self.levels = levels
        self.weights = None if weights is None else lam

    def forward(self, x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        lam = proj_ops.check_weights(x.shape[-2], x.shape[-1], self.weights, self.levels) if x.dim() == 4 else self.weights
        return _PyramidL2Fn.apply(x, t, lam)

    def extra_repr(self) -> str:
        return f"levels={self.levels}, weights={self.weights}"

"""DiffAugment (Zhao et al. 2020) for the training step: one random translation and one random cutout per sample, applied to every
image the critic sees -- real and generated, in both updates -- with the generator's gradient flowing back through it (definition:
DESIGN.md 4.13; kernels: csrc/diffaug.hip through musicgan_amd/aug_ops.py)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from .. import aug_ops


class _DiffAugFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u, ops, p):
        ctx.save_for_backward(u)
        ctx.spec = (ops, p)
        return aug_ops.diffaug_fwd(x.contiguous(), u, ops, p)

    @staticmethod
    @once_differentiable   # nothing in training differentiates twice through T: a second differentiation raises
    def backward(ctx, gy):
        (u,) = ctx.saved_tensors
        return aug_ops.diffaug_bwd(gy.contiguous(), u, *ctx.spec), None, None, None


class DiffAugment:
    """`policy`: a comma-separated subset of translation, cutout; `p`: the probability with which each of them is applied to a
    sample.  Construction validates the arguments and touches no device."""

    def __init__(self, policy: str = "translation,cutout", p: float = 1.0):
        self.ops = aug_ops.parse_policy(policy)
        self.p = aug_ops.check_p(p)
        self.policy = ",".join(k for k, bit in aug_ops.OPS.items() if self.ops & bit)

    @property
    def spec(self) -> Tuple[int, float]:
        """(ops bit mask, p): hashable, what a captured graph of an augmented update depends on"""
        return (self.ops, self.p)

    def draw(self, n: int, device, generator: Optional[torch.Generator] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """u (n, 8) float32 uniform in [0, 1) on `device`, the random numbers of n samples (into `out` if given)"""
        shape = (n, aug_ops.U_COLUMNS)
        if out is not None and tuple(out.shape) != shape:
            raise ValueError(f"out must be {shape}, got {tuple(out.shape)}")
        return torch.rand(shape, device=device, generator=generator, out=out)

    def __call__(self, x: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
        """T x, differentiable with respect to x (the backward pass is aug_ops.diffaug_bwd)"""
        return _DiffAugFn.apply(x, u, self.ops, self.p)

    def __repr__(self) -> str:
        return f"DiffAugment(policy={self.policy!r}, p={self.p})"

"""Tensor-level wrappers over mg_slerp_pairs and mg_rows_sqdist of the C ABI (include/musicgan_hip.h, csrc/ppl.hip): two points a step
`eps` apart on the arc between two latents, pair by pair, and the scaled squared distance of two row sets, row by row, in float64 --
what metrics.PPL is made of.  Every call is asynchronous on the caller's current stream and reads nothing back;
neither kernel needs scratch memory.  Shapes and values are checked on the host, before the library is loaded and before any
tensor's device is looked at.  No fallback path exists: non-GPU tensors raise."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .ops import _chk_typed, _p, _s

MAX_NUMEL = 1 << 38   # numbers of one operand of a launch


def _rows(what: str, name: str, t) -> tuple:
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or min(t.shape) < 1:
        raise ValueError(f"{what}: {name}: non-empty rows (n, d) expected, got {tuple(t.shape) if isinstance(t, torch.Tensor) else t!r}")
    if t.numel() >= MAX_NUMEL:
        raise ValueError(f"{what}: {name}: fewer than {MAX_NUMEL} numbers expected, got {tuple(t.shape)}")
    return tuple(t.shape)


def _number(what: str, name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{what}: {name}: a finite number expected, got {v!r}")
    return float(v)


def slerp_pairs(z0: torch.Tensor, z1: torch.Tensor, t: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """z0, z1 (n, d) float32, t (n,) float64, any d >= 1 -> (za, zb, flag): za[i] = slerp(z0[i], z1[i], t[i]) and zb[i] = slerp(z0[i],
    z1[i], t[i] + eps), (n, d) float32, with slerp the definition of project.slerp (float64 arithmetic on each row as one flat vector,
    the straight line below an angle of 1e-6, one rounding to float32; t[i] = 0 returns z0[i] bit for bit), and flag (n,) int32: 1
    where the angle is within 1e-6 of pi -- project.slerp raises there; here za[i] and zb[i] are zeros and the caller leaves the pair
    out --, else 0.  Every element of the three is written.  The float64 sums behind the angle run in an order that d alone fixes:
    a pair's outputs do not depend on n or on the other pairs, and are the same bits in every run."""
    (n, d), shape1 = _rows("slerp_pairs", "z0", z0), _rows("slerp_pairs", "z1", z1)
    if shape1 != (n, d):
        raise ValueError(f"slerp_pairs: two sets of rows of one shape expected, got {(n, d)} and {shape1}")
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != (n,):
        raise ValueError(f"slerp_pairs: t ({n},) expected, got {tuple(t.shape) if isinstance(t, torch.Tensor) else t!r}")
    eps = _number("slerp_pairs", "eps", eps)
    _chk_typed("slerp_pairs", z0, z1)
    _chk_typed("slerp_pairs", t, dtype=torch.float64)
    za = torch.empty((n, d), dtype=torch.float32, device=z0.device)
    zb = torch.empty((n, d), dtype=torch.float32, device=z0.device)
    flag = torch.empty((n,), dtype=torch.int32, device=z0.device)
    check(_lib.load().mg_slerp_pairs(_p(z0), _p(z1), _p(t), n, d, eps, _p(za), _p(zb), _p(flag), _s()), "mg_slerp_pairs")
    return za, zb, flag


def rows_sqdist(a: torch.Tensor, b: torch.Tensor, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a, b (n, d) float32 -> out (n,) float64, every element written:
        out[i] = scale * the sum over j of (float64(a[i, j]) - float64(b[i, j])) ** 2,
    one wave per pair in an order that d alone fixes: out[i] is a function of its two rows, d and scale, the same bits for any n and
    in every run; exactly 0 for equal finite rows; a NaN or an infinity stays in its pair.  Returns out."""
    (n, d), shape1 = _rows("rows_sqdist", "a", a), _rows("rows_sqdist", "b", b)
    if shape1 != (n, d):
        raise ValueError(f"rows_sqdist: two sets of rows of one shape expected, got {(n, d)} and {shape1}")
    scale = _number("rows_sqdist", "scale", scale)
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (n,)):
        raise ValueError(f"rows_sqdist: out ({n},) expected")
    _chk_typed("rows_sqdist", a, b)
    if out is None:
        out = torch.empty((n,), dtype=torch.float64, device=a.device)
    _chk_typed("rows_sqdist", out, dtype=torch.float64)
    check(_lib.load().mg_rows_sqdist(_p(a), _p(b), n, d, scale, _p(out), _s()), "mg_rows_sqdist")
    return out

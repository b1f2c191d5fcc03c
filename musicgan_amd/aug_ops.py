"""Tensor-level wrappers over the mg_diffaug_* entries of the C ABI (include/musicgan_hip.h, csrc/diffaug.hip): DiffAugment's random
translation and cutout, T, and the adjoint, T^t, on (N, C, H, W) float32 images (definition: DESIGN.md 4.13).  The random numbers u
(N, 8) stay on the device and are read by the kernel: a call reads nothing back, is asynchronous on the caller's current stream and can
be captured, and a captured call follows whatever u holds when it is replayed.  One launch each.  No fallback path exists: non-GPU
tensors raise."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import MG_DIFFAUG_CUTOUT, MG_DIFFAUG_TRANSLATION, check
from .ops import _chk_typed, _p, _s

OPS = {"translation": MG_DIFFAUG_TRANSLATION, "cutout": MG_DIFFAUG_CUTOUT}
U_COLUMNS = 8   # per sample: translation on/off, dy, dx, cutout on/off, centre row, centre column, two reserved


def parse_policy(policy: str) -> int:
    """'translation,cutout' -> the MG_DIFFAUG_* bit mask; ValueError for an empty list, an unknown name or a name given twice."""
    if not isinstance(policy, str):
        raise ValueError(f"a comma-separated subset of {','.join(OPS)} expected, got {policy!r}")
    names = [t.strip() for t in policy.split(",")]
    if not policy.strip() or any(n not in OPS for n in names) or len(set(names)) != len(names):
        raise ValueError(f"a comma-separated subset of {','.join(OPS)} expected, each name once, got {policy!r}")
    mask = 0
    for n in names:
        mask |= OPS[n]
    return mask


def check_p(p) -> float:
    """the probability as a float; ValueError unless 0 <= p <= 1 (NaN included)"""
    try:
        v = float(p)
    except (TypeError, ValueError):
        raise ValueError(f"a probability in [0, 1] expected, got {p!r}")
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"a probability in [0, 1] expected, got {p!r}")
    return v


def _args(what: str, x: torch.Tensor, u: torch.Tensor, ops: int, p: float, out: Optional[torch.Tensor]):
    if not isinstance(x, torch.Tensor) or not isinstance(u, torch.Tensor):
        raise _lib.MusicGanHipError(f"{what}: tensors on a ROCm GPU expected (no CPU fallback)")
    _chk_typed(what, x, u)
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{what}: a non-empty (N, C, H, W) batch expected, got {tuple(x.shape)}")
    if tuple(u.shape) != (x.shape[0], U_COLUMNS) or u.device != x.device:
        raise ValueError(f"{what}: u must be ({x.shape[0]}, {U_COLUMNS}) on {x.device}, got {tuple(u.shape)} on {u.device}")
    if not isinstance(ops, int) or ops & ~(MG_DIFFAUG_TRANSLATION | MG_DIFFAUG_CUTOUT):
        raise ValueError(f"{what}: ops must be a mask of MG_DIFFAUG_TRANSLATION | MG_DIFFAUG_CUTOUT, got {ops!r}")
    p = check_p(p)
    if out is None:
        out = torch.empty_like(x)
    _chk_typed(what, out)
    if out.shape != x.shape or out.device != x.device:
        raise ValueError(f"{what}: out must be {tuple(x.shape)} on {x.device}, got {tuple(out.shape)} on {out.device}")
    return p, out


def diffaug_fwd(x: torch.Tensor, u: torch.Tensor, ops: int, p: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (N, C, H, W), u (N, 8) -> all of out = T x.  `out` must not overlap x (the library refuses it)."""
    p, out = _args("diffaug_fwd", x, u, ops, p, out)
    n, c, h, w = x.shape
    check(_lib.load().mg_diffaug_fwd(_p(x), _p(u), n, c, h, w, ops, p, _p(out), _s()), "mg_diffaug_fwd")
    return out


def diffaug_bwd(gy: torch.Tensor, u: torch.Tensor, ops: int, p: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gy (N, C, H, W), u (N, 8) -> all of out = T^t gy, the gradient of <T x, gy> with respect to x."""
    p, out = _args("diffaug_bwd", gy, u, ops, p, out)
    n, c, h, w = gy.shape
    check(_lib.load().mg_diffaug_bwd(_p(gy), _p(u), n, c, h, w, ops, p, _p(out), _s()), "mg_diffaug_bwd")
    return out


def diffaug_decode(u_cpu, h: int, w: int, ops: int, p: float) -> np.ndarray:
    """HOST: u (N, 8) float32 in host memory (numpy or a CPU tensor) -> (N, 6) int32 rows of dy, dx, y0, y1, x0, x1, through the
    function the kernels call.  T x[i, j] = x[i - dy, j - dx]; rows [y0, y1) x columns [x0, x1) are zeroed (all 0: no box)."""
    if isinstance(u_cpu, torch.Tensor):
        if u_cpu.is_cuda:
            raise _lib.MusicGanHipError("diffaug_decode: u in host memory expected (the kernels decode on the device themselves)")
        u_cpu = u_cpu.numpy()
    u_np = np.ascontiguousarray(u_cpu, dtype=np.float32)
    if u_np.ndim != 2 or u_np.shape[1] != U_COLUMNS or u_np.shape[0] < 1:
        raise ValueError(f"diffaug_decode: u must be (N, {U_COLUMNS}), got {u_np.shape}")
    out = np.empty((u_np.shape[0], 6), dtype=np.int32)
    check(_lib.load().mg_diffaug_decode(u_np.ctypes.data_as(ctypes.c_void_p), u_np.shape[0], int(h), int(w), int(ops), check_p(p),
                                        out.ctypes.data_as(ctypes.c_void_p)), "mg_diffaug_decode")
    return out

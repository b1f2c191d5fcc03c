"""Tensor-level wrapper over `mg_input_transform_windows` (include/musicgan_hip.h, csrc/intransform.hip): the training loop's input
transform -- per-plane min / max, range (-1, 1), antialiased bilinear resize -- on windows cut out of a dataset that lives in device
memory.  Window n is, for both channels and every row, columns [off[n], W) of source[rows_a[n]] followed by columns [0, off[n]) of
source[rows_b[n]]; the result is bit for bit `ops.input_transform` of that window laid out in memory.  The three index arrays are
int32 DEVICE tensors: the call reads nothing back and uploads nothing, so it is asynchronous on the caller's current stream and can be
captured.  The kernels trust the indices; `check_windows` validates them on the host, before whoever built them uploads them (an
epoch's arrays at once: audio.dataset.ResidentLoader).  Scratch memory comes from `ops.workspace`.  No fallback path exists:
non-GPU tensors raise."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .ops import _p, _s


def check_windows(rows_a, rows_b, offsets, rows: int, width: int) -> None:
    """ValueError unless 0 <= rows_a < rows, 0 <= offsets < width and, wherever offsets > 0, 0 <= rows_b < rows (rows_b is not read
    where offsets == 0 and may hold anything there).  Host arrays (numpy or CPU tensors) of one length; nothing touches the device."""
    a, b, o = (np.asarray(v) for v in (rows_a, rows_b, offsets))
    if not (a.ndim == b.ndim == o.ndim == 1 and a.shape == b.shape == o.shape):
        raise ValueError(f"rows_a, rows_b and offsets must be vectors of one length, got {a.shape}, {b.shape}, {o.shape}")
    if any(v.dtype.kind not in "iu" for v in (a, b, o)):
        raise ValueError("rows_a, rows_b and offsets must be integer arrays")
    if a.size and (a.min() < 0 or a.max() >= rows):
        raise ValueError(f"rows_a must lie in [0, {rows}), got [{a.min()}, {a.max()}]")
    if o.size and (o.min() < 0 or o.max() >= width):
        raise ValueError(f"offsets must lie in [0, {width}), got [{o.min()}, {o.max()}]")
    used = b[o > 0]
    if used.size and (used.min() < 0 or used.max() >= rows):
        raise ValueError(f"rows_b must lie in [0, {rows}) wherever the offset is positive, got [{used.min()}, {used.max()}]")


def input_transform_windows(source: torch.Tensor, rows_a: torch.Tensor, rows_b: torch.Tensor, offsets: torch.Tensor, side: int,
                            eps: float = 1e-8) -> torch.Tensor:
    """source (R, 2, H, W) float32 contiguous, rows_a / rows_b / offsets int32 (N,) on source's device -> (N, 2, side, side) float32.
    Two launches.  The indices are NOT checked here (that would be a read-back per batch): see `check_windows`."""
    if not isinstance(source, torch.Tensor) or not source.is_cuda:
        raise _lib.MusicGanHipError("input_transform_windows: tensors on a ROCm GPU expected (no CPU fallback)")
    if source.dim() != 4 or source.shape[1] != 2 or source.dtype != torch.float32 or not source.is_contiguous():
        raise _lib.MusicGanHipError(f"input_transform_windows: contiguous float32 (R, 2, H, W) expected, got {source.dtype} "
                                    f"{tuple(source.shape)}")
    n = rows_a.numel()
    for name, t in (("rows_a", rows_a), ("rows_b", rows_b), ("offsets", offsets)):
        if t.device != source.device or t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
            raise _lib.MusicGanHipError(f"input_transform_windows: {name} must be a contiguous int32 vector of {n} entries on "
                                        f"{source.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    rows, _, h, w = source.shape
    if rows == 0 or n == 0:
        raise ValueError("input_transform_windows: an empty source or batch")
    out = torch.empty((n, 2, side, side), dtype=torch.float32, device=source.device)
    lib = _lib.load()
    nbytes = int(lib.mg_input_transform_windows_ws_bytes(n, h, w, side))
    ws = ops.workspace(nbytes, source.device)
    check(lib.mg_input_transform_windows(_p(source), rows, _p(rows_a), _p(rows_b), _p(offsets), _p(out), _p(ws), ws.numel(),
                                         n, h, w, side, eps, _s()), "mg_input_transform_windows")
    return out

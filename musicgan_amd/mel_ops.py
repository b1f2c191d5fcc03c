"""Tensor-level wrappers over mg_logmel_rows and mg_moments of the C ABI (include/musicgan_hip.h, csrc/logmel.hip, csrc/moments.hip):
the log-mel feature rows of a batch of magnitude images and the float64 mean and covariance of a set of rows -- what metrics.LogMel
and metrics.Frechet are made of.  Every call is asynchronous on the caller's current stream and reads nothing back; scratch memory
(the partial sums of the moments) is allocated here with torch.empty, call by call.  Shapes are checked on the host, before any
tensor's device is looked at.  No fallback path exists: non-GPU tensors raise."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .ops import _chk_typed, _p, _s

MAX_BANDS = 256      # band limits go to the kernel by value
MAX_POOL = 1024      # columns of one pool
MAX_D = 4096         # numbers per row moments takes
MAX_N = 1 << 24      # rows moments takes


def _limits(name: str, v, bands: int) -> torch.Tensor:
    if not isinstance(v, torch.Tensor) or v.is_cuda or v.dtype != torch.int32 or tuple(v.shape) != (bands,):
        raise ValueError(f"logmel_rows: {name}: a host int32 tensor ({bands},) expected")
    return v.contiguous()


def logmel_rows(x: torch.Tensor, c: int, scale: torch.Tensor, weight: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, floor: float,
                pools: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (N, C, H, W) float32, rows = frequency and columns = time, its channel c; scale (H,) and weight (M, H) float32 on x's
    device; lo, hi (M,) int32 HOST tensors with 0 <= lo <= hi <= H (they are read before the call returns); floor > 0; `pools`
    divides W -> out (N, M * pools) float32, every element written:
        p[h,t] = (x[n,c,h,t] * scale[h] + scale[h]) ** 2 and s[m,t] = sum of weight[m,h] * p[h,t] over lo[m] <= h < hi[m], in
        float32 in ascending h; out[n, m * pools + j] = the float64 mean of log(s[m,t] + floor) over the W / pools columns of
        pool j, in ascending t, rounded once.
    Weights outside [lo, hi) are not read.  A row of out depends on its image and on the shapes alone.  Returns out."""
    if not all(isinstance(t, torch.Tensor) for t in (x, scale, weight)):
        raise ValueError("logmel_rows: tensors x, scale and weight expected")
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"logmel_rows: a non-empty batch x (N, C, H, W) expected, got {tuple(x.shape)}")
    n, ch, h, w = x.shape
    if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < ch:
        raise ValueError(f"logmel_rows: a channel in 0 .. {ch - 1} expected, got {c}")
    if weight.dim() != 2 or weight.shape[1] != h or not 1 <= weight.shape[0] <= MAX_BANDS or tuple(scale.shape) != (h,):
        raise ValueError(f"logmel_rows: scale ({h},) and weight (M, {h}) with M in 1 .. {MAX_BANDS} expected, got "
                         f"{tuple(scale.shape)} and {tuple(weight.shape)}")
    bands = weight.shape[0]
    if isinstance(pools, bool) or not isinstance(pools, int) or pools < 1 or w % pools or w // pools > MAX_POOL:
        raise ValueError(f"logmel_rows: a pool count that divides W = {w} into pools of at most {MAX_POOL} columns expected, got {pools}")
    lo, hi = _limits("lo", lo, bands), _limits("hi", hi, bands)
    if bool(((lo < 0) | (lo > hi) | (hi > h)).any()):
        raise ValueError(f"logmel_rows: 0 <= lo <= hi <= H = {h} expected for every band")
    floor = float(floor)
    if not 0.0 < floor < float("inf"):
        raise ValueError(f"logmel_rows: a finite floor > 0 expected, got {floor}")
    if out is not None and tuple(out.shape) != (n, bands * pools):
        raise ValueError(f"logmel_rows: out ({n}, {bands * pools}) expected, got {tuple(out.shape)}")
    _chk_typed("logmel_rows", x, scale, weight)
    if out is None:
        out = torch.empty((n, bands * pools), dtype=torch.float32, device=x.device)
    _chk_typed("logmel_rows", out)
    i32p = ctypes.POINTER(ctypes.c_int32)
    check(_lib.load().mg_logmel_rows(_p(x), n, ch, c, h, w, _p(scale), _p(weight), ctypes.cast(lo.data_ptr(), i32p),
                                     ctypes.cast(hi.data_ptr(), i32p), bands, floor, pools, _p(out), _s()), "mg_logmel_rows")
    return out


def _moments_shape(rows) -> Tuple[int, int]:
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
        raise ValueError("moments: rows (n, d) expected")
    n, d = rows.shape
    if not 2 <= n <= MAX_N or not 1 <= d <= MAX_D:
        raise ValueError(f"moments: 2 .. {MAX_N} rows of 1 .. {MAX_D} numbers expected, got {tuple(rows.shape)}")
    return n, d


def moments_ws_bytes(n: int, d: int) -> int:
    """host query: the scratch memory moments allocates for n rows of d numbers (float64 sums of chunks of 1024 rows: a (d,) and a
    (d, d) block per chunk); 0 for a shape moments refuses"""
    return int(_lib.load().mg_moments_ws_bytes(n, d))


def moments(rows: torch.Tensor, mean: Optional[torch.Tensor] = None, cov: Optional[torch.Tensor] = None):
    """rows (n, d) float32, n >= 2, d <= 4096 -> all of mean (d,) and all of cov (d, d) float64 are written: the mean over the rows
    and the unbiased covariance sum_i (x_ij - mean_j)(x_ik - mean_k) / (n - 1), two passes in float64 in a fixed order (chunks of
    1024 rows, added in chunk order): the same bits in every run, and cov[j, k] and cov[k, j] hold the same bits.  Returns
    (mean, cov)."""
    n, d = _moments_shape(rows)
    for name, t, shape in (("mean", mean, (d,)), ("cov", cov, (d, d))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"moments: {name} {shape} expected, got {tuple(t.shape)}")
    _chk_typed("moments", rows)
    if mean is None:
        mean = torch.empty(d, dtype=torch.float64, device=rows.device)
    if cov is None:
        cov = torch.empty((d, d), dtype=torch.float64, device=rows.device)
    _chk_typed("moments", mean, cov, dtype=torch.float64)
    nbytes = moments_ws_bytes(n, d)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=rows.device)
    check(_lib.load().mg_moments(_p(rows), n, d, _p(mean), _p(cov), _p(ws), nbytes, _s()), "mg_moments")
    return mean, cov

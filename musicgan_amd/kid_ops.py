"""Tensor-level wrappers over mg_standardise_rows and mg_polyk_rowsums of the C ABI (include/musicgan_hip.h, csrc/kid.hip): rows
standardised by float64 moments, and the row sums of the polynomial kernel k(x, y) = (x.y / d + 1)^3 over subsets of two row sets,
fused so that no kernel matrix is stored -- what metrics.poly_mmd2 and metrics.KID are made of.  Every call is asynchronous on the
caller's current stream and reads nothing back; scratch memory (the partial row sums of the column blocks) is allocated here with
torch.empty, call by call.  Shapes are checked on the host, before any tensor's device is looked at.  No fallback path exists:
non-GPU tensors raise."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import check
from .ops import _chk_typed, _p, _s

MAX_D = 4096          # numbers per row polyk_rowsums takes: 16 chunks of 256, walked by one workgroup
MAX_SUBSETS = 65535   # subsets of one launch (grid z)
MAX_ROWS = 1 << 22    # rows of a subset


def _rows(what: str, name: str, t) -> tuple:
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or min(t.shape) < 1:
        raise ValueError(f"{what}: {name}: non-empty rows (n, d) expected, got {tuple(t.shape) if isinstance(t, torch.Tensor) else t!r}")
    return tuple(t.shape)


def standardise_rows(x: torch.Tensor, mean: torch.Tensor, sd: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (n, d) float32, mean (d,) and sd (d,) float64 -> out (n, d) float32, every element written:
        out[i, j] = float32((float64(x[i, j]) - mean[j]) / sd[j]), and 0 in a column whose sd is 0, infinite or NaN,
    bit-equal to that float64 definition.  Returns out."""
    n, d = _rows("standardise_rows", "x", x)
    for name, t in (("mean", mean), ("sd", sd)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (d,):
            raise ValueError(f"standardise_rows: {name} ({d},) expected, got {tuple(t.shape) if isinstance(t, torch.Tensor) else t!r}")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, d)):
        raise ValueError(f"standardise_rows: out ({n}, {d}) expected")
    _chk_typed("standardise_rows", x)
    _chk_typed("standardise_rows", mean, sd, dtype=torch.float64)
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=x.device)
    _chk_typed("standardise_rows", out)
    check(_lib.load().mg_standardise_rows(_p(x), n, d, _p(mean), _p(sd), _p(out), _s()), "mg_standardise_rows")
    return out


def _count(name: str, v, most: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= most:
        raise ValueError(f"polyk: {name} in 1 .. {most} expected, got {v!r}")
    return v


def polyk_ws_bytes(subsets: int, ma: int, mb: int) -> int:
    """host query: the scratch memory polyk_rowsums allocates for `subsets` subsets of ma x mb pairs (one float64 per subset, block
    of 128 columns and row); 0 for a shape polyk_rowsums refuses"""
    return int(_lib.load().mg_polyk_ws_bytes(subsets, ma, mb))


def polyk_rowsums(a: torch.Tensor, b: torch.Tensor, ia: Optional[torch.Tensor] = None, ib: Optional[torch.Tensor] = None, *,
                  skip_diag: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a (na, d) and b (nb, d) float32, d <= 4096; ia (subsets, ma) and ib (subsets, mb) int32 row numbers on the device, None = all
    rows in their order (one subset unless the other list names more) -> out (subsets, ma) float64, every element written:
        out[s, i] = the sum over j of k(a[ia[s, i]], b[ib[s, j]]),  k(x, y) = (x.y / d + 1) ** 3,
    without the pairs j = i if skip_diag (which needs ma = mb).  The rows are gathered by the kernel; a row number outside its set is
    clamped into it.  x.y: float32 in chunks of 256 components, the chunks added in float64; everything after it is float64 in a
    fixed order.  out[s, i] is a function of its row of a, the ordered b rows of subset s, d and skip_diag alone,
    and the same bits in every run.  Returns out."""
    (na, d), (nb, db) = _rows("polyk_rowsums", "a", a), _rows("polyk_rowsums", "b", b)
    if d != db:
        raise ValueError(f"polyk_rowsums: rows of one length expected, got {d} and {db}")
    if d > MAX_D:
        raise ValueError(f"polyk_rowsums: at most {MAX_D} numbers per row, got {d}")
    subsets = None
    for name, t in (("ia", ia), ("ib", ib)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or min(t.shape) < 1:
            raise ValueError(f"polyk_rowsums: {name}: a non-empty int32 tensor (subsets, m) expected")
        if subsets is not None and t.shape[0] != subsets:
            raise ValueError(f"polyk_rowsums: ia and ib name {subsets} and {t.shape[0]} subsets")
        subsets = t.shape[0]
    subsets = _count("subsets", 1 if subsets is None else int(subsets), MAX_SUBSETS)
    ma = _count("ma", na if ia is None else int(ia.shape[1]), MAX_ROWS)
    mb = _count("mb", nb if ib is None else int(ib.shape[1]), MAX_ROWS)
    if skip_diag and ma != mb:
        raise ValueError(f"polyk_rowsums: skip_diag needs as many rows as columns, got {ma} and {mb}")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (subsets, ma)):
        raise ValueError(f"polyk_rowsums: out ({subsets}, {ma}) expected")
    _chk_typed("polyk_rowsums", a, b)
    lists = [t for t in (ia, ib) if t is not None]
    _chk_typed("polyk_rowsums", *lists, dtype=torch.int32)
    if out is None:
        out = torch.empty((subsets, ma), dtype=torch.float64, device=a.device)
    _chk_typed("polyk_rowsums", out, dtype=torch.float64)
    nbytes = polyk_ws_bytes(subsets, ma, mb)
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=a.device)
    check(_lib.load().mg_polyk_rowsums(_p(a), na, _p(b), nb, _p(ia), _p(ib), subsets, ma, mb, d, int(bool(skip_diag)), _p(out),
                                       _p(ws), nbytes, _s()), "mg_polyk_rowsums")
    return out

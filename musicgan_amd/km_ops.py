"""Tensor-level wrappers over the mg_km_* entries of the C ABI (include/musicgan_hip.h, csrc/kmeans.hip): the half of a Lloyd iteration
that is not a distance -- the nearest bin of every row of a distance block, the stable ordering of the points by bin, the segmented
float64 mean -- and the bin counts of metrics.NDB.  Every call is asynchronous on the caller's current stream and reads nothing back;
scratch memory (the update's partial sums) is allocated here with torch.empty, call by call.  No fallback path exists: non-GPU tensors
raise."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import check
from .ops import _chk_typed, _p, _s

MAX_K = 1024        # bins
MAX_N = 1 << 20     # points km_order and km_update take


def _bins(k) -> int:
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"k in 1 .. {MAX_K} expected, got {k}")
    return k


def km_update_ws_bytes(n: int, d: int, k: int) -> int:
    """host query: the scratch memory km_update allocates for n rows of d numbers in k bins (float64 sums of chunks of 32 members)"""
    return int(_lib.load().mg_km_update_ws_bytes(n, d, k))


def km_assign(dist: torch.Tensor, label: torch.Tensor, mind: Optional[torch.Tensor] = None,
              changed: Optional[torch.Tensor] = None):
    """dist (n, k) float64 -> for every row the column of its smallest entry (ties: the smaller column) into label (n,) int32 and that
    entry into mind (n,) float64: all of label and all of mind are written.  changed (1,) int64 is overwritten, not accumulated, with
    the number of rows whose label was rewritten with a different value.  Returns (label, mind, changed)."""
    _chk_typed("km_assign", dist, dtype=torch.float64)
    _chk_typed("km_assign", label, dtype=torch.int32)
    if dist.dim() != 2 or dist.shape[0] < 1:
        raise ValueError(f"a non-empty block dist (n, k) expected, got {tuple(dist.shape)}")
    n, k = dist.shape[0], _bins(dist.shape[1])
    if mind is None:
        mind = torch.empty(n, dtype=torch.float64, device=dist.device)
    if changed is None:
        changed = torch.empty(1, dtype=torch.int64, device=dist.device)
    _chk_typed("km_assign", mind, dtype=torch.float64)
    _chk_typed("km_assign", changed, dtype=torch.int64)
    assert tuple(label.shape) == (n,) and tuple(mind.shape) == (n,) and changed.numel() == 1
    check(_lib.load().mg_km_assign(_p(dist), n, k, _p(label), _p(mind), _p(changed), _s()), "mg_km_assign")
    return label, mind, changed


def km_order(label: torch.Tensor, k: int, start: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None):
    """label (n,) int32 with values in 0 .. k-1 -> all of start (k + 1,) int32, the exclusive prefix sums of the bin sizes, and
    all of order (n,) int32, the positions sorted by (label, position): bin j's members are order[start[j] : start[j + 1]],
    ascending.  n <= 2^20.  Returns (start, order)."""
    _chk_typed("km_order", label, dtype=torch.int32)
    k = _bins(k)
    if label.dim() != 1 or label.shape[0] < 1:
        raise ValueError(f"a non-empty label vector (n,) expected, got {tuple(label.shape)}")
    n = label.shape[0]
    if n > MAX_N:
        raise ValueError(f"at most {MAX_N} points expected, got {n}")
    if start is None:
        start = torch.empty(k + 1, dtype=torch.int32, device=label.device)
    if order is None:
        order = torch.empty(n, dtype=torch.int32, device=label.device)
    _chk_typed("km_order", start, order, dtype=torch.int32)
    assert tuple(start.shape) == (k + 1,) and tuple(order.shape) == (n,)
    check(_lib.load().mg_km_order(_p(label), n, k, _p(start), _p(order), _s()), "mg_km_order")
    return start, order


def km_update(x: torch.Tensor, order: torch.Tensor, start: torch.Tensor, centroid: torch.Tensor) -> torch.Tensor:
    """x (n, d) float32 with km_order's order (n,) and start (k + 1,) int32 -> centroid (k, d) float32, updated in place: row j becomes
    the float64 sum of x[order[start[j] : start[j + 1]]] in that order (chunks of 32 members, added in chunk order), divided in float64
    by the member count and rounded once to float32; the row of a bin without members keeps its bits.  A row depends on its ordered
    member list alone.  n <= 2^20.  Returns centroid."""
    _chk_typed("km_update", x, centroid)
    _chk_typed("km_update", order, start, dtype=torch.int32)
    if x.dim() != 2 or centroid.dim() != 2 or x.shape[1] != centroid.shape[1] or min(x.shape[0], x.shape[1], centroid.shape[0]) < 1:
        raise ValueError(f"x (n, d) and centroid (k, d) expected, got {tuple(x.shape)} and {tuple(centroid.shape)}")
    n, d, k = x.shape[0], x.shape[1], _bins(centroid.shape[0])
    if n > MAX_N:
        raise ValueError(f"at most {MAX_N} points expected, got {n}")
    assert tuple(order.shape) == (n,) and tuple(start.shape) == (k + 1,)
    nbytes = km_update_ws_bytes(n, d, k)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    check(_lib.load().mg_km_update(_p(x), n, d, _p(order), _p(start), k, _p(centroid), _p(ws), nbytes, _s()), "mg_km_update")
    return centroid


def km_count(label: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """label (n,) int32 -> count (k,) int64: count[label[i]] += 1 for every i, accumulated in place, so a set goes through in batches
    without being kept; labels outside 0 .. k-1 are skipped.  Returns count."""
    _chk_typed("km_count", label, dtype=torch.int32)
    _chk_typed("km_count", count, dtype=torch.int64)
    if label.dim() != 1 or label.shape[0] < 1 or count.dim() != 1:
        raise ValueError(f"a non-empty label vector (n,) and counters (k,) expected, got {tuple(label.shape)} and {tuple(count.shape)}")
    k = _bins(count.shape[0])
    check(_lib.load().mg_km_count(_p(label), label.shape[0], k, _p(count), _s()), "mg_km_count")
    return count

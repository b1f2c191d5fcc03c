"""Tensor-level wrappers over the mg_nn_* / mg_prdc_* entries of the C ABI (include/musicgan_hip.h, csrc/nn.hip, csrc/prdc.hip): squared
L2 distances between rows of float32 numbers, the k nearest of a stream of candidates, and the ball-membership scan of metrics.PRDC.  Every call is asynchronous on the caller's current stream;
scratch memory (the per-chunk partial sums) is allocated here with torch.empty, call by call.  No fallback path exists: non-GPU
tensors raise."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import check
from .ops import _chk_typed, _p, _s

MAX_K = 16
EMPTY = torch.finfo(torch.float64).max   # the distance of a slot of a best list that holds no neighbour yet (its id is -1)


def nn_chunk() -> int:
    """host query: the number of consecutive components whose products one wave adds in float32"""
    return int(_lib.load().mg_nn_chunk())


def nn_ws_bytes(nq: int, nr: int, d: int) -> int:
    """host query: the scratch memory nn_sqdist allocates for nq x nr pairs of rows of d numbers"""
    return int(_lib.load().mg_nn_ws_bytes(nq, nr, d))


def nn_sqnorm(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (n, D) float32 -> all of out (n,) float64: every row's sum of squares, added in an order that depends on D alone"""
    _chk_typed("nn_sqnorm", x)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"a non-empty (n, D) matrix expected, got {tuple(x.shape)}")
    if out is None:
        out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    _chk_typed("nn_sqnorm", out, dtype=torch.float64)
    assert tuple(out.shape) == (x.shape[0],)
    check(_lib.load().mg_nn_sqnorm(_p(x), x.shape[0], x.shape[1], _p(out), _s()), "mg_nn_sqnorm")
    return out


def nn_sqdist(q: torch.Tensor, r: torch.Tensor, qn: torch.Tensor, rn: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q (nq, D), r (nr, D) float32 and their nn_sqnorm qn (nq,), rn (nr,) -> all of out (nq, nr) float64: max(0, qn + rn - 2 q.r).
    A pair's value depends on its two rows alone."""
    _chk_typed("nn_sqdist", q, r)
    _chk_typed("nn_sqdist", qn, rn, dtype=torch.float64)
    if q.dim() != 2 or r.dim() != 2 or q.shape[1] != r.shape[1] or min(q.shape[0], r.shape[0], q.shape[1]) < 1:
        raise ValueError(f"two non-empty matrices (nq, D) and (nr, D) expected, got {tuple(q.shape)} and {tuple(r.shape)}")
    nq, nr, d = q.shape[0], r.shape[0], q.shape[1]
    assert tuple(qn.shape) == (nq,) and tuple(rn.shape) == (nr,)
    if out is None:
        out = torch.empty((nq, nr), dtype=torch.float64, device=q.device)
    _chk_typed("nn_sqdist", out, dtype=torch.float64)
    assert tuple(out.shape) == (nq, nr)
    nbytes = nn_ws_bytes(nq, nr, d)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    check(_lib.load().mg_nn_sqdist(_p(q), _p(r), _p(qn), _p(rn), nq, nr, d, _p(out), _p(ws), nbytes, _s()), "mg_nn_sqdist")
    return out


def nn_merge(dist: torch.Tensor, rid: torch.Tensor, best_d: torch.Tensor, best_i: torch.Tensor,
             qid: Optional[torch.Tensor] = None) -> None:
    """the candidates dist (nq, nr) float64 with the ids rid (nr,) int64 into the best lists best_d (nq, k) float64 and best_i
    (nq, k) int64, both rewritten whole: ascending by (distance, id), an empty slot is (EMPTY, -1).  A candidate whose id equals
    qid[i] >= 0 (int64, optional) is not a neighbour of query i."""
    _chk_typed("nn_merge", dist, best_d, dtype=torch.float64)
    _chk_typed("nn_merge", rid, best_i, dtype=torch.int64)
    if qid is not None:
        _chk_typed("nn_merge", qid, dtype=torch.int64)
    if dist.dim() != 2 or best_d.dim() != 2 or dist.shape[0] < 1 or dist.shape[1] < 1:
        raise ValueError(f"dist (nq, nr) and best lists (nq, k) expected, got {tuple(dist.shape)} and {tuple(best_d.shape)}")
    nq, nr = dist.shape
    k = best_d.shape[1]
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k in 1 .. {MAX_K} expected, got {k}")
    assert tuple(best_d.shape) == (nq, k) and best_i.shape == best_d.shape and tuple(rid.shape) == (nr,)
    assert qid is None or tuple(qid.shape) == (nq,)
    check(_lib.load().mg_nn_merge(_p(dist), _p(qid), _p(rid), _p(best_d), _p(best_i), nq, nr, k, _s()), "mg_nn_merge")


def nn_tiled_ws_bytes(nq: int, nr: int, d: int) -> int:
    """host query: the scratch memory nn_sqdist_tiled allocates for nq x nr pairs of rows of d numbers (16 float64 per pair)"""
    return int(_lib.load().mg_nn_tiled_ws_bytes(nq, nr, d))


def nn_sqdist_tiled(q: torch.Tensor, r: torch.Tensor, qn: torch.Tensor, rn: torch.Tensor,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn_sqdist for operands of thousands of rows each: q (nq, D), r (nr, D) float32 and their nn_sqnorm qn (nq,), rn (nr,) ->
    all of out (nq, nr) float64, bit for bit what nn_sqdist writes, with the rows staged in LDS and shared by 128 x 128 pairs."""
    _chk_typed("nn_sqdist_tiled", q, r)
    _chk_typed("nn_sqdist_tiled", qn, rn, dtype=torch.float64)
    if q.dim() != 2 or r.dim() != 2 or q.shape[1] != r.shape[1] or min(q.shape[0], r.shape[0], q.shape[1]) < 1:
        raise ValueError(f"two non-empty matrices (nq, D) and (nr, D) expected, got {tuple(q.shape)} and {tuple(r.shape)}")
    nq, nr, d = q.shape[0], r.shape[0], q.shape[1]
    assert tuple(qn.shape) == (nq,) and tuple(rn.shape) == (nr,)
    if out is None:
        out = torch.empty((nq, nr), dtype=torch.float64, device=q.device)
    _chk_typed("nn_sqdist_tiled", out, dtype=torch.float64)
    assert tuple(out.shape) == (nq, nr)
    nbytes = nn_tiled_ws_bytes(nq, nr, d)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=q.device)
    check(_lib.load().mg_nn_sqdist_tiled(_p(q), _p(r), _p(qn), _p(rn), nq, nr, d, _p(out), _p(ws), nbytes, _s()),
          "mg_nn_sqdist_tiled")
    return out


def prdc_scan(dist: torch.Tensor, radius: torch.Tensor, count: torch.Tensor, rowmin: torch.Tensor) -> None:
    """one block dist (nq, nr) float64 of a distance matrix against the radii radius (nr,) float64 of its columns: count (nq,) int64
    += the number of columns j with dist[i][j] <= radius[j], rowmin (nq,) float64 = min(rowmin, the row's smallest distance); both
    accumulated in place, so a matrix goes through in column blocks with the same result."""
    _chk_typed("prdc_scan", dist, radius, rowmin, dtype=torch.float64)
    _chk_typed("prdc_scan", count, dtype=torch.int64)
    if dist.dim() != 2 or dist.shape[0] < 1 or dist.shape[1] < 1:
        raise ValueError(f"a non-empty block dist (nq, nr) expected, got {tuple(dist.shape)}")
    nq, nr = dist.shape
    assert tuple(radius.shape) == (nr,) and tuple(count.shape) == (nq,) and tuple(rowmin.shape) == (nq,)
    check(_lib.load().mg_prdc_scan(_p(dist), _p(radius), _p(count), _p(rowmin), nq, nr, _s()), "mg_prdc_scan")

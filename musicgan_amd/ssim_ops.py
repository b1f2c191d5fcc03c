"""Tensor-level wrappers over the mg_ssim_* entries of the C ABI (include/musicgan_hip.h, csrc/ssim.hip): multi-scale structural
similarity between pairs of float32 images.  Every call is asynchronous on the caller's current stream; scratch memory (the
coarser scales, the per-tile sums) is allocated here with torch.empty, call by call.  No fallback path exists: non-GPU tensors
raise."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import check
from .ops import _chk_typed, _p, _s

WINDOW = 11


def ssim_scales(h: int, w: int) -> int:
    """host query: the number of scales of an h x w image, 0 when a side is below the window"""
    return int(_lib.load().mg_ssim_scales(h, w))


def ssim_window() -> torch.Tensor:
    """host query: the 11 float32 taps of the window, as the kernels receive them"""
    taps = (ctypes.c_float * WINDOW)()
    check(_lib.load().mg_ssim_window(taps), "mg_ssim_window")
    return torch.tensor(list(taps), dtype=torch.float32)


def ssim_tiles(h: int, w: int) -> int:
    """host query: the workgroups, and so the slots, per channel plane of an h x w level"""
    return int(_lib.load().mg_ssim_tiles(h, w))


def ssim_scratch_bytes(n: int, c: int, h: int, w: int) -> int:
    """host query: the scratch memory ms_ssim_into allocates for n pairs of (c, h, w) images"""
    return int(_lib.load().mg_ssim_scratch_bytes(n, c, h, w))


def ssim_scale(a: torch.Tensor, b: torch.Tensor, slots: torch.Tensor, a_next: Optional[torch.Tensor] = None,
               b_next: Optional[torch.Tensor] = None) -> None:
    """one scale of the pairs a, b (N, C, H, W): every tile's float64 sums of cs and ssim into all of slots (N, C, tiles, 2) and,
    where given, the 2 x 2 means of a and b into all of a_next and b_next (N, C, H/2, W/2)"""
    _chk_typed("ssim_scale", a, b)
    _chk_typed("ssim_scale", slots, dtype=torch.float64)
    n, c, h, w = a.shape
    assert b.shape == a.shape and (a_next is None) == (b_next is None)
    assert tuple(slots.shape) == (n, c, ssim_tiles(h, w), 2), (tuple(slots.shape), (n, c, ssim_tiles(h, w), 2))
    if a_next is not None:
        _chk_typed("ssim_scale", a_next, b_next)
        assert tuple(a_next.shape) == (n, c, h // 2, w // 2) and a_next.shape == b_next.shape
    check(_lib.load().mg_ssim_scale(_p(a), _p(b), _p(a_next), _p(b_next), _p(slots), n, c, h, w, _s()), "mg_ssim_scale")


def ssim_finish(slots: torch.Tensor, n: int, c: int, h: int, w: int, values: torch.Tensor, terms: Optional[torch.Tensor] = None,
                row: int = 0) -> None:
    """slots: the float64 slots of every scale of n pairs of (c, h, w) images, one scale after the other -> values[row .. row + n]
    (float64, one MS-SSIM per pair) and, where given, terms[row .. row + n] (rows, S) float64: the means before the clamp"""
    _chk_typed("ssim_finish", slots, values, dtype=torch.float64)
    assert values.dim() == 1
    if terms is not None:
        _chk_typed("ssim_finish", terms, dtype=torch.float64)
        assert tuple(terms.shape) == (values.shape[0], ssim_scales(h, w))
    check(_lib.load().mg_ssim_finish(_p(slots), slots.numel(), n, c, h, w, _p(values), _p(terms), row, values.shape[0], _s()),
          "mg_ssim_finish")


def ssim_mean(values: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out (one float64) = the mean of the float64 values, added in an order that depends on their number alone"""
    _chk_typed("ssim_mean", values, out, dtype=torch.float64)
    assert values.dim() == 1 and out.numel() == 1
    check(_lib.load().mg_ssim_mean(_p(values), values.numel(), _p(out), _s()), "mg_ssim_mean")
    return out


def ms_ssim_into(a: torch.Tensor, b: torch.Tensor, values: torch.Tensor, terms: Optional[torch.Tensor] = None, row: int = 0) -> None:
    """MS-SSIM of the pairs (a[i], b[i]) of two (N, C, H, W) batches into values[row .. row + N] (and terms[row .. row + N]): one
    launch per scale, each leaving the next scale's images behind, then the finish.  Kernel launches only."""
    _chk_typed("ms_ssim_into", a, b)
    if a.dim() != 4 or a.shape != b.shape or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"two non-empty (N, C, H, W) batches of one shape expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    n, c, h, w = a.shape
    scales = ssim_scales(h, w)
    if scales < 1:
        raise ValueError(f"sides >= {WINDOW} expected, got {h} x {w}")
    counts = [n * c * ssim_tiles(h >> s, w >> s) * 2 for s in range(scales)]
    slots = torch.empty(sum(counts), dtype=torch.float64, device=a.device)
    lo = 0
    for s in range(scales):
        nxt = (None, None)
        if s + 1 < scales:
            nxt = tuple(torch.empty((n, c, h >> (s + 1), w >> (s + 1)), dtype=torch.float32, device=a.device) for _ in range(2))
        ssim_scale(a, b, slots[lo:lo + counts[s]].view(n, c, -1, 2), *nxt)
        lo += counts[s]
        a, b = nxt
    ssim_finish(slots, n, c, h, w, values, terms, row)

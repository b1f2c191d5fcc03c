"""Tensor-level wrappers over the limiter entries of the C ABI (include/musicgan_hip.h, csrc/limiter.hip): the true-peak envelope of a
waveform, the look-ahead limiter that keeps every sample of x G g under a ceiling with one gain curve g for all channels, the trim
by a device scalar and the pre-gain that brings a measured loudness to a target.  Waveforms are float32 (C, L) with C <= 8 and unit
stride along L (any row stride).  Every call is asynchronous on the caller's current stream and synchronises nothing; the pre-gain,
the peak and the record stay in device memory, so a chain of calls can be captured in a graph.  Scratch memory comes from
`ops.workspace`.  No fallback path exists: non-GPU tensors raise."""
from __future__ import annotations

import math

import torch

from . import _lib, loud_ops, ops
from ._lib import check
from .ops import _p, _s

TILE = 2048                   # samples per workgroup of the hold, release and output kernels (TILE of csrc/limiter.hip, mg_limiter_tile)
MAX_LOOKAHEAD = 2047          # samples; a window never spans more than two tiles
MAX_PASSES = 4


def _number(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def check_arguments(sample_rate, ceiling_dbtp=-1.0, attack_ms=5.0, release_ms=50.0):
    """-> (ceiling, lookahead, rho): the linear ceiling 10^(dBTP / 20), the look-ahead round(attack_ms fs / 1000) in samples
    (0 .. MAX_LOOKAHEAD) and the release factor exp(-1 / (release_ms fs / 1000)) per sample, in (0, 1); host arithmetic in float64,
    ValueError for anything else."""
    fs = loud_ops.check_sample_rate(sample_rate)
    ceiling = 10.0 ** (_number("ceiling_dbtp", ceiling_dbtp) / 20.0)
    attack, release = _number("attack_ms", attack_ms), _number("release_ms", release_ms)
    lookahead = int(round(attack * fs / 1000.0)) if attack >= 0 else -1
    if not 0 <= lookahead <= MAX_LOOKAHEAD:
        raise ValueError(f"attack_ms must give a look-ahead of 0 .. {MAX_LOOKAHEAD} samples, got {attack_ms!r} at {fs} Hz")
    rho = math.exp(-1.0 / (release * fs / 1000.0)) if release > 0 else 0.0
    if not 0.0 < rho < 1.0 or not 0.0 < ceiling < math.inf:
        raise ValueError(f"release_ms must be positive (a release factor in (0, 1)) and the ceiling finite, got {release_ms!r}, "
                         f"{ceiling_dbtp!r}")
    return ceiling, lookahead, rho


def check_passes(passes) -> int:
    if isinstance(passes, bool) or not isinstance(passes, int) or not 1 <= passes <= MAX_PASSES:
        raise ValueError(f"passes must be an integer in 1 .. {MAX_PASSES}, got {passes!r}")
    return passes


def _chk(name: str, x: torch.Tensor) -> None:
    loud_ops.check_waveform(x)
    if not x.is_cuda:
        raise _lib.MusicGanHipError(f"{name}: tensors on a ROCm GPU expected (no CPU fallback)")
    if x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise _lib.MusicGanHipError(f"{name}: float32 (C, L) with unit stride along L expected, got {x.dtype} strides {x.stride()}")


def _chk_scalar(name: str, what: str, t: torch.Tensor, dtype, like: torch.Tensor) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() != 1 or t.device != like.device:
        raise _lib.MusicGanHipError(f"{name}: {what}: one {dtype} on the waveform's device expected")


def envelope(x: torch.Tensor) -> torch.Tensor:
    """x float32 (C, L) -> m float32 (L,): per sample the largest magnitude over the channels of the sample and of the seven points
    4n - 3 .. 4n + 3 of the 4x interpolation `ops.resample_rows(x, 1, 4)` (its bits; points beyond the ends do not count).  One
    launch (`mg_limiter_envelope`)."""
    _chk("envelope", x)
    channels, length = x.shape
    out = torch.empty((length,), dtype=torch.float32, device=x.device)
    if length == 0:
        return out
    bank = ops.resample_bank(1, 4, 6, 0.99, x.device)
    check(_lib.load().mg_limiter_envelope(_p(x), channels, length, x.stride(0), _p(bank), bank.numel(), _p(out), _s()),
          "mg_limiter_envelope")
    return out


def limit(x: torch.Tensor, pregain: torch.Tensor, ceiling: float, lookahead: int, rho: float, return_gain: bool = False):
    """x float32 (C, L), pregain one float64 on the device (G), ceiling linear, lookahead in samples (0 .. MAX_LOOKAHEAD), rho the
    release factor per sample in (0, 1) -> float32 (C, L) contiguous: float32(double(x) G g) with the gain curve g of DESIGN.md,
    "True-peak limiter"; return_gain: also g, float64 (L,).  Five launches (`mg_limiter`); the same bits on every run."""
    _chk("limit", x)
    _chk_scalar("limit", "pregain", pregain, torch.float64, x)
    if isinstance(lookahead, bool) or not isinstance(lookahead, int) or not 0 <= lookahead <= MAX_LOOKAHEAD:
        raise ValueError(f"limit: a look-ahead of 0 .. {MAX_LOOKAHEAD} samples expected, got {lookahead!r}")
    ceiling, rho = float(ceiling), float(rho)
    if not (0.0 < ceiling < math.inf and 0.0 < rho < 1.0):
        raise ValueError(f"limit: a positive finite ceiling and a release factor in (0, 1) expected, got {ceiling!r}, {rho!r}")
    channels, length = x.shape
    out = torch.empty((channels, length), dtype=torch.float32, device=x.device)
    gain = torch.empty((length,), dtype=torch.float64, device=x.device) if return_gain else None
    if length > 0:
        lib = _lib.load()
        bank = ops.resample_bank(1, 4, 6, 0.99, x.device)
        nbytes = int(lib.mg_limiter_ws_bytes(channels, length, lookahead))
        if nbytes == 0:
            raise ValueError(f"limit: {length} samples are too many")
        ws = ops.workspace(nbytes, x.device)
        check(lib.mg_limiter(_p(x), channels, length, x.stride(0), _p(bank), bank.numel(), _p(pregain), ceiling, lookahead, rho,
                             _p(out), _p(gain), _p(ws), nbytes, _s()), "mg_limiter")
    return (out, gain) if return_gain else out


def trim(y: torch.Tensor, peak: torch.Tensor, ceiling: float) -> torch.Tensor:
    """y float32 contiguous, peak the float32 of `loud_ops.true_peak(y)` on the device -> float32(double(y) min(1, ceiling / peak)).
    One launch (`mg_limiter_trim`); the factor never visits the host."""
    if not isinstance(y, torch.Tensor) or not y.is_cuda or y.dtype != torch.float32 or not y.is_contiguous():
        raise _lib.MusicGanHipError("trim: contiguous float32 waveform on a ROCm GPU expected (no CPU fallback)")
    _chk_scalar("trim", "peak", peak, torch.float32, y)
    ceiling = float(ceiling)
    if not 0.0 < ceiling < math.inf:
        raise ValueError(f"trim: a positive finite ceiling expected, got {ceiling!r}")
    out = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    check(_lib.load().mg_limiter_trim(_p(y), _p(out), y.numel(), _p(peak), ceiling, _s()), "mg_limiter_trim")
    return out


def pregain(record: torch.Tensor, target_lufs: float, prev=None) -> torch.Tensor:
    """record of `loud_ops.gate` -> float64 (1,) on the device: prev * 10^((target_lufs - record[0]) / 20) (prev: a pre-gain of an
    earlier pass, default 1); the factor is 1 where record[0] is -inf.  One launch (`mg_limiter_pregain`)."""
    target = _number("target_lufs", target_lufs)
    if not isinstance(record, torch.Tensor) or not record.is_cuda or record.dtype != torch.float64 or record.numel() != 4 \
            or not record.is_contiguous():
        raise _lib.MusicGanHipError("pregain: the float64 record of `gate` on a ROCm GPU expected (no CPU fallback)")
    if prev is not None:
        _chk_scalar("pregain", "prev", prev, torch.float64, record)
    out = torch.empty((1,), dtype=torch.float64, device=record.device)
    check(_lib.load().mg_limiter_pregain(_p(record), target, _p(prev), _p(out), _s()), "mg_limiter_pregain")
    return out

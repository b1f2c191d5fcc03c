"""Tensor-level wrappers over the phase-vocoder entries of the C ABI (include/musicgan_hip.h, csrc/phasevocoder.hip).  Spectra are
complex64 (512, T), frequency-major, as `ops.stft_1024` returns them; the rate is the rational number p / q.  The call is
asynchronous on the caller's current stream and synchronises nothing; scratch memory comes from `ops.workspace` (one buffer per device
and stream, shared with the other op modules), the result from torch.empty.  No fallback path exists: non-GPU tensors raise."""
from __future__ import annotations

from fractions import Fraction

import torch

from . import _lib, ops
from ._lib import check
from .ops import _p, _s

TIME_TILE = 256                                  # output frames per workgroup (TILE of csrc/phasevocoder.hip)
LOCK_TILE = 256                                  # output frames per composed map of the locked vocoder (LOCK_TILE there)
MIN_RATE, MAX_RATE = Fraction(1, 8), Fraction(8)


def as_rate(rate) -> Fraction:
    """an int, a Fraction or a float (taken as Fraction(rate).limit_denominator(1000)) -> the rate as a Fraction in [1/8, 8];
    ValueError otherwise, raised before anything touches the device"""
    if isinstance(rate, bool) or not isinstance(rate, (int, float, Fraction)):
        raise ValueError(f"rate must be an int, a fractions.Fraction or a float, got {rate!r}")
    if isinstance(rate, float):
        if rate != rate or rate in (float("inf"), float("-inf")):
            raise ValueError(f"rate must be finite, got {rate!r}")
        rate = Fraction(rate).limit_denominator(1000)
    rate = Fraction(rate)
    if not MIN_RATE <= rate <= MAX_RATE:
        raise ValueError(f"rate must lie in [1/8, 8], got {rate}")
    return rate


def check_arguments(frames: int, p: int, q: int) -> None:
    """the argument errors of the phase vocoder, raised before anything touches the device"""
    for name, v in (("frames", frames), ("p", p), ("q", q)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if p < 1 or q < 1 or p >= 1 << 31 or q >= 1 << 31:
        raise ValueError(f"p and q must lie in [1, 2^31), got {p} and {q}")
    if not MIN_RATE <= Fraction(p, q) <= MAX_RATE:
        raise ValueError(f"rate must lie in [1/8, 8], got {p}/{q}")
    if frames < 1:
        raise ValueError(f"at least one frame expected, got {frames}")
    if frames * p >= 1 << 62:
        raise ValueError(f"frames * p must stay below 2^62, got {frames} * {p}")


def phase_vocoder_len(frames: int, p: int, q: int) -> int:
    """host query: the frames ceil(frames q / p) of the output"""
    check_arguments(frames, p, q)
    n = int(_lib.load().mg_phase_vocoder_len(frames, p, q))
    if n < 0:
        raise ValueError(f"mg_phase_vocoder_len refuses frames {frames}, rate {p}/{q}")
    return n


def phase_vocoder(X: torch.Tensor, p: int, q: int, lock: bool = False) -> torch.Tensor:
    """X complex64 (512, T), rate p / q in [1/8, 8] -> complex64 (512, ceil(T q / p)): torchaudio.functional.phase_vocoder with
    phase_advance pi k / 2 (hop 256 of 1024), magnitudes and angles in float32 as torch takes them, the phase accumulated in float64
    modulo 2 pi; four launches (`mg_phase_vocoder`).  lock: identity phase locking (Laroche & Dolson 1999) -- every bin follows
    the nearest magnitude peak of its output frame and keeps the analysis frame's phase difference against it, so the bins of
    one partial stay together; five launches (`mg_phase_vocoder_locked`)"""
    if not isinstance(lock, bool):
        raise ValueError(f"lock must be True or False, got {lock!r}")
    if X.dim() != 2 or X.shape[0] != 512 or X.shape[1] < 1:
        raise ValueError(f"a (512, T >= 1) spectrum expected, got {tuple(X.shape)}")
    frames = X.shape[1]
    check_arguments(frames, p, q)
    if not X.is_cuda:
        raise _lib.MusicGanHipError("phase_vocoder: tensors on a ROCm GPU expected (no CPU fallback)")
    if X.dtype != torch.complex64 or not X.is_contiguous():
        raise _lib.MusicGanHipError(f"phase_vocoder: contiguous complex64 expected, got {X.dtype} contiguous={X.is_contiguous()}")
    lib = _lib.load()
    n = phase_vocoder_len(frames, p, q)
    ws_bytes, run, what = ((lib.mg_phase_vocoder_locked_ws_bytes, lib.mg_phase_vocoder_locked, "mg_phase_vocoder_locked") if lock else
                           (lib.mg_phase_vocoder_ws_bytes, lib.mg_phase_vocoder, "mg_phase_vocoder"))
    nbytes = int(ws_bytes(frames, p, q))
    if nbytes == 0:
        raise ValueError(f"phase_vocoder: {frames} frames at rate {p}/{q} are too many (2^31 frames and more)")
    ws = ops.workspace(nbytes, X.device)
    out = torch.empty((512, n, 2), dtype=torch.float32, device=X.device)
    check(run(_p(X), _p(out), _p(ws), nbytes, frames, p, q, _s()), what)
    return torch.view_as_complex(out)

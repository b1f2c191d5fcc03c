"""CPU restatement of the phase vocoder ("Phase vocoder") for the project's STFT (window 1024, hop 256, 512 rows) and a
rational rate p / q; the time axis is integer arithmetic everywhere: i0 = (t p) // q, alpha = ((t p) mod q) / q.

`literal`  torchaudio.functional.phase_vocoder's own sequence of operations: wrap(angle1 - angle0 - a_k) + a_k with a_k = pi k / 2,
           phase_0 in front, the last column dropped, cumsum, polar.  Its running sum reaches 8e6 rad at T = 8192.
`exact`    the same quantity modulo 2 pi: only the wrapped deviations are summed, a_k enters as (k mod 4) pi / 2 inside the wrap
           and as the exact factor i^(k t mod 4) outside; the sum is reduced modulo 2 pi before sine and cosine.
`mixed`    what the device computes: abs and angle by torch in float32 on the complex64 input, everything after them in float64 in
           the form of `exact`, the result rounded to complex64.  Its distance from `exact(float64)` on the same input is the `own`
           of the GPU tests' tolerance."""
import functools
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import griffinlim_ref as G  # noqa: E402  (the float64 STFT of the tonal inputs)

NB, HOP, N_FFT = 512, 256, 1024
TWO_PI = 2 * math.pi


def out_len(frames: int, p: int, q: int) -> int:
    return -((-frames * q) // p)


def _time_axis(frames, p, q, dtype):
    t = torch.arange(out_len(frames, p, q), dtype=torch.int64)
    tp = t * p
    return t, tp // q, (tp % q).to(dtype) / q


def _wrap(x):
    return x - TWO_PI * torch.round(x / TWO_PI)


def _gather(mag, ang, i0):
    """the values at frames i0 and i0 + 1 of (512, T) arrays taken as zero at frames T and T + 1"""
    mag = torch.nn.functional.pad(mag, [0, 2])
    ang = torch.nn.functional.pad(ang, [0, 2])
    return mag[:, i0], mag[:, i0 + 1], ang[:, i0], ang[:, i0 + 1]


def _cdtype(dtype):
    return torch.complex128 if dtype == torch.float64 else torch.complex64


def literal(X: torch.Tensor, p: int, q: int, dtype=torch.float64) -> torch.Tensor:
    X = X.to(_cdtype(dtype))
    _, i0, alpha = _time_axis(X.shape[1], p, q, dtype)
    advance = (math.pi * torch.arange(NB, dtype=dtype) / 2)[:, None]   # torchaudio's phase_advance = linspace(0, pi hop, 513)[:512]
    phase_0 = X[:, :1].angle()
    m0, m1, a0, a1 = _gather(X.abs(), X.angle(), i0)
    phase = _wrap(a1 - a0 - advance) + advance
    phase = torch.cat([phase_0, phase[:, :-1]], dim=-1)
    return torch.polar(alpha * m1 + (1 - alpha) * m0, torch.cumsum(phase, dim=-1))


def _exact_from_polar(mag, ang, p, q, dtype):
    t, i0, alpha = _time_axis(mag.shape[1], p, q, dtype)
    k = torch.arange(NB, dtype=torch.int64)[:, None]
    m0, m1, a0, a1 = _gather(mag, ang, i0)
    dev = _wrap(a1 - a0 - (k % 4).to(dtype) * (math.pi / 2))
    theta = ang[:, :1] + torch.cumsum(torch.cat([torch.zeros(NB, 1, dtype=dtype), dev[:, :-1]], dim=-1), dim=-1)
    out = torch.polar(alpha * m1 + (1 - alpha) * m0, _wrap(theta))
    units = torch.tensor([1, 1j, -1, -1j], dtype=out.dtype)
    return out * units[(k * t[None, :]) % 4]


def exact(X: torch.Tensor, p: int, q: int, dtype=torch.float64) -> torch.Tensor:
    X = X.to(_cdtype(dtype))
    return _exact_from_polar(X.abs(), X.angle(), p, q, dtype)


def mixed(X: torch.Tensor, p: int, q: int) -> torch.Tensor:
    assert X.dtype == torch.complex64
    return _exact_from_polar(X.abs().double(), X.angle().double(), p, q, torch.float64).to(torch.complex64)


# ---------------------------------------------------------------- inputs (complex64, (512, T))
@functools.lru_cache(maxsize=None)
def random_spectrum(frames: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(NB, frames, generator=g), torch.randn(NB, frames, generator=g))


@functools.lru_cache(maxsize=None)
def tonal_spectrum(frames: int, seed: int) -> torch.Tensor:
    """the float64 STFT of two sinusoids (440 Hz and 3520.5 Hz) plus 1 % noise"""
    g = torch.Generator().manual_seed(seed)
    tt = max(frames, 8)
    length = HOP * (tt - 1)
    t = torch.arange(length, dtype=torch.float64) / 44100.0
    wav = 0.5 * torch.sin(2 * np.pi * 440.0 * t) + 0.25 * torch.sin(2 * np.pi * 3520.5 * t + 1.0)
    wav = wav + 0.01 * torch.randn(length, generator=g, dtype=torch.float64)
    return G.stft(wav)[:, :frames].to(torch.complex64).contiguous()


@functools.lru_cache(maxsize=None)
def silent_spectrum(frames: int, seed: int) -> torch.Tensor:
    """digital silence: the first 3 and the last 2 frames and the rows 0 - 7 are exactly +0"""
    X = random_spectrum(frames, seed).clone()
    X[:, :3] = 0
    X[:, -2:] = 0
    X[:8] = 0
    return X


MAKERS = {"random": random_spectrum, "tonal": tonal_spectrum, "silence": silent_spectrum}


@functools.lru_cache(maxsize=None)
def case(kind: str, frames: int, p: int, q: int):
    """(X, exact float64, own, tol) of one parity case, computed once: tol = max(4 own, 1e-6 max|ref|)"""
    X = MAKERS[kind](frames, 1000 + frames)
    ref = exact(X, p, q, torch.float64)
    own = float((mixed(X, p, q).to(torch.complex128) - ref).abs().max())
    return X, ref, own, max(4 * own, 1e-6 * float(ref.abs().max()))

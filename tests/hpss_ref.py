"""CPU restatement of the harmonic / percussive separation and of the overlap-add re-timing for the project's STFT
(window 1024, hop 256, 512 rows), in NumPy / float64.

`medians`    H and P of |X|: `scipy.ndimage.median_filter(torch.abs(X).numpy(), size=.., mode='reflect')` along time and along
             frequency.  A median is a selection, so these are float32 values that the device must reproduce bit for bit.
`brute`      the same by reflecting every index (j -> r = j mod 2 n, r < n ? r : 2 n - 1 - r) and sorting the window: what pins the
             reading of mode='reflect', also where an axis is shorter than half the window and folds more than once.
`separate`   masks and products in float64 from those medians (librosa's softmask).
`ola`        y[256 m + j] = w[j] x[a_m + j] + w[j + 256] x[a_{m-1} + j + 256], a_m = floor(256 m p / q), a_{-1} = -256, x = 0 outside
             [0, L), w the periodic Hann window of 512 in float64; with dtype float32 the window is rounded once and the two
             products and the sum are float32 operations, as on the device.

Bounds (u = 2^-24, the rounding unit of float32; (1 + 2^-20) covers the terms of second order):
  MASK   the device forms B = fl(m P) [u], the quotients fl(A / Z) [u] and fl(B / Z) [2 u], their squares [3 u, 5 u], the sum
         [max + u = 6 u] and the quotient [3 u + 6 u + u]: a relative error of 10 u of a value <= 1 (power 1 has fewer steps).
         One of the quotients is exactly 1, so a + b >= 1 and an underflowing square only adds an absolute 2^-126.
  OUTPUT one more product per component: 11 u |X|.
  SUM    with both margins 1 the products m P are exact and the larger quotient and its square are exactly 1.  With r the other
         square [3 u]: the denominator fl(1 + r) is off by 3 u r + u (1 + r), relatively at most 2.5 u as r <= 1; the larger mask
         1 / (1 + r) by 3.5 u, the smaller r / (1 + r) <= 1/2 by 6.5 u; weighted with the masks, which sum to 1, at most 3.5 u + 3 u / 2
         = 5 u, and u more for the two products: 6 u |X|.
  OLA    against the float64 window: each term carries the rounding of w [u] and of its product [u], the sum one more [u of the
         result]: 3 u (|x1| + |x2|), stated as 2^-22 (|x1| + |x2|)."""
import functools
import math
import os
import sys

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import griffinlim_ref as G  # noqa: E402  (the float64 STFT of the tonal input)

NB, HOP, FRAME = 512, 256, 512
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
MASK_BOUND = 10 * U * SLACK + 2.0 ** -126
OUTPUT_FACTOR = 11 * U * SLACK          # times |X| at the bin (+ 2^-126)
SUM_FACTOR = 6 * U * SLACK              # times |X| at the bin
OLA_FACTOR = 2.0 ** -22                 # times |x1| + |x2| at the sample
TINY = float(np.finfo(np.float32).tiny)  # 2^-126


def reflect(j: int, n: int) -> int:
    r = j % (2 * n)
    return r if r < n else 2 * n - 1 - r


def medians(X: torch.Tensor, lh: int, lp: int):
    """(H, P) float32 arrays (512, T)"""
    S = torch.abs(X).numpy()
    assert S.dtype == np.float32
    return (ndimage.median_filter(S, size=(1, lh), mode="reflect"), ndimage.median_filter(S, size=(lp, 1), mode="reflect"))


def brute(X: torch.Tensor, lh: int, lp: int):
    S = torch.abs(X).numpy()
    nb, T = S.shape
    cols = np.array([[reflect(t + d, T) for d in range(-(lh // 2), lh // 2 + 1)] for t in range(T)])      # (T, lh)
    rows = np.array([[reflect(k + d, nb) for d in range(-(lp // 2), lp // 2 + 1)] for k in range(nb)])    # (512, lp)
    H = np.sort(S[:, cols], axis=2)[:, :, lh // 2]
    P = np.sort(S[rows, :], axis=1)[:, lp // 2, :]
    return H, P


def softmask(A, B, power, split: bool):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if power == math.inf:
        return (A > B).astype(np.float64)
    Z = np.maximum(A, B)
    bad = Z < TINY
    Z = np.where(bad, 1.0, Z)
    a, b = (A / Z) ** power, (B / Z) ** power
    return np.where(bad, 0.5 if split else 0.0, a / np.where(bad, 1.0, a + b))


def separate(X: torch.Tensor, kernel=(31, 31), power=2.0, margin=(1.0, 1.0)) -> dict:
    """{"H", "P" float32; "mask_h", "mask_p" float64; "harmonic", "percussive" complex128; "absX" float64}"""
    H, P = medians(X, *kernel)
    split = margin[0] == 1 and margin[1] == 1
    Hd, Pd = H.astype(np.float64), P.astype(np.float64)
    if power == math.inf:   # a comparison of float32 values, the product m P rounded once as the definition has it: exact
        mh, mp = (H > P * np.float32(margin[0])).astype(np.float64), (P > H * np.float32(margin[1])).astype(np.float64)
    else:
        mh, mp = softmask(Hd, Pd * margin[0], power, split), softmask(Pd, Hd * margin[1], power, split)
    Xd = X.to(torch.complex128).numpy()
    return {"H": H, "P": P, "mask_h": mh, "mask_p": mp, "harmonic": Xd * mh, "percussive": Xd * mp, "absX": np.abs(Xd)}


def window(dtype=np.float64):
    return (0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(FRAME, dtype=np.float64) / FRAME))).astype(dtype)


def ola(x, p: int, q: int, out_len: int, dtype=np.float64):
    """(y, |x1| + |x2|) of the definition; x a 1-D array"""
    x = np.asarray(x, dtype=dtype)
    L = x.shape[0]
    if out_len == 0:
        return np.zeros(0, dtype=dtype), np.zeros(0)
    n = np.arange(out_len, dtype=np.int64)
    m, j = n // HOP, n % HOP
    a = np.array([(HOP * v * p) // q for v in range(int(m.max()) + 1)], dtype=np.int64)   # Python integers: no overflow
    a0 = a[m]
    a1 = np.where(m == 0, -HOP, a[np.maximum(m - 1, 0)])
    w = window(dtype)

    def take(idx):
        ok = (idx >= 0) & (idx < L)
        return np.where(ok, x[np.clip(idx, 0, L - 1)], dtype(0))
    x1, x2 = take(a0 + j), take(a1 + j + HOP)
    y = w[j] * x1 + w[j + HOP] * x2
    assert y.dtype == dtype
    return y, np.abs(x1.astype(np.float64)) + np.abs(x2.astype(np.float64))


# ---------------------------------------------------------------- inputs (complex64, (512, T))
@functools.lru_cache(maxsize=None)
def random_spectrum(frames: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(NB, frames, generator=g), torch.randn(NB, frames, generator=g))


@functools.lru_cache(maxsize=None)
def tonal_clicks_spectrum(frames: int, seed: int) -> torch.Tensor:
    """the float64 STFT of two sinusoids (440 Hz and 3520.5 Hz), a click of height 0.8 every 4096 samples and 0.1 % noise: rows that
    are all tone, frames that are all click"""
    g = torch.Generator().manual_seed(seed)
    tt = max(frames, 8)
    length = HOP * (tt - 1)
    t = torch.arange(length, dtype=torch.float64) / 44100.0
    wav = 0.5 * torch.sin(2 * np.pi * 440.0 * t) + 0.25 * torch.sin(2 * np.pi * 3520.5 * t + 1.0)
    wav[1000::4096] += 0.8
    wav = wav + 0.001 * torch.randn(length, generator=g, dtype=torch.float64)
    return G.stft(wav)[:, :frames].to(torch.complex64).contiguous()


@functools.lru_cache(maxsize=None)
def silent_spectrum(frames: int, seed: int) -> torch.Tensor:
    return torch.zeros(NB, frames, dtype=torch.complex64)


MAKERS = {"random": random_spectrum, "tonal_clicks": tonal_clicks_spectrum, "silence": silent_spectrum}


@functools.lru_cache(maxsize=None)
def case(kind: str, frames: int, kernel=(31, 31), power=2.0, margin=(1.0, 1.0)):
    """(X, separate(X, ...)) of one case, computed once and shared; treat both as read-only"""
    X = MAKERS[kind](frames, 2000 + frames)
    return X, separate(X, kernel, power, margin)


@functools.lru_cache(maxsize=None)
def waveform(length: int, seed: int) -> torch.Tensor:
    """float32 noise in [-1, 1) with a click of height 3 every 97 samples"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(length, generator=g) * 2 - 1
    x[::97] = 3.0
    return x

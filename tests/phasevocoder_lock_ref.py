"""CPU restatement of the phase vocoder with identity phase locking ("Phase locking"; Laroche & Dolson 1999, III-C) on top
of tests/phasevocoder_ref.py: the same time axis, the same float32 |X| and arg X by torch, float64 from there on.

`mixed_locked`  the definition, frame after frame: the peaks of the interpolated magnitude, the nearest peak P_t(k) of every bin,
                s_t[k] = s_{t-1}[P] + dev[P, t-1] + (a[k, i0] - a[P, i0]), m4_t[k] = (m4_{t-1}[P] + P) mod 4.
`composed`      the same states from tiles of composed maps, the order of the device's additions: the map of every tile from the
                identity, the carry from tile to tile, the tiles again from their start.
Frame 0 is the step P = k, c = a[k, 0] without a quarter turn on the zero state, as the device stores it."""
import functools
import math
import os
import sys
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import griffinlim_ref as G  # noqa: E402
import phasevocoder_ref as R  # noqa: E402

NB, HOP = R.NB, R.HOP
TWO_PI, INV_TWO_PI, PI_2 = 6.283185307179586, 0.15915494309189535, 1.5707963267948966
UNITS = np.array([1, 1j, -1, -1j], dtype=np.complex128)

Locked = namedtuple("Locked", "out s m4 P c mag")   # out complex128 (512, n); the rest time-major (n, 512)


def wrap(x):
    """the device's reduction: x - 2 pi rint(x / 2 pi), the quotient taken as a product"""
    return x - TWO_PI * np.rint(x * INV_TWO_PI)


def peaks(mag: np.ndarray) -> np.ndarray:
    """(512,) float64 -> bool: above 0, above both lower neighbours, not below both upper ones; neighbours outside are skipped"""
    m = np.concatenate([[-np.inf, -np.inf], mag, [-np.inf, -np.inf]])
    c = m[2:-2]
    return (c > 0) & (c > m[1:-3]) & (c > m[:-4]) & (c >= m[3:-1]) & (c >= m[4:])


def regions(is_peak: np.ndarray) -> np.ndarray:
    """bool (512,) -> the nearest peak of every bin (a tie goes to the lower one); no peak: the bin itself"""
    k = np.arange(is_peak.shape[0])
    idx = np.flatnonzero(is_peak)
    if idx.size == 0:
        return k
    pos = np.searchsorted(idx, k, side="left")          # idx[pos] is the first peak at or above k
    hi = idx[np.minimum(pos, idx.size - 1)]
    lo = idx[np.maximum(pos - 1, 0)]
    return np.where(np.abs(k - lo) <= np.abs(hi - k), lo, hi)


def polar(X: torch.Tensor):
    """(|X|, arg X), float32, by torch's vector routine on EVERY element -- the bits the device restates (csrc/sleef_f32.h).  ATen
    sends the remainder elements at the end of every thread's chunk through libm's scalar atan2f / hypotf instead, an ulp off on some
    inputs, and here one ulp of an angle is more than the whole tolerance: one thread, the length padded to a multiple of 64."""
    flat = X.contiguous().reshape(-1)
    t = torch.cat([flat, torch.ones((-flat.numel()) % 64, dtype=X.dtype)])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        m, a = t.abs(), t.angle()
    finally:
        torch.set_num_threads(threads)
    return m[:flat.numel()].reshape(X.shape), a[:flat.numel()].reshape(X.shape)


def mixed_locked(X: torch.Tensor, p: int, q: int) -> Locked:
    assert X.dtype == torch.complex64 and X.shape[0] == NB
    T = X.shape[1]
    n = R.out_len(T, p, q)
    m32, a32 = polar(X)
    m = np.concatenate([m32.double().numpy(), np.zeros((NB, 2))], axis=1)
    a = np.concatenate([a32.double().numpy(), np.zeros((NB, 2))], axis=1)
    k = np.arange(NB)
    turn = (k % 4).astype(np.float64) * PI_2
    out = np.zeros((NB, n), dtype=np.complex128)
    S, M4, Ps, Cs, Ms = (np.zeros((n, NB)), np.zeros((n, NB), dtype=np.int64), np.zeros((n, NB), dtype=np.int64), np.zeros((n, NB)),
                         np.zeros((n, NB)))
    s, m4 = a[:, 0].copy(), np.zeros(NB, dtype=np.int64)
    for t in range(n):
        i0, alpha = (t * p) // q, ((t * p) % q) / q
        mag = (alpha * m[:, i0 + 1]) + ((1 - alpha) * m[:, i0])
        if t == 0:
            P, c = k, a[:, 0]
        else:
            P = regions(peaks(mag))
            j0 = ((t - 1) * p) // q
            dev = wrap((a[:, j0 + 1] - a[:, j0]) - turn)
            c = dev[P] + (a[:, i0] - a[P, i0])
            s = s[P] + c
            m4 = (m4[P] + P) % 4
        S[t], M4[t], Ps[t], Cs[t], Ms[t] = s, m4, P, c, mag
        out[:, t] = mag * np.exp(1j * wrap(s)) * UNITS[m4]
    return Locked(out, S, M4, Ps, Cs, Ms)


def composed(P: np.ndarray, c: np.ndarray, tile: int):
    """the states (s, m4), both (n, 512), of the steps (P, c) run as the device runs them, `tile` frames per composed map"""
    n = P.shape[0]
    k = np.arange(NB)
    inc = P % 4
    inc[0] = 0
    starts = [(np.zeros(NB), np.zeros(NB, dtype=np.int64))]
    for t0 in range(0, n - tile, tile):                  # every tile but the last
        pi, cc, mm = k, np.zeros(NB), np.zeros(NB, dtype=np.int64)
        for t in range(t0, t0 + tile):
            pi, cc, mm = pi[P[t]], cc[P[t]] + c[t], (mm[P[t]] + inc[t]) % 4
        s0, m0 = starts[-1]
        starts.append((s0[pi] + cc, (m0[pi] + mm) % 4))
    S, M4 = np.zeros((n, NB)), np.zeros((n, NB), dtype=np.int64)
    for j, (s, m4) in enumerate(starts):
        for t in range(j * tile, min(n, (j + 1) * tile)):
            s, m4 = s[P[t]] + c[t], (m4[P[t]] + inc[t]) % 4
            S[t], M4[t] = s, m4
    return S, M4


def additions(n: int, tile: int) -> int:
    """float64 additions on the two paths to a state of frame < n taken together: n sequential ones; at most `tile` inside a composed
    map, one per tile in the carry and `tile` in the tile run again -- bounded by n + tiles + n"""
    return 2 * n + -(-n // tile)


def state_bound(n: int, tile: int, s_max: float) -> float:
    """how far the composed states may lie from the sequential ones.  Both add the same steps c (computed once, bit-equal) in
    another order.  Every partial sum is a state or a difference of two states of one path, at most 2 max|s|, so each addition
    rounds by at most ulp(2 max|s|) / 2 = ulp(max|s|)."""
    return additions(n, tile) * float(np.spacing(s_max))


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def quantised_spectrum(frames: int, seed: int) -> torch.Tensor:
    """real and imaginary parts from {-2 .. 2}: equal magnitudes, plateaus and zeros in every frame"""
    g = torch.Generator().manual_seed(seed)
    re, im = (torch.randint(-2, 3, (NB, frames), generator=g).float() for _ in range(2))
    return torch.complex(re, im)


def zero_spectrum(frames: int, seed: int) -> torch.Tensor:
    return torch.zeros(NB, frames, dtype=torch.complex64)


MAKERS = {**R.MAKERS, "zero": zero_spectrum, "quantised": quantised_spectrum}


def frames_for(n: int, p: int, q: int) -> int:
    """the fewest input frames whose output has at least n frames (a rate gives only some lengths; rates above 1 give all)"""
    return ((n - 1) * p) // q + 1


@functools.lru_cache(maxsize=None)
def case(kind: str, frames: int, p: int, q: int):
    X = MAKERS[kind](frames, 2000 + frames)
    return X, mixed_locked(X, p, q)


# ---------------------------------------------------------------- the audible claim
def glide(hops: int = 511, seed: int = 3) -> torch.Tensor:
    """0.5 sin 2 pi (300 t + 40 t^2) plus 1 % noise, float64: constant amplitude, moving pitch"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(HOP * hops, dtype=torch.float64) / 44100.0
    return 0.5 * torch.sin(2 * math.pi * (300.0 * t + 40.0 * t * t)) + 0.01 * torch.randn(t.numel(), generator=g, dtype=torch.float64)


def ripple(wav) -> float:
    """std / mean of the RMS of 1024-sample windows at hop 256, 12 windows dropped at each end"""
    w = torch.as_tensor(wav).double().cpu().unfold(0, 1024, 256)
    rms = w.pow(2).mean(dim=1).sqrt()[12:-12]
    return float(rms.std() / rms.mean())


def stretch_locked(wav: torch.Tensor, p: int, q: int) -> torch.Tensor:
    """istft(mixed_locked(stft(wav))) in float64 from the complex64 spectrum"""
    return G.istft(torch.from_numpy(mixed_locked(G.stft(wav).to(torch.complex64), p, q).out))


def stretch_unlocked(wav: torch.Tensor, p: int, q: int) -> torch.Tensor:
    return G.istft(R.exact(G.stft(wav).to(torch.complex64), p, q, torch.float64))

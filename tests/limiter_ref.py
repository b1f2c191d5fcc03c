"""Float64 numpy restatement of the look-ahead true-peak limiter ("True-peak limiter", steps 1 - 6) and of the loop of
`normalize_loudness(limiter=True)`.  It takes nothing from the code under test: the release is the plain sequential recurrence, the
hold and the mean are direct windows, the envelope is the float64 evaluation of the interpolation bank of tests/loudness_ref.py.
The gain curve can be computed from a given envelope m (the device's float32 one, which the tests check on its own), so that the
1e-8 bound on g does not have to carry the 1e-6 of a float32 interpolation sum."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as R  # noqa: E402


def interpolate4(x):
    """x (C, L) -> u (C, 4 L) float64: u[4 n + j] as resample(x, 1, 4) writes it, zeros beyond both ends"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    h, w = R.bank_1_to_4()
    xp = np.pad(x, ((0, 0), (w, w + 1)))
    win = np.lib.stride_tricks.sliding_window_view(xp, h.shape[1], axis=1)[:, :x.shape[1]]
    return np.einsum("clk,pk->clp", win, h).reshape(x.shape[0], -1)


def neighbourhood_max(ax, au):
    """ax (C, L) = |x|, au (C, 4 L) = |u| -> m (L,): max over the channels of max(ax[n], au[4n - 3 .. 4n + 3]), ends not counted"""
    channels, length = ax.shape
    pad = np.pad(au, ((0, 0), (3, 3)))                                     # au[k] = pad[k + 3]; k = 4n - 3 .. 4n + 3 -> pad[4n .. 4n + 6]
    win = np.lib.stride_tricks.sliding_window_view(pad, 7, axis=1)[:, ::4][:, :length]
    return np.maximum(ax, win.max(axis=2)).max(axis=0)


def envelope(x):
    """step 1 in float64"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    return neighbourhood_max(np.abs(x), np.abs(interpolate4(x)))


def required_gain(m, G, c):
    """step 2: r over the samples of the file"""
    e = float(G) * np.asarray(m, dtype=np.float64)
    r = np.ones_like(e)
    over = e > c
    r[over] = c / e[over]
    return r


def gain_curve(m, G, c, A, rho):
    """steps 2 - 5 -> dict(r, h, d, q, g): r and g over n = 0 .. L - 1, h, d and q over n = -A .. L - 1 (index n + A)"""
    m = np.asarray(m, dtype=np.float64)
    length = m.shape[0]
    r = required_gain(m, G, c)
    ext = np.concatenate([np.ones(A), r, np.ones(A)])                      # r over n = -A .. L - 1 + A
    h = np.lib.stride_tricks.sliding_window_view(ext, A + 1).min(axis=1)   # h[n] = min r[n .. n + A], n = -A .. L - 1
    assert h.shape[0] == length + A
    d = np.empty(length + A)
    state = 0.0
    for i, u in enumerate(1.0 - h):
        state = max(u, rho * state)
        d[i] = state
    q = 1.0 - d
    mean = np.lib.stride_tricks.sliding_window_view(q, A + 1).sum(axis=1) / (A + 1)   # q[n - A .. n], n = 0 .. L - 1
    assert mean.shape[0] == length
    return dict(r=r, h=h, d=d, q=q, g=np.minimum(r, mean))


def release_closed_form(h, rho, span):
    """d[n] = max_{0 <= k <= span} rho^k (1 - h[n - k]) (zeros before the start): the recurrence unrolled"""
    u = 1.0 - np.asarray(h, dtype=np.float64)
    d = u.copy()
    for k in range(1, span + 1):
        d[k:] = np.maximum(d[k:], rho ** k * u[:-k])
    return d


def limit(x, G, c, A, rho, m=None):
    """-> (y float32 (C, L), g float64 (L,)); m: the envelope to use (default: this file's)"""
    x = np.atleast_2d(x)
    g = gain_curve(envelope(x) if m is None else m, G, c, A, rho)["g"]
    return ((x.astype(np.float64) * float(G)) * g[None, :]).astype(np.float32), g


def parameters(fs, peak_dbtp=-1.0, attack_ms=5.0, release_ms=50.0):
    """-> (c, A, rho)"""
    return 10.0 ** (peak_dbtp / 20.0), int(round(attack_ms * fs / 1000.0)), float(np.exp(-1.0 / (release_ms * fs / 1000.0)))


def normalize(x, fs, target, peak_dbtp=-1.0, attack_ms=5.0, release_ms=50.0, passes=2, m=None):
    """the loop of normalize_loudness(limiter=True) -> dict(out, lufs, peak_dbtp, reduction_db, pregain, static_lufs): `static_lufs`
    is what the one-gain rule min(10^((target - L) / 20), c / true_peak) delivers"""
    x = np.atleast_2d(x)
    c, A, rho = parameters(fs, peak_dbtp, attack_ms, release_ms)
    m = envelope(x) if m is None else m
    l0 = R.loudness(x, fs)["lufs"]
    G = 10.0 ** ((target - l0) / 20.0) if np.isfinite(l0) else 1.0
    for i in range(passes):
        if i > 0:
            li = R.loudness(y, fs)["lufs"]
            if np.isfinite(li):
                G *= 10.0 ** ((target - li) / 20.0)
        y, g = limit(x, G, c, A, rho, m=m)
    t = min(1.0, c / R.true_peak(y))
    out = (y.astype(np.float64) * t).astype(np.float32)
    static = min(10.0 ** ((target - l0) / 20.0), c / R.true_peak(x)) if np.isfinite(l0) else 1.0
    return dict(out=out, lufs=R.loudness(out, fs)["lufs"], peak_dbtp=R.db(R.true_peak(out)), reduction_db=-R.db(g.min()), pregain=G,
                static_lufs=l0 + R.db(static))


def prototype_signal(seed=0, fs=44100, seconds=2.0):
    """a 220 Hz sine at 0.2, Gaussian noise at 0.1 and 200 spikes of N(0, 0.8^2) at random places: (1, L) float32"""
    rng = np.random.default_rng(seed)
    n = int(fs * seconds)
    x = 0.2 * np.sin(2.0 * np.pi * 220.0 * np.arange(n) / fs) + 0.1 * rng.standard_normal(n)
    x[rng.integers(0, n, 200)] += 0.8 * rng.standard_normal(200)
    return x.astype(np.float32)[None, :]

"""Float64 numpy restatement of the loudness definitions (ITU-R BS.1770-4 / EBU R128, DESIGN.md "Loudness"), with
scipy.signal.lfilter for the K-weighting filter.  It takes nothing from the code under test: its own coefficient formulas (the analog
prototypes of libebur128 / pyloudnorm) and its own interpolation bank (torchaudio's published kernel expression for 1 -> 4)."""
import numpy as np
from scipy.signal import lfilter

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
BS1770_SHELF_B = (1.53512485958697, -2.69169618940638, 1.19839281085285)
BS1770_SHELF_A = (-1.69065929318241, 0.73248077421585)
BS1770_HIGHPASS_A = (-1.99004745483398, 0.99007225036621)


def coefficients(fs):
    """((b, a), (b, a)): shelf stage, high-pass stage"""
    f0, g, q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k = np.tan(np.pi * f0 / fs)
    vh = np.power(10.0, g / 20.0)
    vb = np.power(vh, 0.4996667741545416)
    a0 = 1.0 + k / q + k * k
    b1 = np.array([vh + vb * k / q + k * k, 2.0 * (k * k - vh), vh - vb * k / q + k * k]) / a0
    a1 = np.array([1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0])
    f0, q = 38.13547087602444, 0.5003270373238773
    k = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + k / q + k * k
    a2 = np.array([1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0])
    return (b1, a1), (np.array([1.0, -2.0, 1.0]), a2)


def segment_length(fs):
    return (fs + 5) // 10


def kweight(x, fs):
    """x (C, L) -> the K-weighted signal, float64, zero initial state"""
    (b1, a1), (b2, a2) = coefficients(fs)
    return lfilter(b2, a2, lfilter(b1, a1, np.asarray(x, dtype=np.float64), axis=-1), axis=-1)


def segment_energies(x, fs):
    """x (C, L) -> S (C, L // seg) float64"""
    x = np.atleast_2d(x)
    seg = segment_length(fs)
    nseg = x.shape[1] // seg
    y = kweight(x, fs)[:, :nseg * seg]
    return np.sum(y.reshape(x.shape[0], nseg, seg) ** 2, axis=2)


def gate(S, fs, weights=None):
    """S (C, nseg) -> dict(lufs, momentary_max, n_abs, n_rel, l, gamma): l the block loudnesses, gamma the relative gate"""
    S = np.asarray(S, dtype=np.float64)
    channels, nseg = S.shape
    seg = segment_length(fs)
    g = np.ones(channels) if weights is None else np.asarray(weights, dtype=np.float64)
    if nseg < 4:
        return dict(lufs=-np.inf, momentary_max=-np.inf, n_abs=0, n_rel=0, l=np.zeros(0), gamma=-np.inf)
    blocks = S[:, 0:nseg - 3] + S[:, 1:nseg - 2] + S[:, 2:nseg - 1] + S[:, 3:nseg]
    z = (g[:, None] * blocks).sum(axis=0) / (4.0 * seg)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    keep = l > -70.0
    if not keep.any():
        return dict(lufs=-np.inf, momentary_max=float(l.max()), n_abs=0, n_rel=0, l=l, gamma=-np.inf)
    gamma = -0.691 + 10.0 * np.log10(z[keep].mean()) - 10.0
    both = keep & (l > gamma)
    return dict(lufs=float(-0.691 + 10.0 * np.log10(z[both].mean())), momentary_max=float(l.max()), n_abs=int(keep.sum()),
                n_rel=int(both.sum()), l=l, gamma=float(gamma))


def loudness(x, fs, weights=None):
    return gate(segment_energies(x, fs), fs, weights)


def bank_1_to_4(lowpass_filter_width=6, rolloff=0.99):
    """torchaudio's _get_sinc_resample_kernel for orig = 1, new = 4 (sinc_interp_hann) in float64: (4, 2 w + 1) and w"""
    orig, new = 1, 4
    base = min(orig, new) * rolloff
    w = int(np.ceil(lowpass_filter_width * orig / base))
    idx = np.arange(-w, w + orig, dtype=np.float64)[None, :] / orig
    t = (np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx) * base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * np.pi / lowpass_filter_width / 2.0) ** 2
    t = t * np.pi
    scale = base / orig
    k = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t))
    return k * window * scale, w


def true_peak(x):
    """x (C, L) -> max over channels of max(max |x|, max |u|), u the 4x interpolation with zero extension beyond both ends, float64"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    h, w = bank_1_to_4()            # (4, 2 w + 1): torchaudio's kernel has 2 w + orig taps and pads by (w, w + orig)
    taps = h.shape[1]
    xp = np.pad(x, ((0, 0), (w, w + 1)))
    length = x.shape[1]
    win = np.lib.stride_tricks.sliding_window_view(xp, taps, axis=1)[:, :length]   # (C, L, taps): window T = xp[T .. T + taps)
    u = np.einsum("clk,pk->clp", win, h)
    return float(max(np.abs(x).max(), np.abs(u).max()))


def quarter_rate_sine(length, fade=500):
    """sin(2 pi n / 4 + pi / 4), float64: every sample falls 45 degrees off a crest, so the sample peak is 3.01 dB below the
    amplitude 1.  Both ends rise over `fade` samples (half a Hann window): a sine that starts at once overshoots there."""
    x = np.sin(2.0 * np.pi * np.arange(length) / 4.0 + np.pi / 4.0)
    ramp = np.hanning(2 * fade + 1)[:fade]
    x[:fade] *= ramp
    x[length - fade:] *= ramp[::-1]
    return x


def db(v):
    return 20.0 * np.log10(v) if v > 0 else -np.inf


def stereo_sine(fs, parts, freq=1000.0):
    """parts: [(dBFS, seconds)] -> (2, L) float32: one phase-continuous sine whose amplitude steps, the same in both channels"""
    n = [int(round(s * fs)) for _, s in parts]
    t = np.arange(sum(n)) / fs
    amp = np.concatenate([np.full(k, 10.0 ** (d / 20.0)) for (d, _), k in zip(parts, n)])
    x = (amp * np.sin(2.0 * np.pi * freq * t)).astype(np.float32)
    return np.stack([x, x])


# EBU Tech 3341, cases 1, 3, 4, 5: stereo 1 kHz sines at 48 kHz, each -23.0 +- 0.1 LUFS
TECH3341 = {
    1: [(-23.0, 20.0)],
    3: [(-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0)],
    4: [(-72.0, 10.0), (-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0), (-72.0, 10.0)],
    5: [(-26.0, 20.0), (-20.0, 20.1), (-26.0, 20.0)],
}
# the gates of cases 3 and 4 on a few seconds
SHORT_GATES = {
    "3-short": [(-36.0, 1.0), (-23.0, 2.0), (-36.0, 1.0)],
    "4-short": [(-72.0, 0.5), (-36.0, 0.5), (-23.0, 2.0), (-36.0, 0.5), (-72.0, 0.5)],
}

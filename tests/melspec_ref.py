"""Float64 numpy restatements of DESIGN.md 4.21, the yardsticks of test_melspec_cpu.py and test_melspec_gpu.py: the framed
1024 / 256 transform (reflect padding by 512, periodic Hann / sqrt(384), np.fft.rfft, bins 0 .. 511), the mel power under a bank
given as float32 weights (taken exactly), the windows and the pooled log rows, and the codec's inverse in float64.  The `*_f32`
functions evaluate the same chains in float32 on the CPU: what a correct float32 evaluation gives, for the tolerances.  No GPU, no
musicgan_amd import."""
import numpy as np

N_FFT, HOP, BINS = 1024, 256, 512


def window(dtype=np.float64) -> np.ndarray:
    """periodic Hann / sqrt(sum w^2); sum w^2 = 384"""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT)
    return (w / np.sqrt(384.0)).astype(dtype)


def frame_count(length: int) -> int:
    return 1 + length // HOP


def frames(wave: np.ndarray) -> np.ndarray:
    """(L,) -> (T, 1024): frame t holds xpad[256 t .. 256 t + 1023], xpad = reflect-pad(x, 512)"""
    xp = np.pad(wave, (N_FFT // 2, N_FFT // 2), mode="reflect")
    idx = np.arange(N_FFT)[None, :] + HOP * np.arange(frame_count(wave.shape[0]))[:, None]
    return xp[idx]


def stft(wave: np.ndarray, dtype=np.float64) -> np.ndarray:
    """(L,) -> complex (512, T) in `dtype`'s precision (numpy's pocketfft runs float32 input in float32)"""
    f = frames(np.asarray(wave, dtype=dtype)) * window(dtype)[None, :]
    spec = np.fft.rfft(f, axis=1)
    assert spec.dtype == (np.complex128 if dtype == np.float64 else np.complex64), spec.dtype
    return spec[:, :BINS].T


def band_sums(p: np.ndarray, weight: np.ndarray, lo, hi) -> np.ndarray:
    """p (512, T), weight (M, 512) -> (M, T) in p's type: ascending k, product and sum rounded apart, an empty band +0.0"""
    out = np.zeros((weight.shape[0], p.shape[1]), dtype=p.dtype)
    w = weight.astype(p.dtype)
    for m in range(weight.shape[0]):
        s = np.zeros(p.shape[1], dtype=p.dtype)
        for k in range(lo[m], hi[m]):
            s = s + w[m, k] * p[k]
        out[m] = s
    return out


def power_of_bins(x: np.ndarray) -> np.ndarray:
    """complex (512, T) -> re re + im im in the component type, the two products and the sum rounded apart"""
    re, im = x.real, x.imag
    return re * re + im * im


def mel_power(waves: np.ndarray, weight: np.ndarray, lo, hi, dtype=np.float64) -> np.ndarray:
    """(B, L) float32 samples -> (B, M, T) in `dtype`"""
    return np.stack([band_sums(power_of_bins(stft(w, dtype)), weight, lo, hi) for w in np.asarray(waves)])


def mel_power_f32(waves, weight, lo, hi) -> np.ndarray:
    return mel_power(waves, weight, lo, hi, np.float32)


def band_scale(waves: np.ndarray, weight: np.ndarray, lo, hi) -> np.ndarray:
    """(M,): the largest sum of |w| p of a band over the rows and frames of a case, in float64 -- what an error of the band is
    measured against"""
    absw = np.abs(np.where(np.isnan(weight), 0.0, weight.astype(np.float64))).astype(np.float32)
    return mel_power(waves, absw, lo, hi).max(axis=(0, 2))


def window_count(frames_: int, win: int, hop: int) -> int:
    return (frames_ - win) // hop + 1 if frames_ >= win else 0


def logmel_pool(power: np.ndarray, win: int, hop: int, pools: int, floor: float) -> np.ndarray:
    """(B, M, T) float32 or float64 -> (B W, M pools) float64: the mean of log(power + floor) over the win / pools frames of a pool"""
    power = np.asarray(power, dtype=np.float64)
    b, m, t = power.shape
    w = window_count(t, win, hop)
    assert w >= 1 and win % pools == 0
    out = np.empty((b, w, m, pools))
    for n in range(w):
        v = np.log(power[:, :, n * hop:n * hop + win] + floor)
        out[:, n] = v.reshape(b, m, pools, win // pools).mean(3)
    return out.reshape(b * w, m * pools)


def wave_logmel(waves, weight, lo, hi, win, hop, pools, floor, dtype=np.float64) -> np.ndarray:
    """the whole chain: float32 or float64 up to the band sums, float64 from the logarithm on (as the kernels)"""
    return logmel_pool(mel_power(waves, weight, lo, hi, dtype), win, hop, pools, floor)


# ------------------------------------------------------------------ the codec's inverse in float64
def bark_vector() -> np.ndarray:
    f = np.linspace(20.0, 22050.0, BINS)
    s = 6.0 * np.arcsinh(f / 600.0)
    return s / np.sqrt(np.sum(s * s))


def istft(z: np.ndarray) -> np.ndarray:
    """complex128 (513, T) -> (256 (T - 1),) float64: overlap-add of the windowed inverse frames over the window envelope"""
    w = window() * np.sqrt(384.0)
    t = z.shape[1]
    fr = np.fft.irfft(z.T * np.sqrt(384.0), n=N_FFT, axis=1) * w[None, :]
    total = N_FFT + HOP * (t - 1)
    y, env = np.zeros(total), np.zeros(total)
    for i in range(t):
        y[i * HOP:i * HOP + N_FFT] += fr[i]
        env[i * HOP:i * HOP + N_FFT] += w * w
    return y[N_FFT // 2:total - N_FFT // 2] / env[N_FFT // 2:total - N_FFT // 2]


def magn_phase_to_wave(image: np.ndarray) -> np.ndarray:
    """one (2, 512, W) float32 image -> (256 (W - 1),) float64: magnitude (x + 1) / 2 / bark / (max - min), phase the running sum
    of ((x + 1) / 2 * 2 pi - pi), Nyquist row 0 -- the codec's inverse with every operation in float64"""
    x = np.asarray(image, dtype=np.float64)
    magn = (x[0] + 1.0) / 2.0 / bark_vector()[:, None]
    magn = magn / (magn.max() - magn.min())
    phase = np.cumsum((x[1] + 1.0) / 2.0 * 2.0 * np.pi - np.pi, axis=1)
    z = np.concatenate([magn * np.exp(1j * phase), np.zeros((1, x.shape[2]), dtype=np.complex128)], axis=0)
    return istft(z)

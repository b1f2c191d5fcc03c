"""CPU restatement of the Griffin-Lim definition ("Griffin-Lim") with torch.stft / torch.istft, in float64 by default; the
same loop runs in float32 (`dtype`) and its distance from the float64 run is the yardstick of the GPU tests' tolerances.

STFT / ISTFT are the project's (and torchaudio's `normalized=True`): centre reflect padding, periodic Hann(1024), hop 256, division
by sqrt(sum w^2) = sqrt(384).  torch.stft's own `normalized` flag divides by sqrt(n_fft) instead, so it stays off here and the
factor is applied explicitly -- with it the n_iter = 0 result is oracle.audio's inverse (tests/test_griffinlim_cpu.py).  A zero
Nyquist row is appended for the inverse; the forward drops it again.  M and Z0 restate the reference's
music_gan/audio/functions.py:108-123 (oracle.audio.magn_phase_to_wav, same lines) in `dtype`."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import audio as oracle_audio  # noqa: E402

N_FFT, HOP, NB = 1024, 256, 512
SCALE = math.sqrt(384.0)   # sqrt(sum of hann^2 over 1024)


def _window(dtype):
    return torch.hann_window(N_FFT, periodic=True, dtype=torch.float64).to(dtype)


def stft(wav: torch.Tensor) -> torch.Tensor:
    """[256 (TT - 1)] -> complex (512, TT)"""
    c = torch.stft(wav, N_FFT, hop_length=HOP, win_length=N_FFT, window=_window(wav.dtype), center=True, pad_mode="reflect",
                   normalized=False, onesided=True, return_complex=True)
    return (c / SCALE)[:-1]


def istft(Z: torch.Tensor) -> torch.Tensor:
    """complex (512, TT) -> [256 (TT - 1)]; the imaginary part of DC is ignored (irfft), the Nyquist row is zero"""
    real = torch.float64 if Z.dtype == torch.complex128 else torch.float32
    full = torch.cat([Z, torch.zeros(1, Z.shape[1], dtype=Z.dtype)], dim=0) * SCALE
    return torch.istft(full, N_FFT, hop_length=HOP, win_length=N_FFT, window=_window(real), center=True, normalized=False,
                       onesided=True, length=HOP * (Z.shape[1] - 1))


def spectrum(mp: torch.Tensor, init: str = "phase", dtype=torch.float64):
    """(N, 2, 512, W) float32 -> (M, Z0) in `dtype`; the cumulative phase is the reference's sequential sum"""
    cdtype = torch.complex128 if dtype == torch.float64 else torch.complex64
    x = mp.to(dtype)
    magn = x.permute(1, 2, 0, 3).flatten(2, 3)[0]
    phase = x.permute(1, 2, 0, 3).flatten(2, 3)[1]
    bark = torch.from_numpy(oracle_audio.bark_scale_vector(NB, "torch")).to(dtype)
    magn = (magn + 1.) / 2. / bark[:, None]
    magn = magn / (magn.max() - magn.min())
    if init == "zero":
        return magn, torch.complex(magn, torch.zeros_like(magn)).to(cdtype)
    assert init == "phase", init
    two_pi = torch.tensor(2 * np.pi, dtype=dtype)
    phase = (phase + 1.) / 2. * 2. * torch.tensor(np.pi, dtype=dtype) - torch.tensor(np.pi, dtype=dtype)
    phase = torch.cumsum(phase, dim=1) if dtype == torch.float64 else torch.from_numpy(np.cumsum(phase.numpy(), axis=1, dtype=np.float32))
    phase = torch.remainder(phase, two_pi)
    return magn, torch.complex(magn * torch.cos(phase), magn * torch.sin(phase)).to(cdtype)


def project(R, tprev, M, momentum: float):
    """one magnitude projection: (Z, c) from R, the previous R (None: zero) and M"""
    mu = momentum / (1.0 + momentum)
    c = R if tprev is None else R - tprev * torch.tensor(mu, dtype=M.dtype)
    return M * (c / (c.abs() + 1e-16)), c


def loop(M, Z0, n_iter: int, momentum: float, trace: bool = False):
    """the definition: returns (wav, convergence [n_iter] float64, Z after the last projection[, per-iteration (R, c, Z)])"""
    Z, tprev, conv, steps = Z0, None, [], []
    for _ in range(n_iter):
        R = stft(istft(Z))
        Z, c = project(R, tprev, M, momentum)
        tprev = R
        conv.append(float(torch.linalg.norm((R.abs() - M).double()) / torch.linalg.norm(M.double())))
        if trace:
            steps.append((R, c, Z))
    out = (istft(Z), torch.tensor(conv, dtype=torch.float64), Z)
    return out + (steps,) if trace else out


def griffin_lim(mp: torch.Tensor, n_iter: int, momentum: float, init: str = "phase", dtype=torch.float64):
    M, Z0 = spectrum(mp, init, dtype)
    return loop(M, Z0, n_iter, momentum)


def random_images(n: int, w: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 2, NB, w, generator=g) * 2 - 1


def tone_images(n: int, w: int, seed: int) -> torch.Tensor:
    """the codec's forward output (oracle.audio) for two sinusoids plus noise: n images of w frames.  The noise stands at a tenth of
    the louder sinusoid: it sets how many bins hold next to nothing, and with 0.01 the float64 loop started from zero phase itself
    has 0.15 % of its bins below the conditioning threshold of the projection test (1e-3 mean M), with 0.05 at most 0.05 %."""
    g = torch.Generator().manual_seed(seed)
    length = HOP * (n * w + 1)
    t = torch.arange(length, dtype=torch.float64) / 44100.0
    wav = 0.5 * torch.sin(2 * np.pi * 440.0 * t) + 0.25 * torch.sin(2 * np.pi * 3520.0 * t + 1.0)
    wav = (wav + 0.05 * torch.randn(length, generator=g, dtype=torch.float64)).float().numpy()
    magn, phase = oracle_audio.stft_to_phase_magn(oracle_audio.stft(wav), nb_vec=w)
    assert magn.shape == (n, NB, w), magn.shape
    return torch.from_numpy(np.stack([magn, phase], axis=1)).contiguous()

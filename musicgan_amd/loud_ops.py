"""Tensor-level wrappers over the loudness entries of the C ABI (include/musicgan_hip.h, csrc/loudness.hip): K-weighted segment
energies, the BS.1770 gates, true peak, and the gain that brings a waveform to a target.  Waveforms are float32 (C, L) with C <= 8
and unit stride along L (any row stride).  Every call is asynchronous on the caller's current stream and synchronises nothing: the
measurements stay in device memory, and so does the gain between measurement and scaling.  Scratch memory comes from `ops.workspace`
(one buffer per device and stream, shared with the other op modules).  No fallback path exists: non-GPU tensors raise."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib, ops
from ._lib import check
from .ops import _p, _s

CHUNK = 1024                  # samples per chunk of the carried filter state (CHUNK of csrc/loudness.hip, mg_loudness_chunk)
MAX_CHANNELS = 8


def check_sample_rate(sample_rate) -> int:
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or not 0 < sample_rate < 1 << 30:
        raise ValueError(f"sample_rate must be a positive integer, got {sample_rate!r}")
    return sample_rate


def segment_length(sample_rate: int) -> int:
    """the samples of 100 ms, the step of the gating blocks"""
    return (check_sample_rate(sample_rate) + 5) // 10


def _biquad(k: float, q: float, b):
    a0 = 1.0 + k / q + k * k
    return [v / a0 for v in b], [1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]


def kweighting_coefficients(sample_rate: int):
    """((b, a), (b, a)): the shelf and the high-pass stage of the K-weighting filter at `sample_rate` as lists of three float64
    numbers each (a[0] = 1), from the analog prototypes of libebur128 / pyloudnorm; at 48 kHz the table of BS.1770-4.  Host only."""
    fs = float(check_sample_rate(sample_rate))
    f0, gain_db, q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k = math.tan(math.pi * f0 / fs)
    vh = 10.0 ** (gain_db / 20.0)
    vb = vh ** 0.4996667741545416
    shelf = _biquad(k, q, [vh + vb * k / q + k * k, 2.0 * (k * k - vh), vh - vb * k / q + k * k])
    f0, q = 38.13547087602444, 0.5003270373238773
    k = math.tan(math.pi * f0 / fs)
    _, a = _biquad(k, q, [1.0, -2.0, 1.0])
    return shelf, ([1.0, -2.0, 1.0], a)


def check_waveform(x: torch.Tensor) -> None:
    """the argument errors of a waveform, raised before anything touches the device"""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"a waveform (channels, samples) expected, got {tuple(x.shape) if isinstance(x, torch.Tensor) else x!r}")
    if not 1 <= x.shape[0] <= MAX_CHANNELS:
        raise ValueError(f"1 .. {MAX_CHANNELS} channels expected, got {x.shape[0]}")
    if not x.is_floating_point():
        raise ValueError(f"a floating-point waveform expected, got {x.dtype}")


def check_weights(channel_weights, channels: int):
    """None (1.0 each) or one finite non-negative number per channel -> a list of floats"""
    if channel_weights is None:
        return [1.0] * channels
    w = [float(v) for v in channel_weights]
    if len(w) != channels:
        raise ValueError(f"channel_weights must hold one weight per channel ({channels}), got {len(w)}")
    if any(not math.isfinite(v) or v < 0 for v in w):
        raise ValueError(f"channel_weights must be finite and not negative, got {w}")
    return w


def _chk(name: str, x: torch.Tensor) -> None:
    check_waveform(x)
    if not x.is_cuda:
        raise _lib.MusicGanHipError(f"{name}: tensors on a ROCm GPU expected (no CPU fallback)")
    if x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise _lib.MusicGanHipError(f"{name}: float32 (C, L) with unit stride along L expected, got {x.dtype} strides {x.stride()}")


def segment_energies(x: torch.Tensor, sample_rate: int) -> torch.Tensor:
    """x float32 (C, L) -> S float64 (C, L // seg): the sum of squares of the K-weighted channel over every whole 100 ms segment
    (seg = segment_length(sample_rate)); the filter starts from zero state at sample 0, state and sums are float64, the tail is
    dropped.  Four launches (`mg_loudness_energy`); the same bits on every run."""
    seg = segment_length(sample_rate)
    _chk("segment_energies", x)
    channels, length = x.shape
    (b1, a1), (b2, a2) = kweighting_coefficients(sample_rate)
    coef = (ctypes.c_double * 10)(*b1, a1[1], a1[2], *b2, a2[1], a2[2])
    out = torch.empty((channels, length // seg), dtype=torch.float64, device=x.device)
    if out.numel() == 0:
        return out
    lib = _lib.load()
    nbytes = int(lib.mg_loudness_ws_bytes(channels, length, seg))
    if nbytes == 0:
        raise ValueError(f"segment_energies: {length} samples are too many")
    ws = ops.workspace(nbytes, x.device)
    check(lib.mg_loudness_energy(_p(x), channels, length, x.stride(0), seg, coef, _p(out), _p(ws), nbytes, _s()), "mg_loudness_energy")
    return out


def gate(energies: torch.Tensor, sample_rate: int, channel_weights=None) -> torch.Tensor:
    """S float64 (C, nseg) of `segment_energies` -> the record, float64 (4,): integrated loudness in LUFS (-inf below four segments
    or with no block above -70 LUFS), the momentary maximum, the blocks above the absolute gate, the blocks above both gates.  One
    launch, one workgroup (`mg_loudness_gate`)."""
    seg = segment_length(sample_rate)
    if energies.dim() != 2 or not 1 <= energies.shape[0] <= MAX_CHANNELS:
        raise ValueError(f"energies (C <= {MAX_CHANNELS}, segments) expected, got {tuple(energies.shape)}")
    w = check_weights(channel_weights, energies.shape[0])
    if not energies.is_cuda or energies.dtype != torch.float64 or not energies.is_contiguous():
        raise _lib.MusicGanHipError("gate: contiguous float64 energies on a ROCm GPU expected (no CPU fallback)")
    record = torch.empty((4,), dtype=torch.float64, device=energies.device)
    check(_lib.load().mg_loudness_gate(_p(energies), (ctypes.c_double * len(w))(*w), energies.shape[0], energies.shape[1], seg,
                                       _p(record), _s()), "mg_loudness_gate")
    return record


def true_peak(x: torch.Tensor) -> torch.Tensor:
    """x float32 (C, L >= 1) -> float32 0-dim: the largest magnitude among the samples and their 4x interpolation with the bank
    of `ops.resample_rows(x, 1, 4)` (Hann-windowed sinc, 4 phases x 15 taps, zeros beyond both ends), linear.  The interpolated
    signal is never written; two launches (`mg_true_peak`)."""
    _chk("true_peak", x)
    channels, length = x.shape
    if length < 1:
        raise ValueError("true_peak: at least one sample expected")
    lib = _lib.load()
    bank = ops.resample_bank(1, 4, 6, 0.99, x.device)
    nbytes = int(lib.mg_true_peak_ws_bytes(channels, length))
    ws = ops.workspace(nbytes, x.device)
    out = torch.empty((1,), dtype=torch.float32, device=x.device)
    check(lib.mg_true_peak(_p(x), channels, length, x.stride(0), _p(bank), bank.numel(), _p(out), _p(ws), nbytes, _s()), "mg_true_peak")
    return out[0]


def check_targets(target_lufs, peak_dbtp):
    out = []
    for name, v in (("target_lufs", target_lufs), ("peak_dbtp", peak_dbtp)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
        out.append(float(v))
    return out


def normalize(x: torch.Tensor, record: torch.Tensor, peak: torch.Tensor, target_lufs: float, peak_dbtp: float):
    """x float32 contiguous, record of `gate`, peak of `true_peak` -> (x * gain, gain float32 0-dim) with
    gain = min(10^((target_lufs - record[0]) / 20), 10^(peak_dbtp / 20) / peak), computed in float64 on the device and rounded once;
    1 where record[0] is -inf.  Two launches (`mg_loudness_normalize`); the gain never visits the host."""
    target, ceiling = check_targets(target_lufs, peak_dbtp)
    if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
        raise _lib.MusicGanHipError("normalize: contiguous float32 waveform on a ROCm GPU expected (no CPU fallback)")
    if record.dtype != torch.float64 or record.numel() != 4 or peak.dtype != torch.float32 or peak.numel() != 1 \
            or record.device != x.device or peak.device != x.device or not record.is_contiguous():
        raise _lib.MusicGanHipError("normalize: the float64 record of `gate` and the float32 peak of `true_peak` on x's device expected")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    gain = torch.empty((1,), dtype=torch.float32, device=x.device)
    check(_lib.load().mg_loudness_normalize(_p(x), _p(out), x.numel(), _p(record), _p(peak), target, ceiling, _p(gain), _s()),
          "mg_loudness_normalize")
    return out, gain[0]

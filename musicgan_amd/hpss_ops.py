"""Tensor-level wrappers over the harmonic / percussive entries of the C ABI (include/musicgan_hip.h, csrc/hpss.hip).  Spectra are
complex64 (512, T), frequency-major, as `ops.stft_1024` returns them; waveforms are mono float32.  Both calls are one launch,
asynchronous on the caller's current stream, synchronise nothing and need no scratch memory; results come from torch.empty.  No
fallback path exists: non-GPU tensors raise."""
from __future__ import annotations

import math
from fractions import Fraction

import torch

from . import _lib, ops, pv_ops
from ._lib import check
from .ops import _p, _s

TILE = 64                                        # output rows and frames per workgroup (TILE of csrc/hpss.hip)
MIN_KERNEL, MAX_KERNEL = 3, 63
OLA_FRAME, OLA_HOP = 512, 256
# what `hpss` can return, in the order of mg_hpss's output pointers: the two component spectra (complex64), the two median-filtered
# magnitudes and the two masks (float32), all (512, T)
OUTPUTS = ("harmonic", "percussive", "H", "P", "mask_h", "mask_p")


def _pair(value, name: str, kinds) -> tuple:
    if isinstance(value, (tuple, list)):
        if len(value) != 2:
            raise ValueError(f"{name} must be one value or a pair, got {value!r}")
        pair = tuple(value)
    else:
        pair = (value, value)
    for v in pair:
        if isinstance(v, bool) or not isinstance(v, kinds):
            raise ValueError(f"{name} must hold {' or '.join(k.__name__ for k in kinds)} values, got {value!r}")
    return pair


def check_arguments(kernel_size=(31, 31), power=2.0, margin=(1.0, 1.0), want=("harmonic", "percussive")) -> tuple:
    """-> (L_h, L_p, power, m_h, m_p, want) as the library takes them; the argument errors of `hpss` as ValueError, raised before
    anything touches the device.  kernel_size: an odd int in [3, 63] or a pair (frames, bins); power: 1, 2 or inf; margin: a number
    >= 1 or a pair (harmonic, percussive); want: names out of OUTPUTS, each once."""
    lh, lp = _pair(kernel_size, "kernel_size", (int,))
    for length in (lh, lp):
        if not MIN_KERNEL <= length <= MAX_KERNEL or length % 2 == 0:
            raise ValueError(f"kernel lengths must be odd and lie in [{MIN_KERNEL}, {MAX_KERNEL}], got {kernel_size!r}")
    if isinstance(power, bool) or not isinstance(power, (int, float)) or float(power) not in (1.0, 2.0, math.inf):
        raise ValueError(f"power must be 1, 2 or inf, got {power!r}")
    mh, mp = (float(m) for m in _pair(margin, "margin", (int, float)))
    for m in (mh, mp):
        if not (1.0 <= m < math.inf):
            raise ValueError(f"margins must be finite and at least 1, got {margin!r}")
    if isinstance(want, str):
        want = (want,)
    want = tuple(want)
    if not want or any(w not in OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError(f"want must name some of {OUTPUTS}, each once, got {want!r}")
    return lh, lp, float(power), mh, mp, want


def hpss(X: torch.Tensor, kernel_size=(31, 31), power=2.0, margin=(1.0, 1.0), want=("harmonic", "percussive")) -> tuple:
    """X complex64 (512, T >= 1) -> the tensors named by `want`, in that order: median-filtering harmonic / percussive separation
    (`mg_hpss`, one launch).  H is the median of |X| over kernel_size[0] frames, P over kernel_size[1] bins (ends reflected),
    mask_h = softmask(H, margin[0] P), mask_p = softmask(P, margin[1] H) with librosa's softmask at `power`, harmonic = X mask_h,
    percussive = X mask_p.  Only what is asked for is written."""
    lh, lp, power, mh, mp, want = check_arguments(kernel_size, power, margin, want)
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.shape[0] != 512 or X.shape[1] < 1:
        raise ValueError(f"a (512, T >= 1) spectrum expected, got {tuple(getattr(X, 'shape', ()))}")
    frames = X.shape[1]
    if frames >= (1 << 31) - 2 * TILE:
        raise ValueError(f"hpss: {frames} frames are too many (2^31 - 128 and more)")
    if not X.is_cuda:
        raise _lib.MusicGanHipError("hpss: tensors on a ROCm GPU expected (no CPU fallback)")
    if X.dtype != torch.complex64 or not X.is_contiguous():
        raise _lib.MusicGanHipError(f"hpss: contiguous complex64 expected, got {X.dtype} contiguous={X.is_contiguous()}")
    lib = _lib.load()
    out = {}
    for name in want:
        shape = (512, frames, 2) if name in ("harmonic", "percussive") else (512, frames)
        out[name] = torch.empty(shape, dtype=torch.float32, device=X.device)
    check(lib.mg_hpss(_p(X), *[_p(out.get(name)) for name in OUTPUTS], frames, lh, lp, power, mh, mp, _s()), "mg_hpss")
    return tuple(torch.view_as_complex(out[name]) if name in ("harmonic", "percussive") else out[name] for name in want)


def check_ola_arguments(length: int, p: int, q: int, out_len: int) -> None:
    """the argument errors of `ola_stretch` (the integers and limits of pv_ops.check_arguments), raised before anything touches the
    device"""
    for name, v in (("length", length), ("out_len", out_len)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if length < 1 or out_len < 0:
        raise ValueError(f"at least one sample and an output length >= 0 expected, got {length} and {out_len}")
    pv_ops.check_arguments(max(1, out_len), p, q)      # p, q in [1, 2^31), p / q in [1/8, 8], out_len p < 2^62
    if length >= 1 << 40 or out_len >= 1 << 40:
        raise ValueError(f"lengths below 2^40 samples expected, got {length} and {out_len}")


def ola_stretch(x: torch.Tensor, p: int, q: int, out_len: int) -> torch.Tensor:
    """x float32 (L >= 1,), rate p / q in [1/8, 8] -> float32 (out_len,): overlap-add re-timing with a 512-sample Hann frame every
    256 output samples, frame m taken from x at floor(256 m p / q) (`mg_ola_stretch`, one launch).  Every frame is copied as it is,
    so a click keeps its shape; at p = q the result is x (zero past its end) up to the rounding of the window."""
    if not isinstance(x, torch.Tensor) or x.dim() != 1:
        raise ValueError(f"a mono waveform (samples,) expected, got {tuple(getattr(x, 'shape', ()))}")
    check_ola_arguments(x.shape[0], p, q, out_len)
    ops._chk_typed("ola_stretch", x)
    y = torch.empty((out_len,), dtype=torch.float32, device=x.device)
    check(_lib.load().mg_ola_stretch(_p(x), x.shape[0], _p(y), out_len, p, q, _s()), "mg_ola_stretch")
    return y


def stretched_samples(frames: int, rate: Fraction) -> int:
    """host arithmetic: the 256 (n - 1) samples, n = ceil(frames / rate), of a spectrum of `frames` frames re-timed by `rate`"""
    return OLA_HOP * (pv_ops.phase_vocoder_len(frames, rate.numerator, rate.denominator) - 1)

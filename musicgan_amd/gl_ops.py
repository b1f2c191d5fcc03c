"""Tensor-level wrappers over the inverse-STFT / Griffin-Lim entries of the C ABI (include/musicgan_hip.h, csrc/griffinlim.hip and the
front half of the inverse codec in csrc/codec.hip).  Spectra are complex64 (512, TT), frequency-major, as `ops.stft_1024` returns
them.  Every call is asynchronous on the caller's current stream and synchronises nothing; scratch memory comes from `ops.workspace`
(one buffer per device and stream, shared with the other op modules), results from torch.empty.  No fallback path exists:
non-GPU tensors raise."""
from __future__ import annotations

from typing import Tuple, Union

import torch

from . import _lib, ops
from ._lib import check
from .ops import _chk_typed, _p, _s

MIN_FRAMES = 4   # reflect padding of the forward STFT needs 256 * (TT - 1) > 512 samples


def check_loop_arguments(n_iter: int, momentum: float, frames: int) -> None:
    """the argument errors of the Griffin-Lim loop, raised before anything touches the device"""
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
        raise ValueError(f"n_iter must be a non-negative integer, got {n_iter!r}")
    if not 0.0 <= float(momentum) < 1.0:
        raise ValueError(f"momentum must lie in [0, 1), got {momentum!r}")
    if frames < MIN_FRAMES:
        raise ValueError(f"at least {MIN_FRAMES} frames expected, got {frames}")


def codec_inv_spectrum(magn_phase: torch.Tensor, bark_scale: torch.Tensor, zero_phase: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """[N, 2, 512, W] -> (M, Z0): the target magnitude float32 (512, N W) and the complex64 (512, N W) spectrum that `ops.codec_inv`
    inverts (audio/functions.py:108-123 of the reference); zero_phase: Z0 = M + 0i, the phase image is not read."""
    _chk_typed("codec_inv_spectrum", magn_phase, bark_scale)
    if magn_phase.dim() != 4 or magn_phase.shape[1] != 2 or magn_phase.shape[2] != 512 or tuple(bark_scale.shape) != (512,):
        raise ValueError(f"(N, 2, 512, W) and a 512-vector expected, got {tuple(magn_phase.shape)} and {tuple(bark_scale.shape)}")
    n, _, _, w = magn_phase.shape
    if n * w < 2:
        raise ValueError(f"at least 2 frames expected, got {n * w}")
    lib = _lib.load()
    nbytes = int(lib.mg_codec_inv_spectrum_ws_bytes(n, w))
    ws = ops.workspace(nbytes, magn_phase.device)
    magn = torch.empty((512, n * w), dtype=torch.float32, device=magn_phase.device)
    z = torch.empty((512, n * w, 2), dtype=torch.float32, device=magn_phase.device)
    check(lib.mg_codec_inv_spectrum(_p(magn_phase), _p(bark_scale), _p(magn), _p(z), int(bool(zero_phase)), _p(ws), nbytes, n, w, _s()),
          "mg_codec_inv_spectrum")
    return magn, torch.view_as_complex(z)


def istft_1024(Z: torch.Tensor) -> torch.Tensor:
    """complex64 (512, TT), TT >= 4 -> waveform float32 [256 * (TT - 1)]: the inverse of `ops.stft_1024` (Nyquist row zero, the
    imaginary part of DC ignored, overlap-add / window envelope, centre trimmed), one launch"""
    _chk_typed("istft_1024", Z, dtype=torch.complex64)
    if Z.dim() != 2 or Z.shape[0] != 512 or Z.shape[1] < MIN_FRAMES:
        raise ValueError(f"a (512, TT >= {MIN_FRAMES}) spectrum expected, got {tuple(Z.shape)}")
    tt = Z.shape[1]
    wav = torch.empty((256 * (tt - 1),), dtype=torch.float32, device=Z.device)
    check(_lib.load().mg_istft_1024(_p(Z), _p(wav), tt, _s()), "mg_istft_1024")
    return wav


def griffin_lim_ws_bytes(frames: int, n_iter: int) -> int:
    """host query: the scratch memory of griffin_lim (two spectra and the partial sums of every iteration)"""
    return int(_lib.load().mg_griffin_lim_ws_bytes(frames, n_iter))


def griffin_lim(M: torch.Tensor, Z: torch.Tensor, n_iter: int, momentum: float,
                return_convergence: bool = False) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """M float32 (512, TT), Z complex64 (512, TT): n_iter times R = STFT(ISTFT(Z)), c = R - mu R_prev, Z = M c / (|c| + 1e-16) with
    mu = momentum / (1 + momentum); returns the waveform ISTFT(Z) [256 * (TT - 1)].  All of Z is rewritten in place (the last
    projection) if n_iter > 0.  return_convergence: also float64 [n_iter], entry k = || |R_k| - M || / || M ||."""
    _chk_typed("griffin_lim", M)
    _chk_typed("griffin_lim", Z, dtype=torch.complex64)
    if M.dim() != 2 or M.shape[0] != 512 or Z.shape != M.shape:
        raise ValueError(f"M (512, TT) and Z of the same shape expected, got {tuple(M.shape)} and {tuple(Z.shape)}")
    tt = M.shape[1]
    check_loop_arguments(n_iter, momentum, tt)
    lib = _lib.load()
    nbytes = griffin_lim_ws_bytes(tt, n_iter)
    ws = ops.workspace(nbytes, M.device)
    wav = torch.empty((256 * (tt - 1),), dtype=torch.float32, device=M.device)
    conv = torch.empty((n_iter,), dtype=torch.float64, device=M.device) if return_convergence else None
    check(lib.mg_griffin_lim(_p(M), _p(Z), _p(wav), _p(conv) if n_iter else None, _p(ws), nbytes, tt, n_iter, float(momentum), _s()),
          "mg_griffin_lim")
    return (wav, conv) if return_convergence else wav

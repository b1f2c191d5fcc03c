"""Tensor-level wrappers over mg_logmel_rows, mg_moments, mg_mel_power and mg_logmel_pool of the C ABI (include/musicgan_hip.h,
csrc/logmel.hip, csrc/moments.hip, csrc/melspec.hip): the log-mel feature rows of a batch of magnitude images, the float64 mean and
covariance of a set of rows, the mel power spectrogram of waveforms and its pooled log rows -- what metrics.LogMel, metrics.Frechet,
audio.mel_spectrogram and metrics.WaveLogMel are made of.  Every call is asynchronous on the caller's current stream and reads
nothing back; scratch memory (the partial sums of the moments) is allocated here with torch.empty, call by call.  Shapes are checked
on the host, before any tensor's device is looked at.  No fallback path exists: non-GPU tensors raise."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .ops import _chk_typed, _p, _s

MAX_BANDS = 256      # band limits go to the kernel by value
MAX_POOL = 1024      # columns of one pool
MAX_D = 4096         # numbers per row moments takes
MAX_N = 1 << 24      # rows moments takes
MEL_BINS = 512       # bins of a frame of mel_power: N_FFT / 2
MEL_HOP = 256        # samples between two frames


def _limits(name: str, v, bands: int, what: str = "logmel_rows") -> torch.Tensor:
    if not isinstance(v, torch.Tensor) or v.is_cuda or v.dtype != torch.int32 or tuple(v.shape) != (bands,):
        raise ValueError(f"{what}: {name}: a host int32 tensor ({bands},) expected")
    return v.contiguous()


def logmel_rows(x: torch.Tensor, c: int, scale: torch.Tensor, weight: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, floor: float,
                pools: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (N, C, H, W) float32, rows = frequency and columns = time, its channel c; scale (H,) and weight (M, H) float32 on x's
    device; lo, hi (M,) int32 HOST tensors with 0 <= lo <= hi <= H (they are read before the call returns); floor > 0; `pools`
    divides W -> out (N, M * pools) float32, every element written:
        p[h,t] = (x[n,c,h,t] * scale[h] + scale[h]) ** 2 and s[m,t] = sum of weight[m,h] * p[h,t] over lo[m] <= h < hi[m], in
        float32 in ascending h; out[n, m * pools + j] = the float64 mean of log(s[m,t] + floor) over the W / pools columns of
        pool j, in ascending t, rounded once.
    Weights outside [lo, hi) are not read.  A row of out depends on its image and on the shapes alone.  Returns out."""
    if not all(isinstance(t, torch.Tensor) for t in (x, scale, weight)):
        raise ValueError("logmel_rows: tensors x, scale and weight expected")
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"logmel_rows: a non-empty batch x (N, C, H, W) expected, got {tuple(x.shape)}")
    n, ch, h, w = x.shape
    if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < ch:
        raise ValueError(f"logmel_rows: a channel in 0 .. {ch - 1} expected, got {c}")
    if weight.dim() != 2 or weight.shape[1] != h or not 1 <= weight.shape[0] <= MAX_BANDS or tuple(scale.shape) != (h,):
        raise ValueError(f"logmel_rows: scale ({h},) and weight (M, {h}) with M in 1 .. {MAX_BANDS} expected, got "
                         f"{tuple(scale.shape)} and {tuple(weight.shape)}")
    bands = weight.shape[0]
    if isinstance(pools, bool) or not isinstance(pools, int) or pools < 1 or w % pools or w // pools > MAX_POOL:
        raise ValueError(f"logmel_rows: a pool count that divides W = {w} into pools of at most {MAX_POOL} columns expected, got {pools}")
    lo, hi = _limits("lo", lo, bands), _limits("hi", hi, bands)
    if bool(((lo < 0) | (lo > hi) | (hi > h)).any()):
        raise ValueError(f"logmel_rows: 0 <= lo <= hi <= H = {h} expected for every band")
    floor = float(floor)
    if not 0.0 < floor < float("inf"):
        raise ValueError(f"logmel_rows: a finite floor > 0 expected, got {floor}")
    if out is not None and tuple(out.shape) != (n, bands * pools):
        raise ValueError(f"logmel_rows: out ({n}, {bands * pools}) expected, got {tuple(out.shape)}")
    _chk_typed("logmel_rows", x, scale, weight)
    if out is None:
        out = torch.empty((n, bands * pools), dtype=torch.float32, device=x.device)
    _chk_typed("logmel_rows", out)
    i32p = ctypes.POINTER(ctypes.c_int32)
    check(_lib.load().mg_logmel_rows(_p(x), n, ch, c, h, w, _p(scale), _p(weight), ctypes.cast(lo.data_ptr(), i32p),
                                     ctypes.cast(hi.data_ptr(), i32p), bands, floor, pools, _p(out), _s()), "mg_logmel_rows")
    return out


def mel_frames(length: int) -> int:
    """frames of a signal of `length` samples: 1 + length // 256"""
    return 1 + length // MEL_HOP


def mel_power(wave: torch.Tensor, weight: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wave (B, L) float32, L > 512, samples of a row contiguous and rows wave.stride(0) >= L apart (a view of a wider buffer is
    taken as it is); weight (M, 512) float32 on wave's device, M <= 256; lo, hi (M,) int32 HOST tensors with 0 <= lo <= hi <= 512
    (read before the call returns) -> out (B, M, T) float32, T = 1 + L // 256, every element written:
        X[k,t] = ops.stft_1024(row)[k,t]; p[k,t] = re * re + im * im and s[m,t] = sum of weight[m,k] * p[k,t] over
        lo[m] <= k < hi[m], in float32 in ascending k, every operation rounded (no fma); an empty band gives +0.0.
    One launch; the spectrum is never written.  Weights outside [lo, hi) are not read.  A row of out depends on its row of wave
    alone.  Returns out."""
    if not isinstance(wave, torch.Tensor) or not isinstance(weight, torch.Tensor):
        raise ValueError("mel_power: tensors wave and weight expected")
    if wave.dim() != 2 or wave.shape[0] < 1 or wave.shape[1] <= MEL_BINS:
        raise ValueError(f"mel_power: wave (B, L) with B >= 1 and L > {MEL_BINS} expected, got {tuple(wave.shape)}")
    rows, length = wave.shape
    if wave.stride(1) != 1 or (rows > 1 and wave.stride(0) < length):
        raise ValueError(f"mel_power: rows of contiguous samples at least L = {length} apart expected, got strides {wave.stride()}")
    if weight.dim() != 2 or weight.shape[1] != MEL_BINS or not 1 <= weight.shape[0] <= MAX_BANDS:
        raise ValueError(f"mel_power: weight (M, {MEL_BINS}) with M in 1 .. {MAX_BANDS} expected, got {tuple(weight.shape)}")
    bands, frames = weight.shape[0], mel_frames(length)
    lo, hi = _limits("lo", lo, bands, "mel_power"), _limits("hi", hi, bands, "mel_power")
    if bool(((lo < 0) | (lo > hi) | (hi > MEL_BINS)).any()):
        raise ValueError(f"mel_power: 0 <= lo <= hi <= {MEL_BINS} expected for every band")
    if wave.dtype != torch.float32 or weight.dtype != torch.float32 or (out is not None and out.dtype != torch.float32):
        raise ValueError("mel_power: float32 wave, weight and out expected")
    if out is not None and tuple(out.shape) != (rows, bands, frames):
        raise ValueError(f"mel_power: out ({rows}, {bands}, {frames}) expected, got {tuple(out.shape)}")
    if not wave.is_cuda:
        raise _lib.MusicGanHipError("mel_power: tensors on a ROCm GPU expected (no CPU fallback)")
    _chk_typed("mel_power", weight)
    if out is None:
        out = torch.empty((rows, bands, frames), dtype=torch.float32, device=wave.device)
    _chk_typed("mel_power", out)
    i32p = ctypes.POINTER(ctypes.c_int32)
    check(_lib.load().mg_mel_power(_p(wave), rows, length, wave.stride(0) if rows > 1 else length, _p(weight),
                                   ctypes.cast(lo.data_ptr(), i32p), ctypes.cast(hi.data_ptr(), i32p), bands, _p(out), _s()),
          "mg_mel_power")
    return out


def pool_windows(frames: int, win: int, hop: int) -> int:
    """windows of `win` frames every `hop` frames in `frames` frames, the tail dropped; 0 if there is none"""
    return (frames - win) // hop + 1 if frames >= win else 0


def logmel_pool(power: torch.Tensor, win: int, hop: int, pools: int, floor: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """power (B, M, T) float32 (what mel_power returns); windows of `win` frames every `hop` frames, W = (T - win) // hop + 1 per
    row, the tail dropped (T < win is refused); `pools` divides win; floor > 0 -> out (B * W, M * pools) float32, every element
    written: out[b * W + n, m * pools + j] = the float64 mean of log(power[b, m, t] + floor) over the win / pools frames of pool j of
    window n, in ascending t, rounded once.  A row of out depends on its window's frames alone.  Returns out."""
    if not isinstance(power, torch.Tensor) or power.dim() != 3 or min(power.shape) < 1 or power.shape[1] > MAX_BANDS:
        raise ValueError(f"logmel_pool: power (B, M, T), non-empty with M <= {MAX_BANDS}, expected, got "
                         f"{tuple(power.shape) if isinstance(power, torch.Tensor) else type(power).__name__}")
    rows, bands, frames = power.shape
    for name, v in (("win", win), ("hop", hop), ("pools", pools)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"logmel_pool: {name}: an integer >= 1 expected, got {v!r}")
    if win % pools:
        raise ValueError(f"logmel_pool: a pool count that divides win = {win} expected, got {pools}")
    if frames < win:
        raise ValueError(f"logmel_pool: {frames} frames are fewer than one window of {win}")
    floor = float(floor)
    if not 0.0 < floor < float("inf"):
        raise ValueError(f"logmel_pool: a finite floor > 0 expected, got {floor}")
    shape = (rows * pool_windows(frames, win, hop), bands * pools)
    if power.dtype != torch.float32 or (out is not None and out.dtype != torch.float32):
        raise ValueError("logmel_pool: float32 power and out expected")
    if out is not None and tuple(out.shape) != shape:
        raise ValueError(f"logmel_pool: out {shape} expected, got {tuple(out.shape)}")
    _chk_typed("logmel_pool", power)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=power.device)
    _chk_typed("logmel_pool", out)
    check(_lib.load().mg_logmel_pool(_p(power), rows, bands, frames, win, hop, pools, floor, _p(out), _s()), "mg_logmel_pool")
    return out


def _moments_shape(rows) -> Tuple[int, int]:
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
        raise ValueError("moments: rows (n, d) expected")
    n, d = rows.shape
    if not 2 <= n <= MAX_N or not 1 <= d <= MAX_D:
        raise ValueError(f"moments: 2 .. {MAX_N} rows of 1 .. {MAX_D} numbers expected, got {tuple(rows.shape)}")
    return n, d


def moments_ws_bytes(n: int, d: int) -> int:
    """host query: the scratch memory moments allocates for n rows of d numbers (float64 sums of chunks of 1024 rows: a (d,) and a
    (d, d) block per chunk); 0 for a shape moments refuses"""
    return int(_lib.load().mg_moments_ws_bytes(n, d))


def moments(rows: torch.Tensor, mean: Optional[torch.Tensor] = None, cov: Optional[torch.Tensor] = None):
    """rows (n, d) float32, n >= 2, d <= 4096 -> all of mean (d,) and all of cov (d, d) float64 are written: the mean over the rows
    and the unbiased covariance sum_i (x_ij - mean_j)(x_ik - mean_k) / (n - 1), two passes in float64 in a fixed order (chunks of
    1024 rows, added in chunk order): the same bits in every run, and cov[j, k] and cov[k, j] hold the same bits.  Returns
    (mean, cov)."""
    n, d = _moments_shape(rows)
    for name, t, shape in (("mean", mean, (d,)), ("cov", cov, (d, d))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"moments: {name} {shape} expected, got {tuple(t.shape)}")
    _chk_typed("moments", rows)
    if mean is None:
        mean = torch.empty(d, dtype=torch.float64, device=rows.device)
    if cov is None:
        cov = torch.empty((d, d), dtype=torch.float64, device=rows.device)
    _chk_typed("moments", mean, cov, dtype=torch.float64)
    nbytes = moments_ws_bytes(n, d)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=rows.device)
    check(_lib.load().mg_moments(_p(rows), n, d, _p(mean), _p(cov), _p(ws), nbytes, _s()), "mg_moments")
    return mean, cov

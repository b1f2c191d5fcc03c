"""STFT / magnitude-phase codec with the reference's function signatures
(/root/reference/music_gan/audio/functions.py:26-139), evaluated by the HIP kernels `mg_stft_1024`, `mg_codec_fwd`,
`mg_codec_inv` on the current ROCm device.  Results come back as tensors on that device."""
from __future__ import annotations

from fractions import Fraction
import math
from typing import Tuple

import torch as th

from . import constant, wavio
from .. import gl_ops, hpss_ops, lim_ops, loud_ops, mel_ops, ops, pv_ops

_bark_cache = {}


def _device() -> th.device:
    if not th.cuda.is_available():
        from .._lib import MusicGanHipError
        raise MusicGanHipError("musicgan_amd.audio needs a ROCm GPU (no CPU fallback)")
    return th.device("cuda", th.cuda.current_device())


def _bark_vector(nb_freq: int, device) -> th.Tensor:
    """unit-norm 6*asinh(f/600) on linspace(20, 22050, nb_freq) (functions.py:29-35); 512 floats, built once per device."""
    key = (nb_freq, str(device))
    if key not in _bark_cache:
        scale = 6. * th.arcsinh(th.linspace(20., 44100 // 2, nb_freq) / 600.)
        _bark_cache[key] = (scale / scale.norm()).to(device).contiguous()
    return _bark_cache[key]


def bark_magn_scale(magn: th.Tensor, unscale: bool = False) -> th.Tensor:
    assert len(magn.size()) == 2, f"(STFT, TIME), actual = {magn.size()}"
    s = _bark_vector(magn.size()[0], magn.device)[:, None]
    return magn / s if unscale else magn * s


def _fast_stft(nperseg: int, stride: int) -> bool:
    """1024 / 256 (audio/constant.py; all the drivers use) runs the tuned kernel; any other power-of-two window the untuned one."""
    if nperseg == constant.N_FFT and stride == constant.STFT_STRIDE:
        return True
    assert 64 <= nperseg <= 8192 and nperseg & (nperseg - 1) == 0 and stride >= 1, \
        f"nperseg must be a power of two in [64, 8192] and stride >= 1, actual = ({nperseg}, {stride})"
    return False


def stft_from_waveform(raw_audio: th.Tensor, nperseg: int = constant.N_FFT, stride: int = constant.STFT_STRIDE) -> th.Tensor:
    """(channels, samples) or (samples,) -> complex64 (nperseg/2, 1 + samples//stride), Nyquist row dropped."""
    fast = _fast_stft(nperseg, stride)
    dev = raw_audio.device if raw_audio.is_cuda else _device()
    x = raw_audio.to(dev, th.float32)
    if x.dim() == 2 and x.shape[0] > 1:
        frames = x.t().contiguous()  # frames x channels: the mono mean (functions.py:49) is taken by the kernel
        return ops.stft_1024_pcm(frames) if fast else ops.stft_generic(ops.pcm_to_mono(frames), nperseg, stride)
    mono = x.reshape(-1).contiguous()
    return ops.stft_1024(mono) if fast else ops.stft_generic(mono, nperseg, stride)


_mel_banks = {}


def _mel_bank(n_mels: int, f_min: float, f_max: float, device):
    """(weight on `device`, lo, hi on the host) of metrics.mel_filterbank over the 512 bins, built once per bank and device"""
    key = (n_mels, float(f_min), float(f_max), str(device))
    if key not in _mel_banks:
        from ..metrics import mel_filterbank   # (metrics imports this module's codec vector lazily too)
        weight, lo, hi = mel_filterbank(constant.N_FFT // 2, n_mels, f_min, f_max)
        _mel_banks[key] = (weight.to(device), lo, hi)
    return _mel_banks[key]


def mel_spectrogram(waveform: th.Tensor, n_mels: int = 64, f_min: float = 0.0, f_max: float = 22050.0) -> th.Tensor:
    """(..., L) or (L,) samples at 44.1 kHz, L > 512, any float type, any device -> (..., n_mels, 1 + L // 256) float32 on the GPU:
    the mel power spectrogram, one fused launch (csrc/melspec.hip; the spectrum is never written).  It restates
    torchaudio.transforms.MelSpectrogram(sample_rate=44100, n_fft=1024, hop_length=256, power=2, normalized="window",
    mel_scale="htk", norm=None, f_min=f_min, f_max=f_max, n_mels=n_mels): reflect padding by 512, periodic Hann / sqrt(sum w^2),
    |X|^2, and the triangular HTK bank metrics.mel_filterbank(512, n_mels, f_min, f_max) over the bins 0 .. 511.  The Nyquist bin is
    dropped, as everywhere in the codec: its frequency is 22 050 Hz, so for any f_max <= 22050 its weight in every band is 0 and
    nothing is lost.  torchaudio is not installed where this was written; the tests hold the function against a float64 restatement
    of the formula (tests/melspec_ref.py), not against torchaudio itself.  Rows are independent: a multi-channel waveform is NOT
    averaged to mono (the loaders do that), every channel gets its own spectrogram."""
    if not isinstance(waveform, th.Tensor) or waveform.dim() < 1 or not waveform.is_floating_point():
        raise ValueError("mel_spectrogram: a floating-point waveform (..., L) expected")
    if waveform.shape[-1] <= constant.N_FFT // 2 or waveform.numel() == 0:
        raise ValueError(f"mel_spectrogram: more than {constant.N_FFT // 2} samples per row expected, got {tuple(waveform.shape)}")
    from ..metrics import mel_filterbank
    mel_filterbank(constant.N_FFT // 2, n_mels, f_min, f_max)   # refuses a bad bank before a device is looked at
    dev = waveform.device if waveform.is_cuda else _device()
    weight, lo, hi = _mel_bank(n_mels, f_min, f_max, dev)
    rows = waveform.to(dev, th.float32).reshape(-1, waveform.shape[-1]).contiguous()
    out = mel_ops.mel_power(rows, weight, lo, hi)
    return out.reshape(*waveform.shape[:-1], n_mels, out.shape[-1])


def resample(waveform: th.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
             resampling_method: str = "sinc_interp_hann", beta=None) -> th.Tensor:
    """torchaudio.functional.resample: (..., time) -> (..., ceil(time * new / orig)) (rates reduced by their gcd), rows
    independent, band-limited sinc interpolation with a Hann window (`mg_resample_pcm`, one launch).  Results are float32 on the
    device; a CPU tensor is moved there first.  orig_freq == new_freq returns `waveform` itself, as torchaudio does.
    Only sinc_interp_hann is built (`beta` belongs to the Kaiser window and is ignored, as torchaudio ignores it for Hann)."""
    for name, f in (("orig_freq", orig_freq), ("new_freq", new_freq)):
        if isinstance(f, bool) or not isinstance(f, (int, float)) or int(f) != f or f <= 0:
            raise ValueError(f"{name} must be a positive integer, got {f!r}")
    if int(lowpass_filter_width) != lowpass_filter_width or lowpass_filter_width <= 0:
        raise ValueError(f"lowpass_filter_width must be a positive integer, got {lowpass_filter_width!r}")
    if not rolloff > 0:
        raise ValueError(f"rolloff must be positive, got {rolloff!r}")
    if resampling_method != "sinc_interp_hann":
        raise ValueError(f"resampling_method {resampling_method!r} is not supported: only 'sinc_interp_hann' is built")
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq == new_freq:
        return waveform
    if not waveform.is_floating_point():
        raise ValueError(f"resample expects a floating-point waveform, got {waveform.dtype}")
    dev = waveform.device if waveform.is_cuda else _device()
    lead, length = waveform.shape[:-1], waveform.shape[-1]
    out_len = ops.resample_len(length, orig_freq, new_freq)
    if waveform.numel() == 0:
        return th.zeros((*lead, out_len), dtype=th.float32, device=dev)
    x = waveform.to(dev, th.float32).reshape(-1, length)
    if length > 1 and x.stride(1) != 1:
        x = x.contiguous()
    return ops.resample_rows(x, orig_freq, new_freq, int(lowpass_filter_width), float(rolloff)).reshape(*lead, out_len)


def stft_from_pcm(pcm: th.Tensor, nperseg: int = constant.N_FFT, stride: int = constant.STFT_STRIDE,
                  sample_rate: int = constant.SAMPLE_RATE) -> th.Tensor:
    """PCM frames (frames, channels) exactly as a WAV file stores them (wavio.load_pcm), on the device -> the same result as
    wav_to_stft on that file: normalisation to [-1, 1], mono mean and STFT in one launch (two for other window sizes).
    `sample_rate` other than 44.1 kHz: normalisation, mono mean and the resampling to 44.1 kHz in one launch, then the STFT."""
    if sample_rate != constant.SAMPLE_RATE:
        mono = ops.resample_pcm(pcm, sample_rate, constant.SAMPLE_RATE)
        return ops.stft_1024(mono) if _fast_stft(nperseg, stride) else ops.stft_generic(mono, nperseg, stride)
    if _fast_stft(nperseg, stride):
        return ops.stft_1024_pcm(pcm)
    return ops.stft_generic(ops.pcm_to_mono(pcm), nperseg, stride)


def wav_to_stft(wav_p: str, nperseg: int = constant.N_FFT, stride: int = constant.STFT_STRIDE, *, resample: bool = False) -> th.Tensor:
    """`resample`: a file at any other rate is resampled to 44.1 kHz first (torchaudio.functional.resample's defaults); without
    it such a file raises, as the reference does.  A 44.1 kHz file takes the same path either way."""
    import os
    if os.path.splitext(wav_p)[1].lower() == ".flac":  # decoded on the device: the PCM never visits the host
        sr = wavio.flac.read_header(wav_p).sample_rate
        pcm = None
    elif os.path.splitext(wav_p)[1].lower() in wavio.OGG_EXTS:  # Ogg Vorbis: likewise
        sr = wavio.vorbis.read_header(wav_p).sample_rate
        pcm = None
    else:
        pcm, sr = wavio.load_pcm(wav_p)
    assert resample or sr == constant.SAMPLE_RATE, \
        f"Audio sample rate must be {constant.SAMPLE_RATE}Hz, " \
        f"file \"{wav_p}\" is {sr}Hz"
    if pcm is None:
        return stft_from_pcm(wavio.load_pcm_device(wav_p, _device()), nperseg, stride, sample_rate=sr)
    import numpy as np
    return stft_from_pcm(th.from_numpy(np.ascontiguousarray(pcm)).to(_device()), nperseg, stride, sample_rate=sr)


def stft_to_phase_magn(complex_values: th.Tensor, nb_vec: int = constant.N_VEC) -> Tuple[th.Tensor, th.Tensor]:
    dev = complex_values.device if complex_values.is_cuda else _device()
    c = complex_values.to(dev, th.complex64)
    return ops.codec_fwd(c, _bark_vector(c.shape[0], dev), nb_vec)


def stft_to_stacked_phase_magn(complex_values: th.Tensor, nb_vec: int = constant.N_VEC) -> th.Tensor:
    """`th.stack(stft_to_phase_magn(c), dim=1)` -- the (S, 2, 512, nb_vec) tensor create_dataset.py:52-58 builds -- written once by
    the codec kernel instead of two images and a concatenation pass."""
    dev = complex_values.device if complex_values.is_cuda else _device()
    c = complex_values.to(dev, th.complex64)
    return ops.codec_fwd(c, _bark_vector(c.shape[0], dev), nb_vec, stacked=True)


def _check_magn_phase(magn_phase: th.Tensor) -> None:
    assert len(magn_phase.size()) == 4, \
        f"(N, 2, H, W), actual = {magn_phase.size()}"
    assert magn_phase.size()[1] == 2, \
        f"Channels must be equal to 2, actual = {magn_phase.size()[1]}"
    assert magn_phase.size()[2] == constant.N_FFT // 2, \
        f"Frequency size must be equal to {constant.N_FFT // 2}, " \
        f"actual = {magn_phase.size()[2]}"


def istft(complex_values: th.Tensor) -> th.Tensor:
    """complex64 (512, T), T >= 4, Nyquist row dropped -> waveform [256 * (T - 1)]: the counterpart of `stft_from_waveform` for
    1024 / 256 (`mg_istft_1024`, one launch)."""
    if complex_values.dim() != 2 or complex_values.shape[0] != constant.N_FFT // 2 or complex_values.shape[1] < gl_ops.MIN_FRAMES:
        raise ValueError(f"a ({constant.N_FFT // 2}, T >= {gl_ops.MIN_FRAMES}) spectrum expected, got {tuple(complex_values.shape)}")
    dev = complex_values.device if complex_values.is_cuda else _device()
    return gl_ops.istft_1024(complex_values.to(dev, th.complex64).contiguous())


def _check_phase_lock(phase_lock) -> None:
    if not isinstance(phase_lock, bool):
        raise ValueError(f"phase_lock must be True or False, got {phase_lock!r}")


def phase_vocoder(complex_specgrams: th.Tensor, rate, phase_lock: bool = False) -> th.Tensor:
    """torchaudio.functional.phase_vocoder for this package's STFT (1024 / 256, phase_advance pi k / 2): complex (512, T), T >= 1 ->
    complex64 (512, ceil(T / rate)) on the device; a CPU tensor is moved there first.  rate (above 1: faster and shorter) is an int,
    a fractions.Fraction or a float in [1/8, 8]; a float is turned into Fraction(rate).limit_denominator(1000), so that the time axis
    is integer arithmetic.  Magnitudes and angles are float32, the phase is accumulated in float64 modulo 2 pi.
    phase_lock: identity phase locking (Laroche & Dolson 1999): the bins around every magnitude peak of an output frame keep the
    phase differences they have in the analysis frame, which takes the amplitude warble out of moving pitches."""
    r = pv_ops.as_rate(rate)
    _check_phase_lock(phase_lock)
    if complex_specgrams.dim() != 2 or complex_specgrams.shape[0] != constant.N_FFT // 2 or complex_specgrams.shape[1] < 1:
        raise ValueError(f"a ({constant.N_FFT // 2}, T >= 1) spectrum expected, got {tuple(complex_specgrams.shape)}")
    if not complex_specgrams.is_complex():
        raise ValueError(f"a complex spectrum expected, got {complex_specgrams.dtype}")
    dev = complex_specgrams.device if complex_specgrams.is_cuda else _device()
    x = complex_specgrams.to(dev, th.complex64).contiguous()
    if not phase_lock:
        return pv_ops.phase_vocoder(x, r.numerator, r.denominator)
    return pv_ops.phase_vocoder(x, r.numerator, r.denominator, lock=True)


def hpss(complex_spec: th.Tensor, kernel_size=31, power: float = 2.0, margin=1.0, mask: bool = False) -> Tuple[th.Tensor, th.Tensor]:
    """librosa.decompose.hpss for this package's STFT: complex (512, T), T >= 1 -> (harmonic, percussive), two complex64 (512, T)
    spectra on the device (a CPU tensor is moved there first); with `mask` the two float32 masks instead.  Median filtering
    (Fitzgerald 2010): the harmonic estimate is the median of |X| along time, the percussive one along frequency, each over
    kernel_size (an odd int in [3, 63], or a pair (frames, bins)) with reflected ends; the masks are librosa's softmask at `power`
    (1, 2 or inf) with `margin` (a number >= 1, or a pair (harmonic, percussive)).  With margin 1 the two components sum to the
    input; above 1 a residual is left out of both."""
    args = hpss_ops.check_arguments(kernel_size, power, margin, ("mask_h", "mask_p") if mask else ("harmonic", "percussive"))
    if complex_spec.dim() != 2 or complex_spec.shape[0] != constant.N_FFT // 2 or complex_spec.shape[1] < 1:
        raise ValueError(f"a ({constant.N_FFT // 2}, T >= 1) spectrum expected, got {tuple(complex_spec.shape)}")
    if not complex_spec.is_complex():
        raise ValueError(f"a complex spectrum expected, got {complex_spec.dtype}")
    dev = complex_spec.device if complex_spec.is_cuda else _device()
    return hpss_ops.hpss(complex_spec.to(dev, th.complex64).contiguous(), args[:2], args[2], args[3:5], args[5])


def _component(waveform: th.Tensor, index: int, kernel_size, power, margin) -> th.Tensor:
    if waveform.dim() != 1 or not waveform.is_floating_point():
        raise ValueError(f"a mono floating-point waveform (samples,) expected, got {tuple(waveform.shape)} {waveform.dtype}")
    hpss_ops.check_arguments(kernel_size, power, margin)
    return istft(hpss(stft_from_waveform(waveform), kernel_size, power, margin)[index])


def harmonic(waveform: th.Tensor, kernel_size=31, power: float = 2.0, margin=1.0) -> th.Tensor:
    """librosa.effects.harmonic: mono (samples,) float waveform -> its harmonic component, 256 * (samples // 256) samples:
    `istft(hpss(stft_from_waveform(waveform))[0])`; fewer than 4 frames raise the ValueError of `istft`.  kernel_size, power,
    margin: as `hpss` takes them."""
    return _component(waveform, 0, kernel_size, power, margin)


def percussive(waveform: th.Tensor, kernel_size=31, power: float = 2.0, margin=1.0) -> th.Tensor:
    """librosa.effects.percussive: as `harmonic`, the percussive component"""
    return _component(waveform, 1, kernel_size, power, margin)


def time_stretch(waveform: th.Tensor, rate, preserve_transients: bool = False, phase_lock: bool = False) -> th.Tensor:
    """mono (samples,) float waveform -> the same sound `rate` times as fast at the same pitch: `istft(phase_vocoder(
    stft_from_waveform(waveform), rate))`, 256 * (n - 1) samples for n = ceil((1 + samples // 256) / rate) frames; n < 4 raises
    the ValueError of `istft`.  rate: as `phase_vocoder` takes it.
    preserve_transients (Driedger, Mueller, Ewert 2014): the spectrum is split by `hpss`; only the harmonic part goes through the
    phase vocoder, the percussive part is re-timed by overlap-add of short frames, which copies every hit as it is:
    `istft(phase_vocoder(Xh, rate)) + ola_stretch(istft(Xp), p, q, 256 * (n - 1))`, the same length; fewer than 4 frames on either
    side raise the ValueError of `istft`.  phase_lock: passed to `phase_vocoder`."""
    r = pv_ops.as_rate(rate)
    _check_phase_lock(phase_lock)
    if waveform.dim() != 1 or not waveform.is_floating_point():
        raise ValueError(f"a mono floating-point waveform (samples,) expected, got {tuple(waveform.shape)} {waveform.dtype}")
    if not preserve_transients:
        return istft(phase_vocoder(stft_from_waveform(waveform), r, phase_lock=phase_lock))
    return retime_preserving_transients(stft_from_waveform(waveform), r, as_waveform=True, phase_lock=phase_lock)


def retime_preserving_transients(complex_spec: th.Tensor, rate, as_waveform: bool = False, phase_lock: bool = False) -> th.Tensor:
    """complex64 (512, T >= 4) on the device -> the spectrum (512, n = ceil(T / rate)) of the transient-preserving re-timing:
    `phase_vocoder(Xh, rate) + stft(ola_stretch(istft(Xp), p, q, 256 * (n - 1)))` for (Xh, Xp) = hpss(X); as_waveform: the
    waveform `istft(phase_vocoder(Xh, rate)) + ola_stretch(...)` of 256 * (n - 1) samples instead (what `time_stretch` returns).
    phase_lock: the harmonic part goes through the phase-locked vocoder (the configuration of Driedger et al.)."""
    r = pv_ops.as_rate(rate)
    _check_phase_lock(phase_lock)
    xh, xp = hpss(complex_spec)
    samples = hpss_ops.stretched_samples(complex_spec.shape[1], r)
    hits = hpss_ops.ola_stretch(istft(xp), r.numerator, r.denominator, samples)
    tones = phase_vocoder(xh, r, phase_lock=phase_lock)
    if as_waveform:
        return istft(tones) + hits
    return tones + ops.stft_1024(hits)


def pitch_ratio(n_steps) -> Fraction:
    """the frequency ratio 2^(n_steps / 12) of n_steps semitones as the closest fraction P / Q with Q <= 64 (host arithmetic; at
    most 1.955 cents off for every whole n_steps in -12 .. 12)"""
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, float, Fraction)) or float(n_steps) != float(n_steps):
        raise ValueError(f"n_steps must be a number of semitones, got {n_steps!r}")
    return Fraction(2 ** (float(n_steps) / 12)).limit_denominator(64)


def pitch_shift(waveform: th.Tensor, n_steps, sample_rate: int = constant.SAMPLE_RATE, preserve_transients: bool = False,
                phase_lock: bool = False) -> th.Tensor:
    """torchaudio.functional.pitch_shift for a mono (samples,) waveform: with P / Q = pitch_ratio(n_steps), `time_stretch` by Q / P
    (longer for an upward shift), then `resample` from P to Q, cropped or zero-padded to the input's length.  The result does not
    depend on `sample_rate` (kept for torchaudio's signature).  preserve_transients, phase_lock: passed to `time_stretch`."""
    f = pitch_ratio(n_steps)
    pv_ops.as_rate(1 / f)
    y = time_stretch(waveform, 1 / f, preserve_transients=preserve_transients, phase_lock=phase_lock)
    y = resample(y, f.numerator, f.denominator)
    n = waveform.shape[0]
    if y.shape[0] >= n:
        return y[:n]
    out = th.zeros((n,), dtype=y.dtype, device=y.device)
    out[:y.shape[0]] = y
    return out


def griffin_lim(magn_phase: th.Tensor, n_iter: int = 32, momentum: float = 0.99, init: str = "phase", return_convergence: bool = False):
    """(N, 2, 512, W) -> waveform [256 * (N W - 1)] after n_iter rounds of Griffin-Lim (torchaudio.functional.griffinlim with
    power = 1 and rand_init = False): the decoded magnitude is held and the phase moves towards one that a signal can have.
    init: "phase" starts from the decoded phase image (n_iter = 0 is `magn_phase_to_waveform` up to rounding), "zero" from zero
    phase, i.e. from the magnitude alone.  return_convergence: also a float64 tensor [n_iter] on the device, entry k the relative
    distance || |STFT(ISTFT(Z))| - M || / || M || at the start of round k."""
    if init not in ("phase", "zero"):
        raise ValueError(f"init must be 'phase' or 'zero', got {init!r}")
    _check_magn_phase(magn_phase)
    gl_ops.check_loop_arguments(n_iter, momentum, magn_phase.shape[0] * magn_phase.shape[3])
    dev = magn_phase.device if magn_phase.is_cuda else _device()
    mp = magn_phase.to(dev, th.float32).contiguous()
    magn, z = gl_ops.codec_inv_spectrum(mp, _bark_vector(constant.N_FFT // 2, dev), zero_phase=init == "zero")
    return gl_ops.griffin_lim(magn, z, n_iter, momentum, return_convergence=return_convergence)


_griffin_lim = griffin_lim   # the keyword of the two functions below shadows the name


def kweighting_coefficients(sample_rate: int):
    """((b, a), (b, a)): the shelf and the high-pass biquad of the K-weighting filter (ITU-R BS.1770-4) at `sample_rate`, each a
    float64 array of three numbers (a[0] = 1), computed on the host from the analog prototypes libebur128 and pyloudnorm use; at
    48 kHz the standard's table."""
    import numpy as np
    return tuple((np.asarray(b, dtype=np.float64), np.asarray(a, dtype=np.float64))
                 for b, a in loud_ops.kweighting_coefficients(sample_rate))


def _loudness_input(waveform: th.Tensor, min_length: int = 0) -> th.Tensor:
    """(L,) or (C <= 8, L) float -> float32 (C, L) on the device with unit stride along L; ValueError before the device is touched"""
    if not isinstance(waveform, th.Tensor) or waveform.dim() not in (1, 2):
        raise ValueError(f"a waveform (samples,) or (channels, samples) expected, got {getattr(waveform, 'shape', waveform)!r}")
    x = waveform[None, :] if waveform.dim() == 1 else waveform
    loud_ops.check_waveform(x)
    if x.shape[1] < min_length:
        raise ValueError(f"at least one sample expected, got {tuple(waveform.shape)}")
    dev = x.device if x.is_cuda else _device()
    x = x.to(dev, th.float32)
    return x.contiguous() if x.shape[1] > 1 and x.stride(1) != 1 else x


def loudness(waveform: th.Tensor, sample_rate: int, channel_weights=None, return_details: bool = False):
    """Integrated programme loudness in LUFS (ITU-R BS.1770-4 / EBU R128) of a float waveform (L,) or (C <= 8, L): K-weighting,
    400 ms blocks every 100 ms, the absolute gate at -70 LUFS and the relative gate 10 LU below the mean of what passed.  A float64
    0-dim tensor on the device (a CPU tensor is moved there first); -inf for less than 400 ms or when no block passes -70 LUFS.
    channel_weights: one per channel (default 1.0 each; BS.1770 gives the surround channels 1.41).  return_details: also the
    momentary maximum in LUFS and the numbers of blocks above the absolute gate and above both, as float64 0-dim tensors."""
    loud_ops.check_sample_rate(sample_rate)
    if not isinstance(waveform, th.Tensor) or waveform.dim() not in (1, 2):
        raise ValueError(f"a waveform (samples,) or (channels, samples) expected, got {getattr(waveform, 'shape', waveform)!r}")
    weights = loud_ops.check_weights(channel_weights, 1 if waveform.dim() == 1 else waveform.shape[0])
    x = _loudness_input(waveform)
    record = loud_ops.gate(loud_ops.segment_energies(x, sample_rate), sample_rate, weights)
    return (record[0], record[1], record[2], record[3]) if return_details else record[0]


def true_peak(waveform: th.Tensor) -> th.Tensor:
    """The largest magnitude, linear, among the samples of a float waveform (L,) or (C <= 8, L), L >= 1, and the points between
    them: the waveform interpolated 4x with the bank of `resample(waveform, 1, 4)` (Hann-windowed sinc, 4 phases of 15 taps, zeros
    beyond both ends).  A float32 0-dim tensor on the device; 20 log10 of it is dBTP."""
    return loud_ops.true_peak(_loudness_input(waveform, min_length=1))


def limit(waveform: th.Tensor, sample_rate: int, ceiling_dbtp: float = -1.0, gain_db: float = 0.0, attack_ms: float = 5.0,
          release_ms: float = 50.0, return_gain: bool = False):
    """Look-ahead true-peak limiter: waveform * 10^(gain_db / 20) * g in float32 on the device, in the waveform's shape ((L,) or
    (C <= 8, L); a CPU tensor is moved there first), with one gain curve g <= 1 for all channels, so that the stereo image does not
    move.  g holds every sample and the seven points of the 4x interpolation around it at or under 10^(ceiling_dbtp / 20) where they
    are scaled by that sample's gain: it looks attack_ms ahead (5 ms; round(attack_ms fs / 1000) samples, 0 .. 2047), falls over
    that time as the mean of a held minimum and recovers by the factor exp(-1 / (release_ms fs / 1000)) per sample (DESIGN.md,
    "True-peak limiter").  No sample of the result exceeds the ceiling; where nothing reaches it the result is waveform * gain
    exactly.  return_gain: also g, a float64 (L,) tensor on the device."""
    ceiling, lookahead, rho = lim_ops.check_arguments(sample_rate, ceiling_dbtp, attack_ms, release_ms)
    gain = 10.0 ** (lim_ops._number("gain_db", gain_db) / 20.0)
    x = _loudness_input(waveform)
    pregain = th.full((1,), gain, dtype=th.float64, device=x.device)
    out = lim_ops.limit(x, pregain, ceiling, lookahead, rho, return_gain=return_gain)
    if return_gain:
        return out[0].reshape(waveform.shape), out[1]
    return out.reshape(waveform.shape)


def _db20(v: th.Tensor) -> th.Tensor:
    return 20.0 * th.log10(v.to(th.float64))


def normalize_loudness(waveform: th.Tensor, sample_rate: int, target_lufs: float = -14.0, peak_dbtp: float = -1.0,
                       return_gain: bool = False, limiter: bool = False, attack_ms: float = 5.0, release_ms: float = 50.0,
                       passes: int = 2, return_details: bool = False):
    """waveform * gain in float32 on the device, in the waveform's shape, with one gain for all channels:
    gain = min(10^((target_lufs - loudness) / 20), 10^(peak_dbtp / 20) / true_peak) -- the target loudness unless the true-peak
    ceiling binds first; 1 where the loudness is -inf.  The gain is computed in float64 on the device, rounded once to float32 and
    never visits the host.  return_gain: also the gain, a float32 0-dim tensor on the device.
    limiter: the peaks that the target's gain would push past the ceiling are held under it by `limit` (attack_ms, release_ms)
    instead of lowering the whole file: y = limit(waveform, G) with G = 10^((target_lufs - loudness) / 20), `passes` times (1 .. 4),
    G multiplied before every pass but the first by 10^((target_lufs - loudness(y)) / 20) -- limiting lowers the loudness, and this
    hands the loss back -- then y * min(1, ceiling / true_peak(y)), so that the ceiling holds as `true_peak` measures it.  A fixed
    number of passes, every scalar on the device; the gain returned is the last G times that trim, float32.
    return_details: also (loudness in LUFS, true peak in dBTP, largest gain reduction of the limiter in dB) of the result, float64
    0-dim tensors on the device (the reduction is 0 without the limiter): the loudness reached is reported, not promised."""
    loud_ops.check_sample_rate(sample_rate)
    loud_ops.check_targets(target_lufs, peak_dbtp)
    if limiter:
        ceiling, lookahead, rho = lim_ops.check_arguments(sample_rate, peak_dbtp, attack_ms, release_ms)
        lim_ops.check_passes(passes)
    x = _loudness_input(waveform)
    reduction = th.zeros((), dtype=th.float64, device=x.device) if return_details else None
    if x.shape[1] < 1:
        out, gain = x.clone(), th.ones((), dtype=th.float32, device=x.device)
    elif not limiter:
        x = x.contiguous()
        record = loud_ops.gate(loud_ops.segment_energies(x, sample_rate), sample_rate)
        out, gain = loud_ops.normalize(x, record, loud_ops.true_peak(x), target_lufs, peak_dbtp)
    else:
        x = x.contiguous()
        pregain = lim_ops.pregain(loud_ops.gate(loud_ops.segment_energies(x, sample_rate), sample_rate), target_lufs)
        for i in range(passes):
            if i > 0:
                record = loud_ops.gate(loud_ops.segment_energies(y, sample_rate), sample_rate)
                pregain = lim_ops.pregain(record, target_lufs, prev=pregain)
            want_curve = return_details and i == passes - 1
            y = lim_ops.limit(x, pregain, ceiling, lookahead, rho, return_gain=want_curve)
            if want_curve:
                y, curve = y
                reduction = -_db20(curve.min())
        peak = loud_ops.true_peak(y)
        out = lim_ops.trim(y, peak, ceiling)
        gain = (pregain[0] * th.clamp(ceiling / peak.to(th.float64), max=1.0)).to(th.float32) if return_gain else None
    out = out.reshape(waveform.shape)
    result = (out, gain) if return_gain else (out,)
    if return_details:
        if out.numel() and x.shape[1] >= 1:
            flat = out.reshape(x.shape)
            lufs = loud_ops.gate(loud_ops.segment_energies(flat, sample_rate), sample_rate)[0]
            details = (lufs, _db20(loud_ops.true_peak(flat)), reduction)
        else:
            ninf = th.full((), -math.inf, dtype=th.float64, device=x.device)
            details = (ninf, ninf.clone(), reduction)
        result = result + (details,)
    return result if len(result) > 1 else out


def _limiter_keywords(loudness, limiter, attack_ms, release_ms, sample_rate, peak_dbtp) -> dict:
    """the limiter's keywords for `normalize_loudness`, checked; empty without the limiter"""
    if not limiter:
        return {}
    if loudness is None:
        raise ValueError("limiter needs loudness: it holds the peaks that the gain to a loudness target pushes past the ceiling")
    lim_ops.check_arguments(sample_rate, peak_dbtp, attack_ms, release_ms)
    return {"limiter": True, "attack_ms": attack_ms, "release_ms": release_ms}


def magn_phase_to_waveform(magn_phase: th.Tensor, griffin_lim: int = 0, momentum: float = 0.99, loudness=None,
                           peak_dbtp: float = -1.0, sample_rate: int = constant.SAMPLE_RATE, limiter: bool = False,
                           attack_ms: float = 5.0, release_ms: float = 50.0) -> th.Tensor:
    """griffin_lim: rounds of Griffin-Lim phase refinement from the decoded phase (0: none, the reference's single inversion);
    loudness: the integrated loudness in LUFS to bring the waveform to, under the true-peak ceiling peak_dbtp (None: the level the
    codec gives, as the reference), measured at `sample_rate`; limiter: hold the peaks under the ceiling with the look-ahead limiter
    (attack_ms, release_ms: as `limit`) instead of lowering the whole file when the ceiling binds -- needs `loudness`"""
    _check_magn_phase(magn_phase)
    if loudness is not None:
        loud_ops.check_targets(loudness, peak_dbtp)
    extra = _limiter_keywords(loudness, limiter, attack_ms, release_ms, sample_rate, peak_dbtp)
    if griffin_lim:
        wav = _griffin_lim(magn_phase, n_iter=griffin_lim, momentum=momentum)
    else:
        dev = magn_phase.device if magn_phase.is_cuda else _device()
        mp = magn_phase.to(dev, th.float32).contiguous()
        wav = ops.codec_inv(mp, _bark_vector(constant.N_FFT // 2, dev))
    return wav if loudness is None else normalize_loudness(wav, sample_rate, loudness, peak_dbtp, **extra)


def magn_phase_to_wav(magn_phase: th.Tensor, wav_path: str, sample_rate: int, griffin_lim: int = 0, momentum: float = 0.99,
                      loudness=None, peak_dbtp: float = -1.0, limiter: bool = False, attack_ms: float = 5.0,
                      release_ms: float = 50.0):
    """loudness / peak_dbtp / limiter / attack_ms / release_ms: as `magn_phase_to_waveform`; the file is normalised after
    Griffin-Lim and before the writer"""
    extra = {} if loudness is None else {"loudness": loudness, "peak_dbtp": peak_dbtp, "sample_rate": sample_rate}
    if limiter:
        extra.update(limiter=True, attack_ms=attack_ms, release_ms=release_ms)
    raw_audio = magn_phase_to_waveform(magn_phase, griffin_lim=griffin_lim, momentum=momentum, **extra)
    wavio.save(wav_path, raw_audio[None, :], sample_rate)

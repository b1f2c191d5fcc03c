"""Public surface of the reference's `audio` package (/root/reference/music_gan/audio/__init__.py) plus the two
waveform-level helpers the drivers use (`stft_from_waveform`, `magn_phase_to_waveform`), `resample`
(torchaudio.functional.resample, what the reference's users call for files that are not at 44.1 kHz), `istft` (the inverse of
`stft_from_waveform`), `griffin_lim` (torchaudio.functional.griffinlim on a magnitude / phase image) and `phase_vocoder`,
`time_stretch`, `pitch_shift` (torchaudio.functional's, with a rational rate; `pitch_ratio` is the fraction a pitch stands for),
`loudness`, `true_peak`, `normalize_loudness`, `kweighting_coefficients` (ITU-R BS.1770-4 / EBU R128), `limit` (the look-ahead
true-peak limiter behind `normalize_loudness(limiter=True)`), and `hpss`, `harmonic`,
`percussive` (librosa's median-filtering harmonic / percussive separation; `time_stretch(..., preserve_transients=True)` rests on it),
and `mel_spectrogram` (torchaudio.transforms.MelSpectrogram at 1024 / 256, HTK scale: the mel power of waveforms in one launch)."""
from . import constant as _constant
from . import functions as _functions
from .constant import N_FFT, N_VEC, SAMPLE_RATE, STFT_STRIDE
from .dataset import (AudioDataset, PackedAudioDataset, PackedLoader, ResidentDataset, ResidentLoader, WindowBatch, has_packed,
                      window_offsets, write_packed)
from .transforms import ChangeRange, ChannelMinMaxNorm

for _name in ("wav_to_stft", "stft_to_phase_magn", "magn_phase_to_wav", "bark_magn_scale", "stft_from_waveform",
              "magn_phase_to_waveform", "stft_to_stacked_phase_magn", "resample", "istft", "griffin_lim", "phase_vocoder", "time_stretch",
              "pitch_shift", "pitch_ratio", "loudness", "true_peak", "normalize_loudness", "kweighting_coefficients", "hpss", "harmonic",
              "percussive", "limit", "mel_spectrogram"):
    globals()[_name] = getattr(_functions, _name)
del _name

__all__ = ["wav_to_stft", "stft_to_phase_magn", "magn_phase_to_wav", "bark_magn_scale", "stft_from_waveform",
           "magn_phase_to_waveform", "stft_to_stacked_phase_magn", "resample", "istft", "griffin_lim", "phase_vocoder", "time_stretch",
           "pitch_shift", "pitch_ratio", "loudness", "true_peak", "normalize_loudness", "kweighting_coefficients", "hpss", "harmonic",
           "percussive", "limit", "mel_spectrogram", "AudioDataset", "PackedAudioDataset", "PackedLoader",
           "ResidentDataset", "ResidentLoader", "WindowBatch", "window_offsets", "has_packed", "write_packed", "ChannelMinMaxNorm", "ChangeRange", *_constant.__all__]

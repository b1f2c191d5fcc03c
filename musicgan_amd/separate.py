"""`python -m musicgan_amd separate AUDIO -o OUTDIR [--format wav|flac|ogg] [--kernel 31] [--margin 1] [--resample]`: the harmonic
and the percussive component of one recording (audio.hpss, median filtering on the GPU), written as `harmonic.*` and `percussive.*`
for listening -- what `create_dataset --component` would code, and what `--preserve-transients` re-times apart.  The reference has
no counterpart."""
import os

from . import audio, hpss_ops
from .audio import wavio

FORMATS = ("wav", "flac", "ogg")


def separate(audio_path: str, output_dir: str, *, audio_format: str = "wav", kernel_size=31, margin=1.0, resample: bool = False) -> dict:
    """Write OUTDIR/harmonic.<format> and OUTDIR/percussive.<format>, mono at 44.1 kHz, 256 * (frames - 1) samples each for the
    file's `frames` STFT frames; returns {"harmonic": path, "percussive": path, "samples": n}.  kernel_size, margin: as audio.hpss
    takes them; resample: a file that is not at 44.1 kHz is resampled (else it is refused)."""
    if audio_format not in FORMATS:
        raise ValueError(f"audio_format must be one of {FORMATS}, got {audio_format!r}")
    hpss_ops.check_arguments(kernel_size, 2.0, margin)
    spectrum = audio.wav_to_stft(audio_path, resample=resample)
    os.makedirs(output_dir, exist_ok=True)
    out = {}
    for name, part in zip(("harmonic", "percussive"), audio.hpss(spectrum, kernel_size=kernel_size, margin=margin)):
        wav = audio.istft(part)
        out[name] = os.path.join(output_dir, f"{name}.{audio_format}")
        wavio.save(out[name], wav[None, :], audio.SAMPLE_RATE)
        out["samples"] = int(wav.shape[0])
    print(f"{audio_path}: {out['samples']} samples each in {out['harmonic']} and {out['percussive']}")
    return out

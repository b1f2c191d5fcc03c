"""`python -m musicgan_amd loudness "GLOB" [-o out.json]`: integrated loudness, momentary maximum (LUFS, ITU-R BS.1770-4 / EBU
R128) and true peak (dBTP) of every readable audio file, measured on the GPU -- the measuring half of `generate --loudness`, and a
tool for corpora.  The reference has no counterpart."""
import glob
import json
import math

import torch

from . import audio
from .audio import wavio


def _db(v: float) -> float:
    return 20.0 * math.log10(v) if v > 0 else -math.inf


def _fmt(v: float) -> str:
    return f"{v:8.3f}" if math.isfinite(v) else f"{v!s:>8}"


def measure(path: str) -> dict:
    """{"path", "sample_rate", "channels", "seconds", "integrated_lufs", "momentary_max_lufs", "true_peak_dbtp"} of one file"""
    wav, sample_rate = wavio.load(path)
    if wav.shape[0] > 8:
        raise ValueError(f"{path}: {wav.shape[0]} channels (at most 8 are measured)")
    if wav.shape[1] < 1:
        raise ValueError(f"{path}: no samples")
    x = wav.to(torch.device("cuda", torch.cuda.current_device()))
    lufs, top, _, _ = audio.loudness(x, sample_rate, return_details=True)
    peak = audio.true_peak(x)
    return {"path": path, "sample_rate": sample_rate, "channels": int(wav.shape[0]), "seconds": wav.shape[1] / sample_rate,
            "integrated_lufs": float(lufs), "momentary_max_lufs": float(top), "true_peak_dbtp": _db(float(peak))}


def loudness(audio_path: str, output: str = None) -> list:
    """Measure every file `audio_path` (a glob) matches, in sorted order; a file that cannot be read is reported and left out.
    Prints one line per file and returns the list of `measure` records; `output`: also written there as JSON (-inf as -Infinity)."""
    paths = sorted(glob.glob(audio_path))
    if not paths:
        raise FileNotFoundError(f"no file matches \"{audio_path}\"")
    results = []
    print(f"{'LUFS':>8} {'max M':>8} {'dBTP':>8}  file")
    for path in paths:
        try:
            r = measure(path)
        except (ValueError, OSError, EOFError, AssertionError) as e:
            print(f"{'unreadable':>26}  {path}: {e}")
            continue
        results.append(r)
        print(f"{_fmt(r['integrated_lufs'])} {_fmt(r['momentary_max_lufs'])} {_fmt(r['true_peak_dbtp'])}  {path}")
    if output is not None:
        with open(output, "w") as fh:
            json.dump(results, fh, indent=1)
    return results

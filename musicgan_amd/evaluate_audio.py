"""`python -m musicgan_amd evaluate_audio "real/*.flac" "gen/*.wav" --metrics fd,kid,nn,prdc,ndb`: evaluate_mel's five metrics between
two sets of audio FILES, in the waveform log-mel space (metrics.WaveLogMel).  No checkpoint and no dataset are
involved, so this scores sound that did not come from one of this package's generators: another model's output, the reference
implementation's files, an .ogg at quality 3 against its .wav.  Every file is read through the package's loaders (wav / aiff / au /
flac / ogg), averaged to mono, and cut into windows of 512 frames (130 816 samples, 2.97 s: what one 512 x 512 image spans) every 512
frames; a window is a row, as an image is in evaluate_mel.  Single GPU."""
import glob
import json
from typing import Dict, List, Optional, Sequence

import torch

from . import audio
from .audio import wavio
from .evaluate_mel import METRICS_ALL, _RUNNERS, _PowerRows, _check


class _AudioWindows(_PowerRows):
    """A row-backed source with _Images' interface: `real(indices)` / `fake(rows)` hand out the mel power (B, 64, 512) of windows of
    the first / second set of files.  Each file's mel power (64, T) stays on the device (a 10-minute file: 6.6 MB) and a window is
    cut from it when it is asked for; `pairs[s][i]` = (file, window) of row i of set s, after the seeded cut to n rows."""

    def __init__(self, powers, pairs, batch_size: int, device) -> None:
        self.powers, self.pairs, self.batch_size, self.device = powers, pairs, batch_size, device
        self.side = self._WINDOW
        self._setup_rows("waveform log-mel")

    def _rows(self, which: int, rows) -> torch.Tensor:
        if isinstance(rows, slice):
            rows = range(*rows.indices(len(self.pairs[which])))
        w = self._WINDOW
        return torch.stack([self.powers[which][f][:, n * w:(n + 1) * w] for f, n in (self.pairs[which][i] for i in rows)]).contiguous()

    def real(self, indices) -> torch.Tensor:
        return self._rows(0, indices)

    def fake(self, rows) -> torch.Tensor:
        return self._rows(1, rows)

    def batches(self, n: int):
        for lo in range(0, n, self.batch_size):
            yield lo, min(lo + self.batch_size, n)


def _mono(path: str, resample: bool, device) -> torch.Tensor:
    """the file's mono mean at 44.1 kHz on the device, (L,) float32"""
    wav, sample_rate = wavio.load(path)
    if wav.dim() != 2 or wav.shape[1] < 1:
        raise ValueError("no samples")
    mono = wav.to(device).mean(0)
    if sample_rate != audio.SAMPLE_RATE:
        if not resample:
            raise ValueError(f"sample rate {sample_rate} Hz, {audio.SAMPLE_RATE} expected (resample=True / --resample converts it)")
        mono = audio.resample(mono, sample_rate, audio.SAMPLE_RATE)
    return mono.contiguous()


def _read_set(pattern: str, what: str, rows, resample: bool, device):
    """(mel power per usable file, [(file, window)] of every window) of the files `pattern` matches, in sorted order; a file that
    cannot be read or is shorter than one window is reported and left out"""
    paths = sorted(glob.glob(pattern))
    if not paths:
        raise FileNotFoundError(f"no file matches \"{pattern}\"")
    powers, pairs = [], []
    for path in paths:
        try:
            mono = _mono(path, resample, device)
        except (ValueError, OSError, EOFError, AssertionError) as e:
            print(f"{'unreadable':>12}  {path}: {e}")
            continue
        count = rows.windows(mono.shape[0])
        if count < 1:
            print(f"{'too short':>12}  {path}: {mono.shape[0]} samples are fewer than one window of {256 * (rows.window - 1)}")
            continue
        pairs += [(len(powers), n) for n in range(count)]
        powers.append(rows.power(mono[None])[0])
        print(f"{count:>4} windows  {path}")
    print(f"{what}: {len(pairs)} windows of {len(powers)} of {len(paths)} files")
    return powers, pairs


def evaluate_audio(real_path: str, fake_path: str, metrics: Sequence[str] = ("fd",), *, nb_windows: int = 8192, seed: int = 0,
                   resample: bool = False, batch_size: int = 16, output: Optional[str] = None) -> Dict[str, float]:
    """`real_path`, `fake_path`: globs of audio files, the reference set and the set to be judged.  `metrics`: a subset of
    ("fd", "nn", "prdc", "ndb", "kid"), run in that order, with evaluate_mel's keys, counts and printed lines: every "image" there is
    a window of 512 frames here, and the `_real` figures compare two random halves of the first glob's windows.  Both sets are cut to
    n = min(windows of the first, windows of the second, nb_windows) windows by one seeded permutation each, so the two sets have
    equal sizes (fd's bias depends on them).  `resample`: files at another rate than 44.1 kHz are resampled (else they are reported
    and left out, like unreadable files and files shorter than one window).  The least n a metric takes is evaluate_mel's.
    Returns the keys of the metrics asked for and writes them as JSON to `output`."""
    metrics = tuple(metrics)
    if not metrics or any(m not in METRICS_ALL for m in metrics) or len(set(metrics)) != len(metrics):
        raise ValueError(f"metrics: a non-empty subset of {METRICS_ALL} expected, got {metrics}")
    if nb_windows < 1 or batch_size < 1:
        raise ValueError("nb_windows and batch_size must be positive")
    _check(metrics, nb_windows)   # before any work ...
    device = torch.device("cuda", torch.cuda.current_device())
    source = _AudioWindows([[], []], [[], []], batch_size, device)
    sets: List = [_read_set(p, what, source.wave_rows, resample, device) for p, what in ((real_path, "real"), (fake_path, "fake"))]
    n = min(len(sets[0][1]), len(sets[1][1]), nb_windows)
    _check(metrics, n)            # ... and for what the files hold
    for which, (powers, pairs) in enumerate(sets):
        order = torch.randperm(len(pairs), generator=torch.Generator().manual_seed(seed + which)).tolist()[:n]
        source.powers[which], source.pairs[which] = powers, [pairs[i] for i in order]
    print(f"Evaluate {n} real and {n} other windows of {source._WINDOW} frames...")
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()
    result = {}
    for name in METRICS_ALL:
        if name in metrics:
            result.update(_RUNNERS[name](source, n, perm, seed))
    if output is not None:
        with open(output, "w") as f:
            json.dump(result, f, indent=1)
    return result

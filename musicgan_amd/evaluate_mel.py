"""Evaluation in a perceptual feature space: `evaluate_mel(gen_dict_state, rand_channels, input_dataset)` does what `evaluate` does
-- loads a generator saved by train(), draws as many samples as it reads from the dataset -- and compares the two sets in the
log-mel spectrogram of what each image decodes to (metrics.LogMel) instead of in pixels.  Pixel distances weigh the
phase-delta channel, which is close to noise for music, as much as the magnitude, and the magnitude linearly, so that a few loud
bins decide; the log-mel rows drop the phase, weigh the power by mel band and compress it logarithmically, as every audio evaluation
does.  "fd": the Frechet distance between the Gaussians fitted to the two sets of rows (the formula of FID; no pretrained network is
involved).  "nn", "prdc", "ndb": evaluate's own runners on log-mel rows instead of 128 x 128 pixels.  "kid" (in METRICS_ALL, not in
METRICS): the Kernel Inception Distance on the rows of "fd", whose expectation does not depend on the set sizes (metrics.KID).
`evaluate_mel_waveform` takes every row from the waveform an image decodes to instead of from its magnitude channel
(metrics.WaveLogMel): there the phase channel counts.  Single GPU."""
import functools
import json
import sys
from typing import Dict, Optional, Sequence

import torch

_first = f"{__package__}.evaluate" not in sys.modules
from .evaluate import _FINAL_LEVEL, _FULL_SIDE, _Images, _check_sizes, _ndb, _nn, _open, _prdc, evaluate  # noqa: E402
from .metrics import KID, LogMel, WaveLogMel, frechet_distance, kid_subsets  # noqa: E402
from . import audio, mel_ops  # noqa: E402

if _first:   # the import system has just bound the sub-module over the package's lazily exported function `evaluate`: put it back
    setattr(sys.modules[__package__], "evaluate", evaluate)

METRICS = ("fd", "nn", "prdc", "ndb")
METRICS_ALL = METRICS + ("kid",)
_MIN_LEVEL = 4        # 64 x 64: LogMel needs 64 rows (8 bands)
_FD_POOLS = 8         # time pools of the Frechet rows: 64 x 8 = 512 dimensions at level 7, 16 images per dimension at 8192
_FD_MIN_IMAGES = 4    # two halves of two rows
_KID_SUBSETS, _KID_SUBSET_SIZE = 100, 1000   # the protocol of Binkowski et al. 2018
_KID_MIN_IMAGES = 4   # two halves of two rows
# kid draws its generated images in batches of this many, whatever batch_size is: the generator's kernels are chosen by the batch
# size, so the images differ in their last float32 bits from one batching to another, and a number that is there to be compared
# across runs must not move with --batch-size.  16 is every driver's default: a default run draws exactly evaluate's images.
_KID_FAKE_BATCH = 16


def _name_spaces(images, name: str, rows, fd_rows) -> None:
    """how the printed lines name the two row spaces of an image source, and the numbers in a row of each"""
    what = f"{rows.bands} bands x {rows.pools} pools"
    images.space, images.row_what, images.row_numel = f"in {name} space ({what})", f"{name} rows of {what}", rows.dims
    images.fd_what, images.fd_dims, images.fd_name = f"{fd_rows.bands} bands x {fd_rows.pools} pools", fd_rows.dims, name


class _MelImages(_Images):
    """evaluate's image source with log-mel rows where it has reduced pixels: what nn, prdc and ndb compare (`reduced`), and the
    rows of fewer pools that fd and kid compare (`fd_rows`)"""

    def __init__(self, dataset, gen, latents: torch.Tensor, side: int, batch_size: int) -> None:
        super().__init__(dataset, gen, latents, side, batch_size)
        self.logmel = LogMel(side, side)
        self.fd_logmel = LogMel(side, side, pools=min(_FD_POOLS, side // 8))
        _name_spaces(self, "log-mel", self.logmel, self.fd_logmel)

    def reduced(self, x: torch.Tensor) -> torch.Tensor:
        return self.logmel(x)

    def fd_rows(self, x: torch.Tensor) -> torch.Tensor:
        return self.fd_logmel(x)


class _PowerRows:
    """What the sources below share: `real` and `fake` hand out the mel power (B, 64, 512) of one window of sound per row, and the
    rows are pooled from it on demand -- 32 pools for nn, prdc and ndb, 8 for fd and kid."""
    _WINDOW = _FULL_SIDE   # frames of a row: what a 512 x 512 image spans

    def _setup_rows(self, name: str) -> None:
        self.wave_rows = WaveLogMel(pools=32, window=self._WINDOW, hop=self._WINDOW)
        self.wave_fd_rows = WaveLogMel(pools=_FD_POOLS, window=self._WINDOW, hop=self._WINDOW)
        _name_spaces(self, name, self.wave_rows, self.wave_fd_rows)

    def reduced(self, power: torch.Tensor) -> torch.Tensor:
        return self.wave_rows.pool(power)

    def fd_rows(self, power: torch.Tensor) -> torch.Tensor:
        return self.wave_fd_rows.pool(power)


class _WaveMelImages(_PowerRows, _MelImages):
    """the rows of the waveform every image decodes to: each image on its own (the codec's inverse joins a batch along time, and a
    row must depend on its image alone), the generated ones after `griffin_lim` rounds of phase refinement, the real ones as the
    codec gives them -- the data's own phase is the ground truth.  The waveforms of a batch are stacked for one mel_power launch."""

    def __init__(self, dataset, gen, latents: torch.Tensor, side: int, batch_size: int, griffin_lim: int = 0) -> None:
        _Images.__init__(self, dataset, gen, latents, side, batch_size)
        self.griffin_lim = griffin_lim
        self._setup_rows("waveform log-mel")

    def _power(self, x: torch.Tensor, griffin_lim: int) -> torch.Tensor:
        waves = torch.stack([audio.magn_phase_to_waveform(x[i:i + 1], griffin_lim=griffin_lim) for i in range(x.shape[0])])
        return self.wave_rows.power(waves.contiguous())   # (B, 130816): 512 frames, one window

    def real(self, indices) -> torch.Tensor:
        return self._power(super().real(indices), 0)

    def fake(self, rows) -> torch.Tensor:
        return self._power(super().fake(rows), self.griffin_lim)


def _fd(images: _Images, nb_images: int, perm, seed: int) -> Dict[str, float]:
    half = nb_images // 2
    # every image once: the rows of a set are a few MB, and a real image's row does not depend on the batch it was read in
    real = torch.cat([images.fd_rows(images.real(range(lo, hi))) for lo, hi in images.batches(nb_images)])
    fake = torch.cat([images.fd_rows(images.fake(slice(lo, hi))) for lo, hi in images.batches(nb_images)])
    first = real[torch.tensor(perm[:half], device=real.device)].contiguous()
    second = real[torch.tensor(perm[half:2 * half], device=real.device)].contiguous()
    sets = {"fd": (real, fake), "fd_half": (first, fake[:half].contiguous()), "fd_real": (first, second)}
    moments = {}   # a set's moments are taken once (the first half of the real set is in two of the three)

    def host_moments(rows: torch.Tensor):
        key = rows.data_ptr(), rows.shape[0]
        if key not in moments:
            moments[key] = tuple(t.cpu() for t in mel_ops.moments(rows))
        return moments[key]

    result = {name: frechet_distance(*host_moments(a), *host_moments(b)) for name, (a, b) in sets.items()}
    space = f"in {images.fd_name} space ({images.fd_what})"
    for name, (a, b) in sets.items():
        print(f"FD [{name:>7}] = {result[name]:.6f} {space}, {a.shape[0]} real against {b.shape[0]} "
              f"{'real' if name == 'fd_real' else 'generated'} images")
    print("FD: fd_half near fd_real is what a perfect generator scores: fd_real is one random half of the data against the other, "
          "fd_half the first half of the samples against one half of the data -- the same set sizes, because the estimator's bias "
          "grows as the sets shrink")
    if half < 2 * images.fd_dims:
        print(f"FD: {half} images per half are fewer than twice the {images.fd_dims} dimensions: fd is dominated by its bias")
    return result


def _kid(images: _Images, nb_images: int, perm, seed: int) -> Dict[str, float]:
    half = nb_images // 2
    kid = KID(_KID_SUBSETS, _KID_SUBSET_SIZE, seed)                   # on the rows of fd
    for lo, hi in images.batches(nb_images):
        kid.feed_real(images.fd_rows(images.real(range(lo, hi))))
    for lo in range(0, nb_images, _KID_FAKE_BATCH):
        kid.feed_fake(images.fd_rows(images.fake(slice(lo, min(lo + _KID_FAKE_BATCH, nb_images)))))
    result = kid.result()
    # the two random halves of the real set that fd_real compares, standardised by the whole real set's moments like everything else
    real = kid.standardised()[0]
    first = real[torch.tensor(perm[:half], device=real.device)].contiguous()
    second = real[torch.tensor(perm[half:2 * half], device=real.device)].contiguous()
    result["kid_real"], result["kid_real_std"] = kid_subsets(first, second, _KID_SUBSETS, _KID_SUBSET_SIZE, seed)
    space = f"in {images.fd_name} space ({images.fd_what}, standardised by the real images' moments)"
    m, m_real = min(_KID_SUBSET_SIZE, nb_images), min(_KID_SUBSET_SIZE, half)
    count = lambda m, n: "1 subset" if m == n else f"{_KID_SUBSETS} subsets"   # noqa: E731
    print(f"KID [     kid] = {result['kid']:.6f} +- {result['kid_std']:.6f} {space}, {count(m, nb_images)} of {m} real against "
          f"{m} generated images")
    print(f"KID [kid_full] = {result['kid_full']:.6f} {space}, {nb_images} real against {nb_images} generated images")
    print(f"KID [kid_real] = {result['kid_real']:.6f} +- {result['kid_real_std']:.6f} {space}, "
          f"{count(m_real, half)} of {m_real} real against {m_real} real images")
    print("KID: the unbiased estimate of the squared MMD under k(x, y) = (x.y / d + 1)^3: its expectation does not depend on the "
          "set sizes and is 0 for two samples of one distribution, so it can be negative; kid_real (one random half of the data "
          "against the other) shows how far from 0 chance alone puts it")
    return result


# metric: its runner; nn, prdc and ndb are evaluate's, their least image counts with them
_RUNNERS = {"fd": _fd, "nn": _nn, "prdc": _prdc, "ndb": _ndb, "kid": _kid}
assert tuple(_RUNNERS) == METRICS_ALL


def _check(metrics: Sequence[str], nb_images: int) -> None:
    if "fd" in metrics and nb_images < _FD_MIN_IMAGES:
        raise ValueError(f"fd needs at least {_FD_MIN_IMAGES} images (two halves of two), got {nb_images}")
    if "kid" in metrics and nb_images < _KID_MIN_IMAGES:
        raise ValueError(f"kid needs at least {_KID_MIN_IMAGES} images (two halves of two), got {nb_images}")
    _check_sizes(metrics, nb_images)


def evaluate_mel(gen_dict_state: str, rand_channels: int, input_dataset: str, metrics: Sequence[str] = ("fd",), *,
                 level: int = _FINAL_LEVEL, nb_images: int = 8192, batch_size: int = 16, seed: int = 0,
                 output: Optional[str] = None) -> Dict[str, float]:
    """`level`: the growth level the checkpoint was saved at, 4 (64 x 64) .. 7 (fully grown, 512 x 512); real samples are brought to
    that level's side by the training loop's own input transform and are not reduced further.  `metrics`: a subset of ("fd", "nn",
    "prdc", "ndb", "kid"), run in that order.  The images, the one draw of latents and the seeded order of the dataset are evaluate's for
    the same arguments.  Returns the keys of the metrics asked for and writes them as JSON to `output`.

    "fd": rows are LogMel(side, side, pools=min(8, side // 8)) -- side // 8 mel bands x 8 time pools, 512 dimensions at level 7.
    `fd` = the Frechet distance of all generated against all real images; `fd_half` = the first nb_images // 2 generated images
    against one random half of the real ones; `fd_real` = that half against the other random half.  The estimate is biased upwards
    by an amount that grows as the sets shrink and the dimensions grow, so `fd` is not comparable across set sizes; `fd_half` and
    `fd_real` have the same set sizes, and `fd_half` near `fd_real` is what a perfect generator scores.  Needs nb_images >= 4.

    "nn", "prdc", "ndb": evaluate's runners with the same counts, queries and keys, on LogMel(side, side) rows (side // 8 bands x
    min(32, side // 8) pools) instead of pixels at 128 x 128; their lines name the space.

    "kid" (not in the default tuple METRICS; METRICS_ALL has it): the rows of "fd", standardised column by column with the real
    set's float64 mean and standard deviation.  `kid` / `kid_std` = the mean and population standard deviation, over 100 random
    subsets of min(1000, nb_images) images of each set, of the unbiased estimate of the squared maximum mean discrepancy under
    k(x, y) = (x.y / d + 1)^3 (Binkowski et al. 2018; one subset and a deviation of 0.0 if that is all images); `kid_full` = the
    estimate on the whole sets; `kid_real` / `kid_real_std` = the same protocol for the two random halves of the real set that
    `fd_real` compares, whose expectation is 0.  Unlike `fd`, the estimate's expectation does not depend on the set sizes, so runs
    at different nb_images can be compared; it can be negative.  The generated images of "kid" are drawn in batches of 16 whatever
    `batch_size` is (the real ones in batches of `batch_size`; a real row does not depend on its batch), so none of the five numbers
    depends on `batch_size`; at the default batch size they are the images of the other metrics.  Needs nb_images >= 4.

    `evaluate_mel_waveform` takes the same rows from the waveform every image decodes to instead."""
    if not _MIN_LEVEL <= level <= _FINAL_LEVEL:
        raise ValueError(f"level must be in {_MIN_LEVEL} .. {_FINAL_LEVEL} (log-mel rows need at least 64 image rows), got {level}")
    if nb_images < 1 or batch_size < 1:
        raise ValueError("nb_images and batch_size must be positive")
    metrics = tuple(metrics)
    if not metrics or any(m not in METRICS_ALL for m in metrics) or len(set(metrics)) != len(metrics):
        raise ValueError(f"metrics: a non-empty subset of {METRICS_ALL} expected, got {metrics}")
    _check(metrics, nb_images)   # before any work ...
    return _run(_MelImages, metrics, gen_dict_state, rand_channels, input_dataset, level, nb_images, batch_size, seed, output)


def _run(source, metrics, gen_dict_state, rand_channels, input_dataset, level, nb_images, batch_size, seed, output) -> Dict[str, float]:
    """the checked arguments of either driver: open `source`, run the metrics in METRICS_ALL's order, write `output`"""
    images, nb_images, perm = _open(source, lambda n: _check(metrics, n), gen_dict_state, rand_channels, input_dataset, level,
                                    nb_images, batch_size, seed)
    result = {}
    for name in METRICS_ALL:
        if name in metrics:
            result.update(_RUNNERS[name](images, nb_images, perm, seed))
    if output is not None:
        with open(output, "w") as f:
            json.dump(result, f, indent=1)
    return result


def evaluate_mel_waveform(gen_dict_state: str, rand_channels: int, input_dataset: str, metrics: Sequence[str] = ("fd",), *,
                          level: int = _FINAL_LEVEL, nb_images: int = 8192, batch_size: int = 16, seed: int = 0,
                          output: Optional[str] = None, griffin_lim: int = 0) -> Dict[str, float]:
    """`evaluate_mel` -- the same arguments, images, metrics, keys and counts -- with every row, of all five metrics, taken from the
    WAVEFORM its image decodes to (metrics.WaveLogMel) instead of from the image's channel 0, so that the phase
    channel counts: inconsistent phases cancel and smear energy in the overlap-add, and only the sound shows it.  Each image is
    decoded on its own by audio.magn_phase_to_waveform -- generated ones after `griffin_lim` rounds of Griffin-Lim (what `generate
    --griffin-lim N` writes), real ones with the data's own phase --, a batch's waveforms go through one mel_power launch, and the
    rows have 64 bands x 8 pools (fd, kid) or x 32 pools (nn, prdc, ndb) as in evaluate_mel at level 7.  The printed lines say "in
    waveform log-mel space".  Level 7 only: the codec's inverse needs 512 rows.  On the command line: `evaluate_mel --waveform
    [--griffin-lim N]`.  (A function of its own, not two more keywords of evaluate_mel: that function's parameter list is part of
    what its tests pin.)"""
    if isinstance(griffin_lim, bool) or not isinstance(griffin_lim, int) or griffin_lim < 0:
        raise ValueError(f"griffin_lim: a number of rounds >= 0 expected, got {griffin_lim!r}")
    if level != _FINAL_LEVEL:
        raise ValueError(f"waveform rows need level {_FINAL_LEVEL}: the codec's inverse takes images of 512 rows, got level {level}")
    if nb_images < 1 or batch_size < 1:
        raise ValueError("nb_images and batch_size must be positive")
    metrics = tuple(metrics)
    if not metrics or any(m not in METRICS_ALL for m in metrics) or len(set(metrics)) != len(metrics):
        raise ValueError(f"metrics: a non-empty subset of {METRICS_ALL} expected, got {metrics}")
    _check(metrics, nb_images)   # before any work ...
    return _run(functools.partial(_WaveMelImages, griffin_lim=griffin_lim), metrics, gen_dict_state, rand_channels, input_dataset,
                level, nb_images, batch_size, seed, output)

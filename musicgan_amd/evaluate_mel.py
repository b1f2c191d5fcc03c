"""Evaluation in a perceptual feature space: `evaluate_mel(gen_dict_state, rand_channels, input_dataset)` does what `evaluate` does
-- loads a generator saved by train(), draws as many samples as it reads from the dataset -- and compares the two sets in the
log-mel spectrogram of what each image decodes to (metrics.LogMel) instead of in pixels.  Pixel distances weigh the
phase-delta channel, which is close to noise for music, as much as the magnitude, and the magnitude linearly, so that a few loud
bins decide; the log-mel rows drop the phase, weigh the power by mel band and compress it logarithmically, as every audio evaluation
does.  "fd": the Frechet distance between the Gaussians fitted to the two sets of rows (the formula of FID; no pretrained network is
involved).  "nn", "prdc", "ndb": evaluate's own runners on log-mel rows instead of 128 x 128 pixels.
Single GPU."""
import json
import sys
from typing import Dict, Optional, Sequence

import torch

_first = f"{__package__}.evaluate" not in sys.modules
from .evaluate import _FINAL_LEVEL, _Images, _check_sizes, _ndb, _nn, _open, _prdc, evaluate  # noqa: E402
from .metrics import LogMel, frechet_distance  # noqa: E402
from . import mel_ops  # noqa: E402

if _first:   # the import system has just bound the sub-module over the package's lazily exported function `evaluate`: put it back
    setattr(sys.modules[__package__], "evaluate", evaluate)

METRICS = ("fd", "nn", "prdc", "ndb")
_MIN_LEVEL = 4        # 64 x 64: LogMel needs 64 rows (8 bands)
_FD_POOLS = 8         # time pools of the Frechet rows: 64 x 8 = 512 dimensions at level 7, 16 images per dimension at 8192
_FD_MIN_IMAGES = 4    # two halves of two rows


class _MelImages(_Images):
    """evaluate's image source with log-mel rows where it has reduced pixels: what nn, prdc and ndb compare"""

    def __init__(self, dataset, gen, latents: torch.Tensor, side: int, batch_size: int) -> None:
        super().__init__(dataset, gen, latents, side, batch_size)
        self.logmel = LogMel(side, side)
        what = f"{self.logmel.bands} bands x {self.logmel.pools} pools"
        self.space, self.row_what, self.row_numel = f"in log-mel space ({what})", f"log-mel rows of {what}", self.logmel.dims

    def reduced(self, x: torch.Tensor) -> torch.Tensor:
        return self.logmel(x)


def _fd(images: _Images, nb_images: int, perm, seed: int) -> Dict[str, float]:
    half, side = nb_images // 2, images.side
    logmel = LogMel(side, side, pools=min(_FD_POOLS, side // 8))
    # every image once: the rows of a set are a few MB, and a real image's row does not depend on the batch it was read in
    real = torch.cat([logmel(images.real(range(lo, hi))) for lo, hi in images.batches(nb_images)])
    fake = torch.cat([logmel(images.fake(slice(lo, hi))) for lo, hi in images.batches(nb_images)])
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
    space = f"in log-mel space ({logmel.bands} bands x {logmel.pools} pools)"
    for name, (a, b) in sets.items():
        print(f"FD [{name:>7}] = {result[name]:.6f} {space}, {a.shape[0]} real against {b.shape[0]} "
              f"{'real' if name == 'fd_real' else 'generated'} images")
    print("FD: fd_half near fd_real is what a perfect generator scores: fd_real is one random half of the data against the other, "
          "fd_half the first half of the samples against one half of the data -- the same set sizes, because the estimator's bias "
          "grows as the sets shrink")
    if half < 2 * logmel.dims:
        print(f"FD: {half} images per half are fewer than twice the {logmel.dims} dimensions: fd is dominated by its bias")
    return result


# metric: its runner; nn, prdc and ndb are evaluate's, their least image counts with them
_RUNNERS = {"fd": _fd, "nn": _nn, "prdc": _prdc, "ndb": _ndb}
assert tuple(_RUNNERS) == METRICS


def _check(metrics: Sequence[str], nb_images: int) -> None:
    if "fd" in metrics and nb_images < _FD_MIN_IMAGES:
        raise ValueError(f"fd needs at least {_FD_MIN_IMAGES} images (two halves of two), got {nb_images}")
    _check_sizes(metrics, nb_images)


def evaluate_mel(gen_dict_state: str, rand_channels: int, input_dataset: str, metrics: Sequence[str] = ("fd",), *,
                 level: int = _FINAL_LEVEL, nb_images: int = 8192, batch_size: int = 16, seed: int = 0,
                 output: Optional[str] = None) -> Dict[str, float]:
    """`level`: the growth level the checkpoint was saved at, 4 (64 x 64) .. 7 (fully grown, 512 x 512); real samples are brought to
    that level's side by the training loop's own input transform and are not reduced further.  `metrics`: a subset of ("fd", "nn",
    "prdc", "ndb"), run in that order.  The images, the one draw of latents and the seeded order of the dataset are evaluate's for
    the same arguments.  Returns the keys of the metrics asked for and writes them as JSON to `output`.

    "fd": rows are LogMel(side, side, pools=min(8, side // 8)) -- side // 8 mel bands x 8 time pools, 512 dimensions at level 7.
    `fd` = the Frechet distance of all generated against all real images; `fd_half` = the first nb_images // 2 generated images
    against one random half of the real ones; `fd_real` = that half against the other random half.  The estimate is biased upwards
    by an amount that grows as the sets shrink and the dimensions grow, so `fd` is not comparable across set sizes; `fd_half` and
    `fd_real` have the same set sizes, and `fd_half` near `fd_real` is what a perfect generator scores.  Needs nb_images >= 4.

    "nn", "prdc", "ndb": evaluate's runners with the same counts, queries and keys, on LogMel(side, side) rows (side // 8 bands x
    min(32, side // 8) pools) instead of pixels at 128 x 128; their lines name the space."""
    if not _MIN_LEVEL <= level <= _FINAL_LEVEL:
        raise ValueError(f"level must be in {_MIN_LEVEL} .. {_FINAL_LEVEL} (log-mel rows need at least 64 image rows), got {level}")
    if nb_images < 1 or batch_size < 1:
        raise ValueError("nb_images and batch_size must be positive")
    metrics = tuple(metrics)
    if not metrics or any(m not in METRICS for m in metrics) or len(set(metrics)) != len(metrics):
        raise ValueError(f"metrics: a non-empty subset of {METRICS} expected, got {metrics}")
    _check(metrics, nb_images)   # before any work ...
    images, nb_images, perm = _open(_MelImages, lambda n: _check(metrics, n), gen_dict_state, rand_channels, input_dataset, level,
                                    nb_images, batch_size, seed)
    result = {}
    for name in METRICS:
        if name in metrics:
            result.update(_RUNNERS[name](images, nb_images, perm, seed))
    if output is not None:
        with open(output, "w") as f:
            json.dump(result, f, indent=1)
    return result

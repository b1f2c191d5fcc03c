"""Perceptual path length of a checkpoint: `path_length(gen_dict_state, rand_channels)` loads a generator saved by train() and
reports how fast its output moves, in the log-mel rows of `evaluate_mel`'s "fd" (metrics.LogMel, or with `waveform` metrics.WaveLogMel
on the sound every image decodes to), when the latent moves a step `epsilon` along the arc between two random latents (metrics.PPL,
DESIGN.md 4.22; Karras et al. 2019 with the squared row distance in the place of LPIPS).  Every other metric of the package compares
sets of samples; this one says whether the latent space between the samples is smooth -- whether `generate --morph-to` glides or
jumps.  It needs no dataset.  Single GPU."""
import json
from typing import Dict, Optional

import torch

_FINAL_LEVEL, _FULL_SIDE = 7, 512
_MIN_LEVEL = 4        # 64 x 64: LogMel needs 64 rows (8 bands)
_FD_POOLS = 8         # the time pools of evaluate_mel's "fd" rows
_MAX_EPSILON = 0.1
_LABELS = {"ppl": "the mean between the 1st and the 99th percentile", "ppl_mean": "the mean of all pairs",
           "ppl_chord": "the mean squared distance between the two ends of an arc",
           "ppl_ratio": "ppl_mean / ppl_chord", "ppl_pairs": "pairs used"}


def _check(level, nb_pairs, epsilon, sampling, seed, waveform, griffin_lim) -> None:
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)   # noqa: E731
    if not is_int(level) or not _MIN_LEVEL <= level <= _FINAL_LEVEL:
        raise ValueError(f"level must be in {_MIN_LEVEL} .. {_FINAL_LEVEL} (log-mel rows need at least 64 image rows), got {level!r}")
    if not is_int(griffin_lim) or griffin_lim < 0:
        raise ValueError(f"griffin_lim: a number of rounds >= 0 expected, got {griffin_lim!r}")
    if waveform and level != _FINAL_LEVEL:
        raise ValueError(f"waveform rows need level {_FINAL_LEVEL}: the codec's inverse takes images of 512 rows, got level {level}")
    if griffin_lim and not waveform:
        raise ValueError("griffin_lim needs waveform=True: the rows of the images have no phase to refine")
    if not is_int(nb_pairs) or nb_pairs < 2:
        raise ValueError(f"nb_pairs >= 2 expected, got {nb_pairs!r}")
    if isinstance(epsilon, bool) or not isinstance(epsilon, (int, float)) or not 0.0 < epsilon <= _MAX_EPSILON:
        raise ValueError(f"epsilon in (0, {_MAX_EPSILON}] expected, got {epsilon!r}")
    if sampling not in ("full", "end"):
        raise ValueError(f"sampling: \"full\" or \"end\" expected, got {sampling!r}")
    if not is_int(seed):
        raise ValueError(f"an integer seed expected, got {seed!r}")


def path_length(gen_dict_state: str, rand_channels: int, *, level: int = _FINAL_LEVEL, nb_pairs: int = 8192, epsilon: float = 1e-4,
                sampling: str = "full", seed: int = 0, output: Optional[str] = None, waveform: bool = False,
                griffin_lim: int = 0) -> Dict[str, float]:
    """`level`: the growth level the checkpoint was saved at, 4 (64 x 64) .. 7 (fully grown, 512 x 512).  For each of `nb_pairs`
    pairs of latents z0, z1 ~ N(0, I) and a position t ~ U[0, 1) (`sampling` "full") or t = 0 ("end"), all from one device generator
    seeded with `seed`, the generator draws the images of slerp(z0, z1, t) and slerp(z0, z1, t + epsilon) (project.slerp's arc, the
    one `generate --morph-to` walks) in one call, next to each other in a batch of 16, and
        d = |rows(first image) - rows(second image)|^2 / (D epsilon^2)
    with rows = LogMel(side, side, pools=min(8, side // 8)), the D numbers of evaluate_mel's "fd" rows; with `waveform` (level 7
    only) rows = WaveLogMel(pools=8) of the waveform each image decodes to after `griffin_lim` rounds of Griffin-Lim, as in
    evaluate_mel_waveform.  d is in nat^2 per dimension per unit of t.

    Returns, prints and writes as JSON to `output`: `ppl` = the mean of the d between their 1st and 99th percentile (the StyleGAN
    protocol: ranks floor(0.01 (n - 1)) and ceil(0.99 (n - 1)), both kept); `ppl_mean` = the mean of all d; with "full" sampling
    `ppl_chord` = the mean of |rows(G(z0)) - rows(G(z1))|^2 / D, the squared distance between the two ends of an arc, and
    `ppl_ratio` = ppl_mean / ppl_chord: the mean squared speed along the arcs over the squared length of their chords, which needs
    no scale, is >= 1 in expectation (not pair by pair) and 1 for straight paths walked at constant speed; `ppl_pairs` = the pairs
    used (a pair of antipodal latents has no single shortest arc and is left out).  No key depends on a batch size: there is none.
    Arguments are checked before the checkpoint is opened."""
    _check(level, nb_pairs, epsilon, sampling, seed, waveform, griffin_lim)
    if isinstance(rand_channels, bool) or not isinstance(rand_channels, int) or rand_channels < 1:
        raise ValueError(f"rand_channels >= 1 expected, got {rand_channels!r}")
    from . import audio
    from .metrics import PPL, LogMel, WaveLogMel
    from .networks import Generator
    side = _FULL_SIDE >> (_FINAL_LEVEL - level)
    device = torch.device("cuda", torch.cuda.current_device())

    print("Load model...")
    gen = Generator(rand_channels, end_layer=level)
    gen.load_state_dict(torch.load(gen_dict_state, map_location="cpu"))
    gen = gen.to(device).eval()

    def images(latents: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            return gen(latents, 1.0).contiguous()

    if waveform:
        rows, name = WaveLogMel(pools=_FD_POOLS, window=_FULL_SIDE, hop=_FULL_SIDE), "waveform log-mel"

        def rows_of(latents: torch.Tensor) -> torch.Tensor:   # each image decoded on its own: a row depends on its image alone
            x = images(latents)
            waves = torch.stack([audio.magn_phase_to_waveform(x[i:i + 1], griffin_lim=griffin_lim) for i in range(x.shape[0])])
            return rows(waves.contiguous())
    else:
        rows, name = LogMel(side, side, pools=min(_FD_POOLS, side // 8)), "log-mel"

        def rows_of(latents: torch.Tensor) -> torch.Tensor:
            return rows(images(latents))

    print(f"Walk {nb_pairs} pairs of latents, epsilon = {epsilon:g}, {sampling} sampling, images of {side} x {side}...")
    ppl = PPL(rows_of, epsilon, sampling, seed, rand_channels=rand_channels)
    ppl.feed(nb_pairs)
    result = ppl.result()
    space = f"in {name} space ({rows.bands} bands x {rows.pools} pools)"
    for key, value in result.items():
        shown = f"{value}" if key == "ppl_pairs" else f"{value:.6f}"
        print(f"PPL [{key:>9}] = {shown} {space}: {_LABELS[key]}")
    if "ppl_ratio" in result:
        print("PPL: ppl_ratio is the mean squared speed along the arcs over the mean squared length of their chords, so it needs no "
              "scale: 1 for straight paths walked at constant speed in row space, and the further above 1 the more the images "
              "wander or rush between two latents (>= 1 in expectation, not pair by pair)")
    if result["ppl_pairs"] < nb_pairs:
        print(f"PPL: {nb_pairs - result['ppl_pairs']} pairs of antipodal latents were left out")
    if output is not None:
        with open(output, "w") as f:
            json.dump(result, f, indent=1)
    return result

"""`python -m musicgan_amd <mode> ...`: the reference's four sub-commands with its positional names and flags
(/root/reference/music_gan/__main__.py:11-124) and `evaluate`, `loudness`, `separate`, `project`, `evaluate_mel`, `evaluate_audio` and `path_length`, which the reference does not have, declared as data and dispatched
lazily (importing `train` pulls in the GPU library, `view_audio` pulls in matplotlib)."""
import argparse
import importlib
import re
from fractions import Fraction

_METRICS = ("swd", "msssim", "nn")
_METRICS_ALL = _METRICS + ("prdc",)
_METRICS_EVERY = _METRICS_ALL + ("ndb",)
_MEL_METRICS = ("fd", "nn", "prdc", "ndb")   # evaluate_mel.METRICS
_MEL_METRICS_ALL = _MEL_METRICS + ("kid",)   # evaluate_mel.METRICS_ALL
_AUGMENTS = ("translation", "cutout")   # aug_ops.OPS (not imported here: the modes are dispatched lazily)


def _metric_list(text: str):
    names = tuple(t.strip() for t in text.split(","))
    if any(n not in _METRICS_EVERY for n in names) or len(set(names)) != len(names):
        raise argparse.ArgumentTypeError(f"a comma-separated subset of {','.join(_METRICS_EVERY)} expected, got {text!r}")
    return names


def _mel_metric_list(text: str):
    names = tuple(t.strip() for t in text.split(","))
    if any(n not in _MEL_METRICS_ALL for n in names) or len(set(names)) != len(names):
        raise argparse.ArgumentTypeError(f"a comma-separated subset of {','.join(_MEL_METRICS_ALL)} expected, got {text!r}")
    return names


def _fraction_list(text: str):
    """'9/10,1.1' -> (Fraction(9, 10), Fraction(11, 10)): a/b or decimals, taken exactly"""
    try:
        return tuple(Fraction(t.strip()) for t in text.split(","))
    except (ValueError, ZeroDivisionError):
        raise argparse.ArgumentTypeError(f"a comma-separated list of numbers (a/b or decimals) expected, got {text!r}")


def _augment_policy(text: str):
    """'translation,cutout' as given, once the names are known ones, each given once"""
    names = tuple(t.strip() for t in text.split(","))
    if any(n not in _AUGMENTS for n in names) or len(set(names)) != len(names):
        raise argparse.ArgumentTypeError(f"a comma-separated subset of {','.join(_AUGMENTS)} expected, got {text!r}")
    return ",".join(names)


def _probability(text: str):
    try:
        p = float(text)
    except ValueError:
        p = -1.0
    if not 0.0 <= p <= 1.0:
        raise argparse.ArgumentTypeError(f"a probability in [0, 1] expected, got {text!r}")
    return p


def _step(text: str):
    try:
        eps = float(text)
    except ValueError:
        eps = 0.0
    if not 0.0 < eps <= 0.1:
        raise argparse.ArgumentTypeError(f"a step in (0, 0.1] expected, got {text!r}")
    return eps


# mode -> (module, function, [(flags, kwargs)], lambda args: positional call arguments[, lambda args: keyword call arguments])
_MODES = {
    "create_dataset": ("create_dataset", "create_dataset", [
        (("audio_path",), dict(type=str, help="can be /path/to/*.wav")),
        (("-o", "--output-dir"), dict(type=str, required=True, help="The folder where the tensor files will be saved")),
        (("--resample",), dict(action="store_true", help="resample files that are not at 44.1 kHz (else they are refused)")),
        (("--stretch",), dict(type=_fraction_list, default=(), metavar="9/10,1.1",
                              help="also write every file re-timed by these rates (a/b or decimals in [1/8, 8], above 1: faster) "
                                   "at its own pitch: GPU phase vocoder")),
        (("--pitch",), dict(type=_fraction_list, default=(), metavar="-1,1",
                            help="also write every file transposed by these numbers of semitones at its own duration")),
        (("--preserve-transients",), dict(dest="preserve_transients", action="store_true",
                                          help="with --stretch / --pitch: re-time only the harmonic part of every variant with the "
                                               "phase vocoder and overlap-add its percussive part, so that drum hits stay sharp")),
        (("--phase-lock",), dict(dest="phase_lock", action="store_true",
                                 help="with --stretch / --pitch: identity phase locking in the phase vocoder, so that the bins of "
                                      "one partial keep their phase differences and moving pitches do not warble")),
        (("--component",), dict(choices=("harmonic", "percussive"), default=None,
                                help="code only this component of every spectrum (median-filtering harmonic / percussive "
                                     "separation), the original's and each variant's")),
    ], lambda a: (a.audio_path, a.output_dir),
        lambda a: {**({"resample": True} if a.resample else {}), **({"stretch": a.stretch} if a.stretch else {}),
                   **({"pitch": a.pitch} if a.pitch else {}),
                   **({"preserve_transients": True} if a.preserve_transients else {}),
                   **({"phase_lock": True} if a.phase_lock else {}),
                   **({"component": a.component} if a.component is not None else {})}),
    "train": ("train", "train", [
        (("run",), dict(type=str, metavar="RUN_NAME")),
        (("-o", "--out-path"), dict(dest="out_path", type=str, required=True)),
        (("-i", "--input-dataset"), dict(dest="input_dataset", type=str, required=True)),
        (("--ema-decay",), dict(dest="ema_decay", type=float, default=0.0, metavar="D",
                                help="also keep an exponential running average of the generator's weights, decay D per generator "
                                     "update (one in five iterations; Karras et al. use 0.999), saved as gen_ema_K.pt; 0: off")),
        (("--resident",), dict(action="store_true",
                               help="upload the dataset's side-car to device memory once and gather every batch there (no per-batch "
                                    "host copy); refused when it would take more than three quarters of the free memory")),
        (("--random-offset",), dict(dest="random_offset", action="store_true",
                                    help="train on 512-frame windows at a random time offset into two consecutive chunks of a track, "
                                         "redrawn every epoch (needs a dataset written by create_dataset in one process)")),
        (("--augment",), dict(type=_augment_policy, default=None, metavar="translation,cutout",
                              help="DiffAugment: shift (up to 1/8 of each side, zero fill) and / or cut a half-size box out of every "
                                   "image the critic sees, real and generated; the generator's gradient flows back through it")),
        (("--augment-p",), dict(dest="augment_p", type=_probability, default=None, metavar="P",
                                help="probability with which each transform of --augment is applied to a sample (default 1)")),
    ], lambda a: (a.run, a.input_dataset, a.out_path),
        lambda a: {**({"ema_decay": a.ema_decay} if a.ema_decay else {}), **({"resident": True} if a.resident else {}),
                   **({"random_offset": True} if a.random_offset else {}), **({"augment": a.augment} if a.augment else {}),
                   **({"augment_p": a.augment_p} if a.augment_p is not None else {})}),
    "generate": ("generate", "generate", [
        (("gen_dict_state",), dict(type=str)),
        (("rand_channels",), dict(type=int)),
        (("-n", "--nb-vec"), dict(type=int, default=10)),
        (("-m", "--nb-music"), dict(type=int, default=5)),
        (("-o", "--output-dir"), dict(type=str, required=True)),
        (("--format",), dict(dest="audio_format", choices=("wav", "flac", "ogg"), default="wav",
                             help="wav: 32-bit float (default); flac: 24-bit FLAC; ogg: Ogg Vorbis at quality 3 (both "
                                  "encoded on the GPU)")),
        (("--griffin-lim",), dict(dest="griffin_lim", type=int, default=0, metavar="N",
                                  help="N rounds of Griffin-Lim phase refinement before the file is written (default 0: none)")),
        (("--loudness",), dict(type=float, default=None, metavar="LUFS",
                               help="bring every file to this integrated loudness (ITU-R BS.1770-4), e.g. -14 (default: the level "
                                    "the codec gives)")),
        (("--true-peak",), dict(dest="true_peak", type=float, default=None, metavar="DBTP",
                                help="true-peak ceiling of --loudness in dBTP (default -1)")),
        (("--limiter",), dict(action="store_true",
                              help="with --loudness: hold the peaks under the ceiling with a look-ahead true-peak limiter, so that "
                                   "a file with a high crest factor reaches the target too (default: one gain, lowered until the "
                                   "peak fits)")),
        (("--limiter-attack",), dict(dest="limiter_attack", type=float, default=None, metavar="MS",
                                     help="look-ahead of --limiter in ms (default 5)")),
        (("--limiter-release",), dict(dest="limiter_release", type=float, default=None, metavar="MS",
                                      help="release time of --limiter in ms (default 50)")),
        (("--seed",), dict(type=int, default=None, help="draw the latents from a generator seeded with this (default: unseeded)")),
        (("--latents",), dict(type=str, default=None, metavar="LATENTS.pt",
                              help="a latents.pt written by `project`: its windows, joined along time, are the one latent and "
                                   "sound_0 the one file (-n and -m are not used)")),
        (("--morph-to",), dict(dest="morph_to", type=str, default=None, metavar="LATENTS.pt",
                               help="with --latents: a second latents.pt with as many windows; -m files on the arc from the first "
                                    "to the second (spherical interpolation, window by window), ends included")),
    ], lambda a: (a.output_dir, a.rand_channels, a.gen_dict_state, a.nb_vec, a.nb_music),
        lambda a: {**({"audio_format": a.audio_format} if a.audio_format != "wav" else {}),
                   **({"griffin_lim": a.griffin_lim} if a.griffin_lim else {}),
                   **({"loudness": a.loudness} if a.loudness is not None else {}),
                   **({"peak_dbtp": a.true_peak} if a.true_peak is not None else {}),
                   **({"limiter": True} if a.limiter else {}),
                   **({"limiter_attack": a.limiter_attack} if a.limiter_attack is not None else {}),
                   **({"limiter_release": a.limiter_release} if a.limiter_release is not None else {}),
                   **({"seed": a.seed} if a.seed is not None else {}),
                   **({"latents": a.latents} if a.latents is not None else {}),
                   **({"morph_to": a.morph_to} if a.morph_to is not None else {})}),
    "view_audio": ("view_audio", "view_audio", [
        (("--input-audio",), dict(type=str, required=True)),
        (("--image-idx",), dict(type=int, required=True)),
    ], lambda a: (a.input_audio, a.image_idx)),
    "evaluate": ("evaluate", "evaluate", [
        (("gen_dict_state",), dict(type=str)),
        (("rand_channels",), dict(type=int)),
        (("-i", "--input-dataset"), dict(dest="input_dataset", type=str, required=True)),
        (("--level",), dict(type=int, default=7, help="growth level of the checkpoint (7: fully grown, 512 x 512)")),
        (("-n", "--nb-images"), dict(dest="nb_images", type=int, default=8192, help="images per set (clipped to the dataset)")),
        (("--batch-size",), dict(dest="batch_size", type=int, default=16)),
        (("--seed",), dict(type=int, default=0)),
        (("-o", "--output"), dict(type=str, default=None, help="also write the result as JSON to this file")),
        (("--metrics",), dict(type=_metric_list, default=None, metavar="swd,msssim,nn,prdc,ndb",
                              help="what to report (default: swd); msssim: MS-SSIM between random pairs of generated images "
                                   "and of real ones -- a generated value well above the real one means mode collapse; nn: RMS "
                                   "distance to the nearest dataset image, of generated images and of real ones -- a generated "
                                   "value well below the real one, or a smallest value near 0, means memorised samples; prdc: "
                                   "k-nearest-neighbour precision / recall / density / coverage of all generated against all real "
                                   "images -- low precision means samples off the data manifold, low recall or coverage means "
                                   "missing modes; compare with the _real figures; ndb: the share of k-means bins of the real "
                                   "images whose share of the generated images is statistically different, and the Jensen-Shannon "
                                   "divergence of the two bin histograms -- ndb well above ndb_real means modes missing or "
                                   "over-produced")),
    ], lambda a: (a.gen_dict_state, a.rand_channels, a.input_dataset),
        lambda a: dict(level=a.level, nb_images=a.nb_images, batch_size=a.batch_size, seed=a.seed, output=a.output,
                       **({"metrics": a.metrics} if a.metrics is not None else {}))),
}
# sub-commands that work on audio files, not on a model (same declaration; kept apart from the five modes above)
_FILE_MODES = {
    "loudness": ("loudness", "loudness", [
        (("audio_path",), dict(type=str, help="can be /path/to/*.wav (any format that can be read: wav, aiff, au, flac, ogg)")),
        (("-o", "--output"), dict(type=str, default=None, help="also write the measurements as JSON to this file")),
    ], lambda a: (a.audio_path,), lambda a: {"output": a.output} if a.output is not None else {}),
    "separate": ("separate", "separate", [
        (("audio_path",), dict(type=str, metavar="AUDIO", help="one recording (any format that can be read: wav, aiff, au, flac, ogg)")),
        (("-o", "--output-dir"), dict(type=str, required=True, help="receives harmonic.* and percussive.*")),
        (("--format",), dict(dest="audio_format", choices=("wav", "flac", "ogg"), default="wav")),
        (("--kernel",), dict(type=int, default=31, metavar="L",
                             help="length of both median filters, odd, 3 .. 63 (default 31: 0.18 s of frames, 1.3 kHz of bins)")),
        (("--margin",), dict(type=float, default=1.0, metavar="M",
                             help="how much larger a component's estimate must be to claim a bin (default 1: the two files sum "
                                  "to the input; above 1 a residual is left out of both)")),
        (("--resample",), dict(action="store_true", help="resample a file that is not at 44.1 kHz (else it is refused)")),
    ], lambda a: (a.audio_path, a.output_dir),
        lambda a: {**({"audio_format": a.audio_format} if a.audio_format != "wav" else {}),
                   **({"kernel_size": a.kernel} if a.kernel != 31 else {}), **({"margin": a.margin} if a.margin != 1.0 else {}),
                   **({"resample": True} if a.resample else {})}),
}
# sub-commands that work on latents (same declaration; kept apart as well)
_LATENT_MODES = {
    "project": ("project", "project", [
        (("gen_dict_state",), dict(type=str)),
        (("rand_channels",), dict(type=int)),
        (("audio_path",), dict(type=str, help="the recording to project (any format that can be read: wav, aiff, au, flac, ogg)")),
        (("-o", "--output-dir"), dict(type=str, required=True, help="receives latents.pt, projection.json and, at level 7, "
                                                                    "reconstruction.* and target.*")),
        (("--level",), dict(type=int, default=7, help="growth level of the checkpoint (7: fully grown, 512 x 512)")),
        (("--steps",), dict(type=int, default=1000, help="Adam steps per window (default 1000, the StyleGAN2 projector's)")),
        (("--lr",), dict(type=float, default=0.1, help="peak learning rate: linear ramp over the first 5 %% of the steps, cosine "
                                                       "decay over the last 25 %%")),
        (("--candidates",), dict(type=int, default=16, help="seeded random latents per window of which the closest is the start")),
        (("--batch-size",), dict(dest="batch_size", type=int, default=6, help="windows optimised together")),
        (("--seed",), dict(type=int, default=0)),
        (("--format",), dict(dest="audio_format", choices=("wav", "flac", "ogg"), default="wav")),
        (("--griffin-lim",), dict(dest="griffin_lim", type=int, default=0, metavar="N",
                                  help="N rounds of Griffin-Lim phase refinement before the two audio files are written")),
        (("--resample",), dict(action="store_true", help="resample a file that is not at 44.1 kHz (else it is refused)")),
    ], lambda a: (a.gen_dict_state, a.rand_channels, a.audio_path, a.output_dir),
        lambda a: dict(level=a.level, steps=a.steps, lr=a.lr, candidates=a.candidates, batch_size=a.batch_size, seed=a.seed,
                       **({"audio_format": a.audio_format} if a.audio_format != "wav" else {}),
                       **({"griffin_lim": a.griffin_lim} if a.griffin_lim else {}),
                       **({"resample": True} if a.resample else {}))),
}
# sub-commands that compare two sets of audio files, with no model involved (same declaration; kept apart as well)
_FILE_SET_MODES = {
    "evaluate_audio": ("evaluate_audio", "evaluate_audio", [
        (("real_path",), dict(type=str, metavar="REAL_GLOB", help="the reference set, can be \"real/*.flac\" (any format that can be "
                                                                  "read: wav, aiff, au, flac, ogg)")),
        (("fake_path",), dict(type=str, metavar="OTHER_GLOB", help="the set to be judged, can be \"gen/*.wav\"")),
        (("-n", "--nb-windows"), dict(dest="nb_windows", type=int, default=8192,
                                      help="windows of 512 frames (2.97 s) per set (clipped to what the files hold)")),
        (("--seed",), dict(type=int, default=0)),
        (("--resample",), dict(action="store_true", help="resample files that are not at 44.1 kHz (else they are left out)")),
        (("-o", "--output"), dict(type=str, default=None, help="also write the result as JSON to this file")),
        (("--metrics",), dict(type=_mel_metric_list, default=None, metavar="fd,nn,prdc,ndb,kid",
                              help="evaluate_mel's metrics and keys between the windows of the two sets of files, in the log-mel "
                                   "spectrogram of the waveforms (default: fd); the _real figures compare two halves of REAL_GLOB")),
    ], lambda a: (a.real_path, a.fake_path),
        lambda a: dict(nb_windows=a.nb_windows, seed=a.seed, output=a.output,
                       **({"metrics": a.metrics} if a.metrics is not None else {}),
                       **({"resample": True} if a.resample else {}))),
}
# sub-commands that evaluate a checkpoint in a feature space other than pixels (same declaration; kept apart as well)
_FEATURE_MODES = {
    "evaluate_mel": ("evaluate_mel", "evaluate_mel", [
        (("gen_dict_state",), dict(type=str)),
        (("rand_channels",), dict(type=int)),
        (("-i", "--input-dataset"), dict(dest="input_dataset", type=str, required=True)),
        (("--level",), dict(type=int, default=7, help="growth level of the checkpoint, 4 .. 7 (7: fully grown, 512 x 512)")),
        (("-n", "--nb-images"), dict(dest="nb_images", type=int, default=8192, help="images per set (clipped to the dataset)")),
        (("--batch-size",), dict(dest="batch_size", type=int, default=16)),
        (("--seed",), dict(type=int, default=0)),
        (("-o", "--output"), dict(type=str, default=None, help="also write the result as JSON to this file")),
        (("--metrics",), dict(type=_mel_metric_list, default=None, metavar="fd,nn,prdc,ndb,kid",
                              help="what to report in the log-mel spectrogram of what the images decode to (default: fd); fd: the "
                                   "Frechet distance between the Gaussians fitted to the generated and to the real rows, with "
                                   "fd_half and fd_real at equal set sizes -- fd_half near fd_real is what a perfect generator "
                                   "scores; nn, prdc, ndb: as in evaluate, on log-mel rows instead of pixels; kid: the Kernel "
                                   "Inception Distance on the rows of fd (mean and deviation over 100 subsets of 1000, kid_full on "
                                   "all images, kid_real for two halves of the data): unbiased, so comparable across set sizes")),
        (("--waveform",), dict(action="store_true",
                               help="take every row from the waveform its image decodes to instead of from the magnitude channel, "
                                    "so that the phase channel counts (level 7 only); the lines say \"in waveform log-mel space\"")),
        (("--griffin-lim",), dict(dest="griffin_lim", type=int, default=0, metavar="N",
                                  help="with --waveform: N rounds of Griffin-Lim phase refinement on every generated image before "
                                       "it is scored, as generate --griffin-lim N writes it (default 0: none)")),
    ], lambda a: (a.gen_dict_state, a.rand_channels, a.input_dataset),
        lambda a: dict(level=a.level, nb_images=a.nb_images, batch_size=a.batch_size, seed=a.seed, output=a.output,
                       **({"metrics": a.metrics} if a.metrics is not None else {}),
                       **({"griffin_lim": a.griffin_lim} if a.griffin_lim else {}))),
}

# sub-commands that measure a checkpoint's latent space, with no dataset involved (same declaration; kept apart as well)
_PATH_MODES = {
    "path_length": ("path_length", "path_length", [
        (("gen_dict_state",), dict(type=str)),
        (("rand_channels",), dict(type=int)),
        (("--level",), dict(type=int, default=7, help="growth level of the checkpoint, 4 .. 7 (7: fully grown, 512 x 512)")),
        (("-n", "--nb-pairs"), dict(dest="nb_pairs", type=int, default=8192, help="pairs of latents (four images each)")),
        (("--epsilon",), dict(type=_step, default=1e-4, help="the step along the arc between two latents, in (0, 0.1]")),
        (("--sampling",), dict(choices=("full", "end"), default="full",
                               help="full: the step starts at a random position of the arc; end: at its first latent")),
        (("--seed",), dict(type=int, default=0)),
        (("--waveform",), dict(action="store_true",
                               help="take every row from the waveform its image decodes to instead of from the magnitude channel, "
                                    "so that the phase channel counts (level 7 only)")),
        (("--griffin-lim",), dict(dest="griffin_lim", type=int, default=0, metavar="N",
                                  help="with --waveform: N rounds of Griffin-Lim phase refinement on every image before it is scored")),
        (("-o", "--output"), dict(type=str, default=None, help="also write the result as JSON to this file")),
    ], lambda a: (a.gen_dict_state, a.rand_channels),
        lambda a: dict(level=a.level, nb_pairs=a.nb_pairs, epsilon=a.epsilon, sampling=a.sampling, seed=a.seed, output=a.output,
                       **({"waveform": True} if a.waveform else {}),
                       **({"griffin_lim": a.griffin_lim} if a.griffin_lim else {}))),
}


def _all_modes() -> dict:
    return {**_MODES, **_FILE_MODES, **_LATENT_MODES, **_FILE_SET_MODES, **_PATH_MODES, **_FEATURE_MODES}


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser("MusicGAN")
    modes = parser.add_subparsers(dest="mode")
    modes.required = True
    for mode, (_, _, arguments, *_) in _all_modes().items():
        sub = modes.add_parser(mode)
        for flags, kwargs in arguments:
            sub.add_argument(*flags, **kwargs)
        # argparse takes "-1" for a value and "-1,1" for an unknown flag: lists of numbers are values too (`--pitch -1,1`)
        sub._negative_number_matcher = re.compile(r"^-\d[\d.,/-]*$|^-\.\d[\d.,/-]*$")
    return parser


def main(argv=None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.mode in ("evaluate_mel", "path_length") and args.griffin_lim and not args.waveform:
        parser.error("--griffin-lim needs --waveform")
    if args.mode == "generate" and args.loudness is None and (
            args.limiter or args.limiter_attack is not None or args.limiter_release is not None):
        parser.error("--limiter, --limiter-attack and --limiter-release need --loudness")
    module, function, _, call_args, *call_kwargs = _all_modes()[args.mode]
    if args.mode == "evaluate_mel" and args.waveform:
        function = "evaluate_mel_waveform"   # the same arguments, rows from the decoded waveforms (and griffin_lim)
    kwargs = call_kwargs[0](args) if call_kwargs else {}
    getattr(importlib.import_module(f".{module}", __package__), function)(*call_args(args), **kwargs)


if __name__ == "__main__":
    main()

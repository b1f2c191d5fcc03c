"""musicgan_amd -- the Ipsedo/MusicGAN training hot path on AMD MI355X (gfx950): ProGAN WGAN-GP generator/discriminator step
and the STFT / magnitude-phase codec, hand-written HIP behind a C ABI (include/musicgan_hip.h), with the reference's Python
surface (`networks`, `audio`, `train`, `generate`, `create_dataset`, `view_audio`) on top, plus `evaluate` / `metrics`
(sliced Wasserstein distance of a checkpoint's samples to the data) and `evaluate_mel` (Frechet distance, Kernel Inception Distance and kNN
metrics of log-mel spectrograms, of the images, or in `evaluate_mel_waveform` of the sound they decode to) and `evaluate_audio` (the same
metrics between two sets of audio files) and `path_length` (the perceptual path length of a checkpoint's latent space in those rows), which
the reference does not have."""


def __getattr__(name):  # lazy: importing the package must not drag in the data/IO stack
    if name in ("train", "generate", "create_dataset", "view_audio", "evaluate", "evaluate_mel", "evaluate_audio", "path_length"):
        import importlib
        fn = getattr(importlib.import_module(f".{name}", __name__), name)
        globals()[name] = fn  # the import system bound the sub-module under this name; re-bind the function like the reference
        return fn
    if name == "evaluate_mel_waveform":
        import importlib
        module = importlib.import_module(".evaluate_mel", __name__)
        globals()["evaluate_mel"] = module.evaluate_mel  # (the import bound the sub-module under that name)
        return module.evaluate_mel_waveform
    if name in ("networks", "audio", "ops", "optim", "dist", "utils", "train_step", "metrics"):
        import importlib
        return importlib.import_module(f".{name}", __name__)
    raise AttributeError(name)

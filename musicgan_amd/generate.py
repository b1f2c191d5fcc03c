"""Sampling driver with the reference's entry point `generate(output_dir, rand_channels, gen_dict_state, nb_vec, nb_music)`
(/root/reference/music_gan/generate.py:12-65): a fully grown generator turns wide latents into (2, 512, 512 * nb_vec)
magnitude / phase images, which the inverse codec + inverse STFT turn into `sound_{i}.wav` (`.flac` with audio_format="flac",
`.ogg` with "ogg") -- all of it on the GPU."""
import os

import torch

from . import audio
from .networks import Generator

_LATENT_H, _LATENT_W = 2, 2   # latent tile that grows to one 512 x 512 image; nb_vec tiles side by side along time
_FINAL_LEVEL = 7


def _load_generator(rand_channels: int, checkpoint: str, device: torch.device) -> Generator:
    net = Generator(rand_channels, end_layer=_FINAL_LEVEL)
    net.load_state_dict(torch.load(checkpoint, map_location="cpu"))
    return net.to(device).eval()


def _given_latents(latents, morph_to, rand_channels: int, nb_music: int):
    """The wide latents of `latents` / `morph_to` (files written by `project`), on the CPU: one (1, C, 2, 2 N) tensor, or nb_music of
    them on the arc from A to B, window by window.  None when neither is given.  Touches no device."""
    if latents is None:
        if morph_to is not None:
            raise ValueError("morph_to needs latents: the file to start from")
        return None
    from . import project
    a = project.load_latents(latents, rand_channels, _FINAL_LEVEL)
    if morph_to is None:
        return [project.wide_latent(a)]
    b = project.load_latents(morph_to, rand_channels, _FINAL_LEVEL)
    if a.shape != b.shape:
        raise ValueError(f"\"{latents}\" holds {a.shape[0]} windows and \"{morph_to}\" {b.shape[0]}: a morph needs as many in both")
    if nb_music < 2:
        raise ValueError(f"a morph writes its two ends: nb_music must be at least 2, got {nb_music}")
    return [project.wide_latent(torch.stack([project.slerp(wa, wb, i / (nb_music - 1)) for wa, wb in zip(a, b)]))
            for i in range(nb_music)]


def generate(output_dir: str, rand_channels: int, gen_dict_state: str, nb_vec: int, nb_music: int,
             audio_format: str = "wav", griffin_lim: int = 0, loudness=None, peak_dbtp: float = -1.0,
             latents=None, morph_to=None, seed=None, limiter: bool = False, limiter_attack: float = 5.0,
             limiter_release: float = 50.0) -> None:
    """audio_format: "wav" (32-bit float, the reference's output), "flac" (24-bit) or "ogg" (Ogg Vorbis at the default quality),
    the last two encoded on the GPU; griffin_lim: rounds of Griffin-Lim phase refinement before the file is written (0: none);
    loudness: bring every file to this integrated loudness in LUFS (ITU-R BS.1770-4) under the true-peak ceiling peak_dbtp in dBTP
    (None: the level the codec gives); limiter: with `loudness`, hold the peaks under the ceiling with the look-ahead true-peak limiter
    (limiter_attack, limiter_release in ms: audio.limit) instead of delivering a file below the target when the ceiling binds; seed: the latents come from a device generator seeded with it (None: the global generator's
    next draw, as ever); latents: a `latents.pt` written by `project` -- its N windows, side by side along time, are the one latent
    and `sound_0` the one file (nb_vec and nb_music are not used); morph_to: a second such file with as many windows -- nb_music
    files, file i at t = i / (nb_music - 1) of the arc from the first file's latents to the second's, window by window
    (project.slerp)"""
    given = _given_latents(latents, morph_to, rand_channels, nb_music)
    if loudness is not None:
        from . import loud_ops
        loud_ops.check_targets(loudness, peak_dbtp)
    if limiter:
        from . import lim_ops
        if loudness is None:
            raise ValueError("limiter needs loudness: it holds the peaks that the gain to a loudness target pushes past the ceiling")
        lim_ops.check_arguments(audio.SAMPLE_RATE, peak_dbtp, limiter_attack, limiter_release)
    if isinstance(griffin_lim, bool) or not isinstance(griffin_lim, int) or griffin_lim < 0:
        raise ValueError(f"griffin_lim must be a non-negative integer, got {griffin_lim!r}")
    if audio_format not in ("wav", "flac", "ogg"):
        raise ValueError(f"audio_format must be 'ogg', 'wav' or 'flac', got {audio_format!r}")
    if os.path.exists(output_dir) and not os.path.isdir(output_dir):
        raise NotADirectoryError(f"\"{output_dir}\" is not a directory")
    os.makedirs(output_dir, exist_ok=True)

    device = torch.device("cuda", torch.cuda.current_device())
    print("Load model...")
    gen = _load_generator(rand_channels, gen_dict_state, device)

    print("Pass rand data to generator...")
    if given is not None:
        items = [z.to(device) for z in given]
    elif seed is not None:
        rng = torch.Generator(device=device).manual_seed(int(seed))
        items = torch.randn(nb_music, rand_channels, _LATENT_H, _LATENT_W * nb_vec, device=device, generator=rng).split(1, dim=0)
    else:
        items = torch.randn(nb_music, rand_channels, _LATENT_H, _LATENT_W * nb_vec, device=device).split(1, dim=0)
    print("Saving sound...")
    with torch.no_grad():
        # one item at a time: the level-7 activations of a 512 x (512 * nb_vec) image are ~1 GB each
        for idx, z in enumerate(items):
            image = gen(z.contiguous(), 1.0)
            audio.magn_phase_to_wav(image, os.path.join(output_dir, f"sound_{idx}.{audio_format}"), audio.SAMPLE_RATE,
                                    **({"griffin_lim": griffin_lim} if griffin_lim else {}),
                                    **({"loudness": loudness, "peak_dbtp": peak_dbtp} if loudness is not None else {}),
                                    **({"limiter": True, "attack_ms": limiter_attack, "release_ms": limiter_release}
                                       if limiter else {}))

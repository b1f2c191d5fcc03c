"""Latent projection: `project(gen_dict_state, rand_channels, audio_path, output_dir)` finds, for every 512-frame window of a
recording, the latent whose image is closest to the window's under the multi-scale L2 loss -- the projector every
published ProGAN / StyleGAN code base ships next to its metrics, which the reference does not have.  The generator's weights stay
frozen: a step is a forward pass that saves, the loss launch, the data-only backward pass down to the latent
(engine.DataOnlySink) and one FusedAdam launch on the latent; nothing is read back inside the loop.  `slerp` and `load_latents` are
what `generate --latents / --morph-to` builds on; both are plain torch and touch no device."""
from __future__ import annotations

import json
import math
import os
from typing import Optional, Sequence

import torch

_FINAL_LEVEL, _FULL_SIDE = 7, 512
_LATENT_H, _LATENT_W = 2, 2
# the StyleGAN2 projector's schedule: linear ramp over the first 5 % of the steps, cosine decay over the last 25 %
_RAMP_UP, _RAMP_DOWN = 0.05, 0.25
_SLERP_MIN_ANGLE = 1e-6


def lr_at(step: int, steps: int, lr: float) -> float:
    """the learning rate of step 0 .. steps - 1 (Karras et al., projector.py of StyleGAN2: step 0 runs at 0)"""
    t = step / steps
    ramp = min(1.0, (1.0 - t) / _RAMP_DOWN)
    ramp = 0.5 - 0.5 * math.cos(ramp * math.pi)
    return lr * ramp * min(1.0, t / _RAMP_UP)


def slerp(a: torch.Tensor, b: torch.Tensor, t: float) -> torch.Tensor:
    """Spherical interpolation between two tensors of one shape, each taken as one flat vector: computed in float64, rounded once to
    float32.  a at t = 0 and b at t = 1, exactly; for inputs of equal norm every point has that norm.  An angle below 1e-6 (equal or
    nearly parallel inputs, or a zero vector) falls back to the straight line (1 - t) a + t b; antipodal inputs (angle within 1e-6 of
    pi), between which every great circle is a shortest path, raise ValueError."""
    if a.shape != b.shape:
        raise ValueError(f"slerp: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    a64, b64, t = a.to(torch.float64), b.to(torch.float64), float(t)
    na, nb = float(a64.norm()), float(b64.norm())
    omega = 0.0
    if na > 0.0 and nb > 0.0:
        omega = math.acos(max(-1.0, min(1.0, float((a64 * b64).sum()) / (na * nb))))
    if math.pi - omega < _SLERP_MIN_ANGLE:
        raise ValueError("slerp: the inputs are antipodal, no single shortest arc joins them")
    if omega < _SLERP_MIN_ANGLE:
        out = (1.0 - t) * a64 + t * b64
    else:
        s = math.sin(omega)
        out = (math.sin((1.0 - t) * omega) / s) * a64 + (math.sin(t * omega) / s) * b64
    return out.to(torch.float32)


def load_latents(path: str, rand_channels: int, level: int = _FINAL_LEVEL) -> torch.Tensor:
    """the (N, C, 2, 2) float32 latents of a `latents.pt` written by `project`, on the CPU; ValueError when the file is no such
    dict, or was projected with another `rand_channels` or at another level"""
    d = torch.load(path, map_location="cpu")
    if not isinstance(d, dict) or not all(k in d for k in ("latents", "rand_channels", "level")):
        raise ValueError(f"\"{path}\" is no latents file written by project")
    z = d["latents"]
    if int(d["rand_channels"]) != rand_channels or int(d["level"]) != level:
        raise ValueError(f"\"{path}\" was projected with rand_channels={d['rand_channels']} at level {d['level']}, "
                         f"not rand_channels={rand_channels} at level {level}")
    if not isinstance(z, torch.Tensor) or z.dim() != 4 or z.shape[0] < 1 or tuple(z.shape[1:]) != (rand_channels, _LATENT_H, _LATENT_W):
        raise ValueError(f"\"{path}\": latents of shape (N, {rand_channels}, {_LATENT_H}, {_LATENT_W}) expected")
    return z.to(torch.float32).contiguous()


def wide_latent(z: torch.Tensor) -> torch.Tensor:
    """(N, C, 2, 2) -> (1, C, 2, 2 N): the windows side by side along time, as `generate` lays out its random tiles"""
    return torch.cat(list(z), dim=-1)[None].contiguous()


def window_seed(seed: int, window: int) -> int:
    """the seed of the generator that draws window `window`'s candidates"""
    return (int(seed) * 1000003 + int(window)) % (1 << 63)


def draw_candidates(seed: int, window: int, candidates: int, rand_channels: int, device) -> torch.Tensor:
    rng = torch.Generator(device=device).manual_seed(window_seed(seed, window))
    return torch.randn(candidates, rand_channels, _LATENT_H, _LATENT_W, device=device, generator=rng)


def _check_counts(steps, candidates, batch_size, lr):
    for name, v in (("steps", steps), ("candidates", candidates), ("batch_size", batch_size)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    if not (isinstance(lr, (int, float)) and math.isfinite(lr) and lr >= 0):
        raise ValueError(f"lr must be a finite number >= 0, got {lr!r}")


def project_images(gen, targets: torch.Tensor, *, steps: int = 1000, lr: float = 0.1, candidates: int = 16, batch_size: int = 6,
                   seed: int = 0, levels: Optional[int] = None, weights: Optional[Sequence[float]] = None,
                   schedule: bool = True) -> dict:
    """The projector on target images (N, 2, side, side) float32 on the generator's device, as the critic would see them.  Returns
    CPU tensors: `latents` (N, C, 2, 2) float32, `loss_start` / `loss` (N,) float64 (at step 0 and after the last step), `rms` (N,)
    float64 (square root of the plain MSE after the last step) and `history` (steps, N) float64, read back once at the end.
    `schedule=False` keeps `lr` constant."""
    from . import proj_ops
    from .networks import engine
    from .optim import FusedAdam
    _check_counts(steps, candidates, batch_size, lr)
    if targets.dim() != 4 or targets.shape[0] < 1:
        raise ValueError(f"targets: a non-empty (N, 2, side, side) batch expected, got {tuple(targets.shape)}")
    targets = targets.contiguous()
    n, _, h, w = targets.shape
    lam = proj_ops.check_weights(h, w, weights, levels)
    device = targets.device
    params = list(gen.parameters())
    was = [p.requires_grad for p in params]
    for p in params:
        p.requires_grad_(False)
    rc = params[0].shape[1]
    W, cache = gen._weights(), gen._pack_cache
    lanes = torch.arange(candidates, device=device)
    z_all = torch.empty(n, rc, _LATENT_H, _LATENT_W, device=device)
    history = torch.empty(steps, n, dtype=torch.float64, device=device)
    loss_end = torch.empty(n, dtype=torch.float64, device=device)
    mse_end = torch.empty(n, dtype=torch.float64, device=device)
    try:
        with torch.no_grad():
            # the start of every window: the best of `candidates` seeded draws, chosen on the device (ties: the smaller index)
            for wi in range(n):
                zc = draw_candidates(seed, wi, candidates, rc, device)
                lc = torch.empty(candidates, dtype=torch.float64, device=device)
                for lo in range(0, candidates, batch_size):
                    img, _ = engine.gen_forward(W, zc[lo:lo + batch_size], 1.0, cache, save=False)
                    tgt = targets[wi:wi + 1].expand(img.shape[0], -1, -1, -1).contiguous()
                    lc[lo:lo + batch_size] = proj_ops.pyramid_l2(img, tgt, lam, need_grad=False)[0]
                best = torch.where(lc == lc.min(), lanes, candidates).min().clamp(max=candidates - 1)
                z_all[wi:wi + 1] = zc.index_select(0, best.reshape(1))
            for lo in range(0, n, batch_size):
                hi = min(n, lo + batch_size)
                z = z_all[lo:hi].clone().requires_grad_(True)
                tgt = targets[lo:hi]
                opt = FusedAdam([z], lr=lr, betas=(0.9, 0.999))
                for k in range(steps):
                    if schedule:
                        opt.param_groups[0]["lr"] = lr_at(k, steps, lr)
                    img, ctx = engine.gen_forward(W, z, 1.0, cache, save=True)
                    loss, g = proj_ops.pyramid_l2(img, tgt, lam)
                    history[k, lo:hi] = loss
                    z.grad = engine.gen_backward(W, ctx, g, cache, engine.DataOnlySink(), need_gz=True)
                    opt.step()
                img, _ = engine.gen_forward(W, z, 1.0, cache, save=False)
                loss_end[lo:hi] = proj_ops.pyramid_l2(img, tgt, lam, need_grad=False)[0]
                mse_end[lo:hi] = proj_ops.pyramid_l2(img, tgt, (1.0,), need_grad=False)[0]
                z_all[lo:hi] = z.detach()
    finally:
        for p, r in zip(params, was):
            p.requires_grad_(r)
    hist = history.cpu()   # the one read-back
    return {"latents": z_all.cpu(), "loss_start": hist[0].clone(), "loss": loss_end.cpu(), "rms": mse_end.cpu().sqrt(), "history": hist}


def _targets_of_file(audio_path: str, side: int, resample: bool) -> torch.Tensor:
    """the file's windows as the critic would see them: (N, 2, side, side) float32 in [-1, 1]"""
    from . import audio, ops
    spectrum = audio.wav_to_stft(audio_path, resample=resample)
    if spectrum.size()[1] - 1 < audio.N_VEC:   # create_dataset's rule: no complete image
        raise ValueError(f"\"{audio_path}\" is shorter than one window of {audio.N_VEC} frames")
    both = audio.stft_to_stacked_phase_magn(spectrum, nb_vec=audio.N_VEC)
    return ops.input_transform(both.contiguous(), side)


def project(gen_dict_state: str, rand_channels: int, audio_path: str, output_dir: str, *, level: int = _FINAL_LEVEL, steps: int = 1000,
            lr: float = 0.1, candidates: int = 16, batch_size: int = 6, seed: int = 0, levels: Optional[int] = None,
            weights: Optional[Sequence[float]] = None, audio_format: str = "wav", griffin_lim: int = 0, resample: bool = False) -> dict:
    """Project every window of `audio_path` onto the generator checkpoint `gen_dict_state` (grown to `level`).  Writes `latents.pt`
    and `projection.json` into `output_dir`, and at level 7 `reconstruction.{fmt}` (from G(z)) and `target.{fmt}` (from the
    normalised targets by the same path: what the codec and the per-window min-max alone cost).  `steps`, `lr` and `candidates`
    default to the StyleGAN2 projector's habits; they were not measured here.  Returns what `latents.pt` holds."""
    from . import audio
    from .networks import Generator
    if not 0 <= level <= _FINAL_LEVEL:
        raise ValueError(f"level must be in 0 .. {_FINAL_LEVEL}, got {level}")
    _check_counts(steps, candidates, batch_size, lr)
    if isinstance(griffin_lim, bool) or not isinstance(griffin_lim, int) or griffin_lim < 0:
        raise ValueError(f"griffin_lim must be a non-negative integer, got {griffin_lim!r}")
    if audio_format not in ("wav", "flac", "ogg"):
        raise ValueError(f"audio_format must be 'ogg', 'wav' or 'flac', got {audio_format!r}")
    if os.path.exists(output_dir) and not os.path.isdir(output_dir):
        raise NotADirectoryError(f"\"{output_dir}\" is not a directory")
    side = _FULL_SIDE >> (_FINAL_LEVEL - level)
    from . import proj_ops
    proj_ops.check_weights(side, side, weights, levels)
    os.makedirs(output_dir, exist_ok=True)
    device = torch.device("cuda", torch.cuda.current_device())

    print("Load model...")
    gen = Generator(rand_channels, end_layer=level)
    gen.load_state_dict(torch.load(gen_dict_state, map_location="cpu"))
    gen = gen.to(device).eval()

    targets = _targets_of_file(audio_path, side, resample)
    n = targets.shape[0]
    print(f"Project {n} windows of {side} x {side}: best of {candidates} starts, {steps} steps each...")
    res = project_images(gen, targets, steps=steps, lr=lr, candidates=candidates, batch_size=batch_size, seed=seed, levels=levels,
                         weights=weights)
    out = {"latents": res["latents"], "loss": res["loss"], "loss_start": res["loss_start"], "rand_channels": int(rand_channels),
           "level": int(level), "steps": int(steps), "seed": int(seed), "source": os.path.basename(audio_path)}
    torch.save(out, os.path.join(output_dir, "latents.pt"))
    with open(os.path.join(output_dir, "projection.json"), "w") as fh:
        json.dump({"source": out["source"], "level": level, "steps": steps, "seed": seed,
                   "windows": [{"loss_start": float(a), "loss": float(b), "rms": float(c)}
                               for a, b, c in zip(res["loss_start"], res["loss"], res["rms"])]}, fh, indent=1)
    for i, (a, b, c) in enumerate(zip(res["loss_start"], res["loss"], res["rms"])):
        print(f"window {i:3d}: loss {float(a):.6f} -> {float(b):.6f}, rms {float(c):.6f}")
    if level != _FINAL_LEVEL:
        print(f"No audio written: a level-{level} generator makes {side} x {side} images, the codec needs {_FULL_SIDE} frequency rows")
        return out
    extra = {"griffin_lim": griffin_lim} if griffin_lim else {}
    with torch.no_grad():
        z = res["latents"].to(device)
        images = [gen(z[lo:lo + batch_size].contiguous(), 1.0) for lo in range(0, n, batch_size)]
        along_time = lambda x: torch.cat(list(x), dim=-1)[None].contiguous()   # (N, 2, 512, 512) -> (1, 2, 512, 512 N)
        audio.magn_phase_to_wav(along_time(torch.cat(images)), os.path.join(output_dir, f"reconstruction.{audio_format}"),
                                audio.SAMPLE_RATE, **extra)
        audio.magn_phase_to_wav(along_time(targets), os.path.join(output_dir, f"target.{audio_format}"), audio.SAMPLE_RATE, **extra)
    return out

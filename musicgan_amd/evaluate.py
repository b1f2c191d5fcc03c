"""Evaluation driver: how close are a checkpoint's samples to the data?  `evaluate(gen_dict_state, rand_channels, input_dataset)`
loads a generator saved by train() (`gen_{k}.pt`), draws as many samples from it as it reads from the dataset and reports the
sliced Wasserstein distance between the two sets per pyramid level (musicgan_amd/metrics.py) -- one number per scale, x 1000 as
in the paper, lower is better.  With "msssim" among `metrics` it also reports MS-SSIM between random pairs of generated images
next to the same number for pairs of real images: a generated value well above the real one means the generator repeats itself
(mode collapse), which SWD does not show.  Single GPU."""
import json
from typing import Dict, Optional, Sequence

import torch

from . import audio, ops
from .metrics import MSSSIM, SWD
from .networks import Generator

_FINAL_LEVEL, _FULL_SIDE = 7, 512
_LATENT_H, _LATENT_W = 2, 2
METRICS = ("swd", "msssim")


def evaluate(gen_dict_state: str, rand_channels: int, input_dataset: str, metrics: Sequence[str] = ("swd",), *,
             level: int = _FINAL_LEVEL, nb_images: int = 8192, batch_size: int = 16, seed: int = 0,
             output: Optional[str] = None) -> Dict[str, float]:
    """`level`: the growth level the checkpoint was saved at (7 = fully grown, 512 x 512); real samples are brought to that level's
    side by the training loop's own input transform.  `metrics`: a subset of ("swd", "msssim").  Returns {"<side>": swd, ...,
    "avg": swd, "msssim_real": .., "msssim_fake": ..} (the keys of the metrics asked for) and writes it as JSON to `output`."""
    if not 0 <= level <= _FINAL_LEVEL:
        raise ValueError(f"level must be in 0 .. {_FINAL_LEVEL}, got {level}")
    if nb_images < 1 or batch_size < 1:
        raise ValueError("nb_images and batch_size must be positive")
    metrics = tuple(metrics)
    if not metrics or any(m not in METRICS for m in metrics) or len(set(metrics)) != len(metrics):
        raise ValueError(f"metrics: a non-empty subset of {METRICS} expected, got {metrics}")
    side = _FULL_SIDE >> (_FINAL_LEVEL - level)
    device = torch.device("cuda", torch.cuda.current_device())

    print("Load model...")
    gen = Generator(rand_channels, end_layer=level)
    gen.load_state_dict(torch.load(gen_dict_state, map_location="cpu"))
    gen = gen.to(device).eval()

    dataset = audio.PackedAudioDataset(input_dataset) if audio.has_packed(input_dataset) else audio.AudioDataset(input_dataset)
    if nb_images > len(dataset):
        print(f"The dataset holds {len(dataset)} samples: evaluating on {len(dataset)} images instead of {nb_images}")
        nb_images = len(dataset)
    if "msssim" in metrics and nb_images < 2:
        raise ValueError(f"MS-SSIM needs at least 2 images to pair, got {nb_images}")

    print(f"Evaluate {nb_images} real and {nb_images} generated images of {side} x {side}...")
    rng = torch.Generator(device=device).manual_seed(seed)
    # every latent in one draw (a few MB): the samples do not depend on the batch size
    latents = torch.randn(nb_images, rand_channels, _LATENT_H, _LATENT_W, device=device, generator=rng)
    result = {}
    if "swd" in metrics:
        swd = SWD(side, side, channels=2, images=nb_images, seed=seed)
        with torch.no_grad():
            for lo in range(0, nb_images, batch_size):
                n = min(batch_size, nb_images - lo)
                real = torch.stack([dataset[i] for i in range(lo, lo + n)]).to(device)
                swd.feed_real(ops.input_transform(real.contiguous(), side))
                swd.feed_fake(gen(latents[lo:lo + n].contiguous(), 1.0).contiguous())
        result.update(swd.result())
        for name, value in result.items():
            print(f"SWD x 1e3 [{name:>3}] = {value:.4f}")
    if "msssim" in metrics:
        # random pairs, the same index pairs for both sets: consecutive dataset samples are adjacent chunks of one track, and
        # pairing neighbours would inflate the real number
        perm = torch.randperm(nb_images, generator=torch.Generator().manual_seed(seed)).tolist()
        half = nb_images // 2
        first, second = perm[:half], perm[half:2 * half]
        ms_real, ms_fake = (MSSSIM(side, side, channels=2, pairs=half) for _ in range(2))

        def real_images(idx):
            return ops.input_transform(torch.stack([dataset[i] for i in idx]).to(device).contiguous(), side)

        def fake_images(idx):
            return gen(latents[torch.tensor(idx, device=device)].contiguous(), 1.0).contiguous()

        with torch.no_grad():
            for lo in range(0, half, batch_size):
                ia, ib = first[lo:lo + batch_size], second[lo:lo + batch_size]
                ms_real.feed(real_images(ia), real_images(ib))
                ms_fake.feed(fake_images(ia), fake_images(ib))
        result["msssim_real"], result["msssim_fake"] = ms_real.result(), ms_fake.result()
        for name in ("msssim_real", "msssim_fake"):
            print(f"MS-SSIM [{name[7:]}] = {result[name]:.6f}")
    if output is not None:
        with open(output, "w") as f:
            json.dump(result, f, indent=1)
    return result

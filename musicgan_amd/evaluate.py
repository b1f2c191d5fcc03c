"""Evaluation driver: how close are a checkpoint's samples to the data?  `evaluate(gen_dict_state, rand_channels, input_dataset)`
loads a generator saved by train() (`gen_{k}.pt`), draws as many samples from it as it reads from the dataset and reports the
sliced Wasserstein distance between the two sets per pyramid level (musicgan_amd/metrics.py) -- one number per scale, x 1000 as
in the paper, lower is better.  With "msssim" among `metrics` it also reports MS-SSIM between random pairs of generated images
next to the same number for pairs of real images: a generated value well above the real one means the generator repeats itself
(mode collapse), which SWD does not show.  With "nn" it reports how far generated images are from their nearest dataset image,
next to the same number for real images against the rest of the dataset: a generator that replays its corpus scores perfectly on
the other two and near zero here.  With "prdc" it reports k-nearest-neighbour precision / recall / density / coverage of all
generated against all real images: which way a checkpoint is wrong -- off the data manifold, or on it but covering part of it.
With "ndb" it reports the share of k-means bins of the data whose share of the generated images is statistically different, and
the Jensen-Shannon divergence of the two bin histograms: how the probability mass of the samples is spread over the corpus, which
none of the others measures.
Single GPU."""
import json
from typing import Dict, Optional, Sequence

import torch

from . import audio, ops
from .metrics import MSSSIM, NDB, PRDC, SWD, KMeans, NearestNeighbours
from .networks import Generator

_FINAL_LEVEL, _FULL_SIDE = 7, 512
_LATENT_H, _LATENT_W = 2, 2
METRICS = ("swd", "msssim", "nn")
METRICS_ALL = METRICS + ("prdc",)
METRICS_EVERY = METRICS_ALL + ("ndb",)
# the nearest-neighbour check: queries per set, the side images are compared at (pixel L2 at 512 x 512 is dominated by sub-pixel
# shifts and would cost 16 x more than the rest of the evaluation), neighbours kept per query
_NN_QUERIES, _NN_SIDE, _NN_K = 256, 128, 1
_PRDC_K = 3   # neighbours that define a sample's ball (Kynkaanniemi et al. 2019; also the 3 of StyleGAN2's tables); the side is _NN_SIDE
# NDB: at most 50 bins (GANSynth's number at this set size), at least 20 reference images per bin where the set allows it, Lloyd
# iterations, and the fewest images that give two halves of two bins of two; the side is _NN_SIDE
_NDB_BINS, _NDB_PER_BIN, _NDB_ITERATIONS, _NDB_MIN_IMAGES = 50, 20, 25, 8


def _ndb_bins(half: int) -> int:
    return min(_NDB_BINS, max(2, half // _NDB_PER_BIN))


def evaluate(gen_dict_state: str, rand_channels: int, input_dataset: str, metrics: Sequence[str] = ("swd",), *,
             level: int = _FINAL_LEVEL, nb_images: int = 8192, batch_size: int = 16, seed: int = 0,
             output: Optional[str] = None) -> Dict[str, float]:
    """`level`: the growth level the checkpoint was saved at (7 = fully grown, 512 x 512); real samples are brought to that level's
    side by the training loop's own input transform.  `metrics`: a subset of ("swd", "msssim", "nn", "prdc", "ndb").  Returns {"<side>": swd, ...,
    "avg": swd, "msssim_real": .., "msssim_fake": .., "nn_fake": .., "nn_real": .., "nn_fake_min": .., "nn_real_min": .., "precision": ..,
    "recall": .., "density": .., "coverage": .., "precision_real": .., .., "coverage_real": ..} (the keys of the metrics asked for)
    and writes it as JSON to `output`.

    "nn": the first min(nb_images, 256) generated images and as many real ones (random dataset entries, each barred from matching
    itself) are compared with all `nb_images` real images at min(side, 128) pixels a side (larger images are reduced by 2 x 2
    means).  Every number is a per-component RMS difference sqrt(d / D) to the nearest dataset image: `nn_fake` / `nn_real` the
    mean over the queries, `nn_fake_min` / `nn_real_min` the smallest (one memorised sample does not move a mean).  `nn_fake`
    well below `nn_real`, or `nn_fake_min` near 0, means memorisation.  Consecutive dataset entries are adjacent chunks of one
    track, so a real image's nearest neighbour is often its own continuation and `nn_real` is small: that is the honest
    calibration -- it is the distance at which the data resembles itself.

    "prdc": all `nb_images` generated images against all `nb_images` real ones, reduced as for "nn", with balls reaching to the
    3rd nearest other member of the own set (metrics.PRDC).  Appends `precision` (share of generated images inside some real
    image's ball: low = samples off the data manifold), `recall` (share of real images inside some generated image's ball: low =
    modes missing), `density` and `coverage` (their outlier-robust successors), then `precision_real` .. `coverage_real`: the same
    four between two disjoint random halves of the real set, which is what a perfect generator would score on this corpus.

    "ndb" (not in the default tuple METRICS_ALL; METRICS_EVERY has it): with half = nb_images // 2, min(50, max(2, half // 20))
    k-means bins are fitted on one random half of the real images, reduced as for "nn" (metrics.KMeans, 25 iterations).  Appends
    `ndb` (the share of bins whose share of the first `half` generated images differs from their share of that half at the 0.05
    level) and `jsd` (the Jensen-Shannon divergence of the two bin histograms), then `ndb_real` / `jsd_real`: the same for the
    other random half of the real set, which has as many images.  `ndb` well above `ndb_real` means modes missing or
    over-produced; needs nb_images >= 8."""
    if not 0 <= level <= _FINAL_LEVEL:
        raise ValueError(f"level must be in 0 .. {_FINAL_LEVEL}, got {level}")
    if nb_images < 1 or batch_size < 1:
        raise ValueError("nb_images and batch_size must be positive")
    metrics = tuple(metrics)
    if not metrics or any(m not in METRICS_EVERY for m in metrics) or len(set(metrics)) != len(metrics):
        raise ValueError(f"metrics: a non-empty subset of {METRICS_EVERY} expected, got {metrics}")
    if "prdc" in metrics and nb_images < 2 * (_PRDC_K + 1):
        raise ValueError(f"prdc needs at least {2 * (_PRDC_K + 1)} images (two halves of k + 1 = {_PRDC_K + 1}), got {nb_images}")
    if "ndb" in metrics and nb_images < _NDB_MIN_IMAGES:
        raise ValueError(f"ndb needs at least {_NDB_MIN_IMAGES} images (two halves, two bins of two in each), got {nb_images}")
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
    if "nn" in metrics and nb_images < 2:
        raise ValueError(f"nearest neighbours need at least 2 images (a real query may not match itself), got {nb_images}")
    if "prdc" in metrics and nb_images < 2 * (_PRDC_K + 1):
        raise ValueError(f"prdc needs at least {2 * (_PRDC_K + 1)} images (two halves of k + 1 = {_PRDC_K + 1}), got {nb_images}")
    if "ndb" in metrics and nb_images < _NDB_MIN_IMAGES:
        raise ValueError(f"ndb needs at least {_NDB_MIN_IMAGES} images (two halves, two bins of two in each), got {nb_images}")

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
    if any(m in metrics for m in ("msssim", "nn", "prdc", "ndb")):   # one seeded order of the dataset, shared by all four
        perm = torch.randperm(nb_images, generator=torch.Generator().manual_seed(seed)).tolist()
    if "msssim" in metrics:
        # random pairs, the same index pairs for both sets: consecutive dataset samples are adjacent chunks of one track, and
        # pairing neighbours would inflate the real number
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
    if "nn" in metrics or "prdc" in metrics or "ndb" in metrics:   # all compare images reduced to at most _NN_SIDE pixels a side
        cside = min(side, _NN_SIDE)

        def reduced(x):
            while x.shape[-1] > cside:
                x = ops.avgpool2_fwd(x)
            return x

        def real_at(idx):
            return reduced(ops.input_transform(torch.stack([dataset[i] for i in idx]).to(device).contiguous(), side))

    if "nn" in metrics:
        nq = min(nb_images, _NN_QUERIES)
        with torch.no_grad():
            fake_q = torch.cat([reduced(gen(latents[lo:lo + batch_size].contiguous(), 1.0).contiguous())
                                for lo in range(0, nq, batch_size)])[:nq].contiguous()
            real_q = torch.cat([real_at(perm[lo:min(lo + batch_size, nq)]) for lo in range(0, nq, batch_size)])
            nn_fake = NearestNeighbours(fake_q, k=_NN_K)
            nn_real = NearestNeighbours(real_q, k=_NN_K, query_ids=perm[:nq])   # a real query does not match itself
            for lo in range(0, nb_images, batch_size):
                ids = list(range(lo, min(lo + batch_size, nb_images)))
                real = real_at(ids)
                nn_fake.feed(real, ids)
                nn_real.feed(real, ids)
        comps = fake_q[0].numel()
        rms = {name: (nn.result()[0][:, 0].cpu() / comps).sqrt() for name, nn in (("fake", nn_fake), ("real", nn_real))}
        for suffix, fn in (("", torch.mean), ("_min", torch.min)):
            for name in ("fake", "real"):
                result[f"nn_{name}{suffix}"] = float(fn(rms[name]))
        for name in ("fake", "real"):
            print(f"NN RMS [{name}] = {result['nn_' + name]:.6f} (smallest {result['nn_' + name + '_min']:.6f}) at {cside} x {cside}")
        print("NN: fake well below real, or a smallest fake value near 0, means memorised training samples")
    if "prdc" in metrics:
        need, free = 2 * nb_images * 2 * cside * cside * 4, torch.cuda.mem_get_info(device)[0]
        if need > 0.75 * free:
            raise ValueError(f"prdc keeps {nb_images} real and {nb_images} generated images of {cside} x {cside} resident: {need} "
                             f"bytes, more than three quarters of the {free} bytes free on the device")
        half = nb_images // 2
        with torch.no_grad():
            prdc = PRDC(k=_PRDC_K)
            for lo in range(0, nb_images, batch_size):
                prdc.feed_real(real_at(list(range(lo, min(lo + batch_size, nb_images)))))
                prdc.feed_fake(reduced(gen(latents[lo:lo + batch_size].contiguous(), 1.0).contiguous()))
            result.update(prdc.result())
            prdc = PRDC(k=_PRDC_K)   # the data against itself: two disjoint random halves (the first pair of sets is released)
            for lo in range(0, half, batch_size):
                prdc.feed_real(real_at(perm[lo:min(lo + batch_size, half)]))
                prdc.feed_fake(real_at(perm[half + lo:min(half + lo + batch_size, 2 * half)]))
            result.update({name + "_real": value for name, value in prdc.result().items()})
        for suffix in ("", "_real"):
            for name in PRDC.KEYS:
                print(f"PRDC [{name + suffix:>14}] = {result[name + suffix]:.6f} at {cside} x {cside}, k = {_PRDC_K}")
        print("PRDC: low precision means samples off the data manifold, low recall or coverage means modes missing; compare with "
              "the _real column (two halves of the data against each other)")
    if "ndb" in metrics:
        half = nb_images // 2
        bins = _ndb_bins(half)
        need, free = half * 2 * cside * cside * 4, torch.cuda.mem_get_info(device)[0]
        if need > 0.75 * free:
            raise ValueError(f"ndb keeps {half} real images of {cside} x {cside} resident: {need} bytes, more than three quarters of "
                             f"the {free} bytes free on the device")
        with torch.no_grad():
            km = KMeans(bins, iterations=_NDB_ITERATIONS, seed=seed)   # the bins: fitted on one random half of the real set
            for lo in range(0, half, batch_size):
                km.feed(real_at(perm[lo:min(lo + batch_size, half)]))
            km.fit()
            ndb_fake, ndb_real = NDB(km), NDB(km)   # both query sets have `half` images: the z-test's power depends on the size
            for lo in range(0, half, batch_size):
                n = min(batch_size, half - lo)
                ndb_fake.feed(reduced(gen(latents[lo:lo + n].contiguous(), 1.0).contiguous()))
                ndb_real.feed(real_at(perm[half + lo:half + lo + n]))
            result.update(ndb_fake.result())
            result.update({name + "_real": value for name, value in ndb_real.result().items()})
        last = int(km.changed[-1])
        print(f"NDB: {bins} k-means bins fitted on {half} real images at {cside} x {cside}; the last of {_NDB_ITERATIONS} iterations "
              f"changed {last} labels" + ("" if last == 0 else " (not converged: raise the iterations)"))
        if half < _NDB_PER_BIN * bins:
            print(f"NDB: fewer than {_NDB_PER_BIN} reference images per bin: the test has little power")
        for suffix in ("", "_real"):
            print(f"NDB [{'ndb' + suffix:>8}] = {result['ndb' + suffix]:.6f}, JSD [{'jsd' + suffix:>8}] = {result['jsd' + suffix]:.6f}")
        print("NDB: ndb well above ndb_real means the samples are spread over the corpus differently from the data: modes missing or "
              "over-produced; ndb_real is about 0.05 for a held-out half")
    if output is not None:
        with open(output, "w") as f:
            json.dump(result, f, indent=1)
    return result

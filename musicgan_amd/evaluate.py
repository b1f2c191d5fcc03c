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


class _Images:
    """Where every metric draws its images from: `dataset` entries brought to `side` by the training loop's own input transform, and
    the generator's samples of rows of `latents`.  Which rows share a batch is up to the caller, and is part of the result: the
    generator's kernels are chosen by the batch size."""

    def __init__(self, dataset, gen, latents: torch.Tensor, side: int, batch_size: int) -> None:
        self.dataset, self.gen, self.latents, self.device = dataset, gen, latents, latents.device
        self.side, self.cside, self.batch_size = side, min(side, _NN_SIDE), batch_size
        # the space the kNN metrics compare in: how the printed lines name it, what a row is called, the numbers in a row
        self.space, self.row_what = f"at {self.cside} x {self.cside}", f"images of {self.cside} x {self.cside}"
        self.row_numel = 2 * self.cside * self.cside

    def real(self, indices) -> torch.Tensor:
        return ops.input_transform(torch.stack([self.dataset[i] for i in indices]).to(self.device).contiguous(), self.side)

    def fake(self, rows) -> torch.Tensor:
        """`rows`: a slice, or a list of row numbers"""
        if not isinstance(rows, slice):
            rows = torch.tensor(rows, device=self.device)
        with torch.no_grad():
            return self.gen(self.latents[rows].contiguous(), 1.0).contiguous()

    def reduced(self, x: torch.Tensor) -> torch.Tensor:
        """the rows the kNN metrics compare: here at most _NN_SIDE pixels a side, by 2 x 2 means"""
        while x.shape[-1] > self.cside:
            x = ops.avgpool2_fwd(x)
        return x

    def batches(self, n: int):
        """(lo, hi) of the batches that make up 0 .. n"""
        for lo in range(0, n, self.batch_size):
            yield lo, min(lo + self.batch_size, n)


def _check_resident(images: _Images, count: int, what: str) -> None:
    need, free = count * images.row_numel * 4, torch.cuda.mem_get_info(images.device)[0]
    if need > 0.75 * free:
        raise ValueError(f"{what} {images.row_what} resident: {need} bytes, more than three quarters of the "
                         f"{free} bytes free on the device")


# One runner per metric: (images, nb_images, perm, seed) -> its keys of the result, in order; it prints its own lines.  `perm` is one
# seeded order of the dataset, shared by all.
def _swd(images: _Images, nb_images: int, perm, seed: int) -> Dict[str, float]:
    swd = SWD(images.side, images.side, channels=2, images=nb_images, seed=seed)
    for lo, hi in images.batches(nb_images):
        swd.feed_real(images.real(range(lo, hi)))
        swd.feed_fake(images.fake(slice(lo, hi)))
    result = swd.result()
    for name, value in result.items():
        print(f"SWD x 1e3 [{name:>3}] = {value:.4f}")
    return result


def _msssim(images: _Images, nb_images: int, perm, seed: int) -> Dict[str, float]:
    # random pairs, the same index pairs for both sets: consecutive dataset samples are adjacent chunks of one track, and
    # pairing neighbours would inflate the real number
    half = nb_images // 2
    first, second = perm[:half], perm[half:2 * half]
    ms_real, ms_fake = (MSSSIM(images.side, images.side, channels=2, pairs=half) for _ in range(2))
    for lo, hi in images.batches(half):
        ia, ib = first[lo:hi], second[lo:hi]
        ms_real.feed(images.real(ia), images.real(ib))
        ms_fake.feed(images.fake(ia), images.fake(ib))
    result = {"msssim_real": ms_real.result(), "msssim_fake": ms_fake.result()}
    for name in result:
        print(f"MS-SSIM [{name[7:]}] = {result[name]:.6f}")
    return result


def _nn(images: _Images, nb_images: int, perm, seed: int) -> Dict[str, float]:
    nq = min(nb_images, _NN_QUERIES)
    fake_q = torch.cat([images.reduced(images.fake(slice(lo, lo + images.batch_size)))   # whole batches, cut to nq afterwards
                        for lo, _ in images.batches(nq)])[:nq].contiguous()
    real_q = torch.cat([images.reduced(images.real(perm[lo:hi])) for lo, hi in images.batches(nq)])
    nn_fake = NearestNeighbours(fake_q, k=_NN_K)
    nn_real = NearestNeighbours(real_q, k=_NN_K, query_ids=perm[:nq])   # a real query does not match itself
    for lo, hi in images.batches(nb_images):
        ids = list(range(lo, hi))
        real = images.reduced(images.real(ids))
        nn_fake.feed(real, ids)
        nn_real.feed(real, ids)
    comps = fake_q[0].numel()
    rms = {name: (nn.result()[0][:, 0].cpu() / comps).sqrt() for name, nn in (("fake", nn_fake), ("real", nn_real))}
    result = {}
    for suffix, fn in (("", torch.mean), ("_min", torch.min)):
        for name in ("fake", "real"):
            result[f"nn_{name}{suffix}"] = float(fn(rms[name]))
    for name in ("fake", "real"):
        print(f"NN RMS [{name}] = {result['nn_' + name]:.6f} (smallest {result['nn_' + name + '_min']:.6f}) {images.space}")
    print("NN: fake well below real, or a smallest fake value near 0, means memorised training samples")
    return result


def _prdc(images: _Images, nb_images: int, perm, seed: int) -> Dict[str, float]:
    _check_resident(images, 2 * nb_images, f"prdc keeps {nb_images} real and {nb_images} generated")
    half = nb_images // 2
    prdc = PRDC(k=_PRDC_K)
    for lo, hi in images.batches(nb_images):
        prdc.feed_real(images.reduced(images.real(range(lo, hi))))
        prdc.feed_fake(images.reduced(images.fake(slice(lo, hi))))
    result = prdc.result()
    prdc = PRDC(k=_PRDC_K)   # the data against itself: two disjoint random halves (the first pair of sets is released)
    for lo, hi in images.batches(half):
        prdc.feed_real(images.reduced(images.real(perm[lo:hi])))
        prdc.feed_fake(images.reduced(images.real(perm[half + lo:half + hi])))
    result.update({name + "_real": value for name, value in prdc.result().items()})
    for name in result:
        print(f"PRDC [{name:>14}] = {result[name]:.6f} {images.space}, k = {_PRDC_K}")
    print("PRDC: low precision means samples off the data manifold, low recall or coverage means modes missing; compare with "
          "the _real column (two halves of the data against each other)")
    return result


def _ndb(images: _Images, nb_images: int, perm, seed: int) -> Dict[str, float]:
    half = nb_images // 2
    bins = _ndb_bins(half)
    _check_resident(images, half, f"ndb keeps {half} real")
    km = KMeans(bins, iterations=_NDB_ITERATIONS, seed=seed)   # the bins: fitted on one random half of the real set
    for lo, hi in images.batches(half):
        km.feed(images.reduced(images.real(perm[lo:hi])))
    km.fit()
    ndb_fake, ndb_real = NDB(km), NDB(km)   # both query sets have `half` images: the z-test's power depends on the size
    for lo, hi in images.batches(half):
        ndb_fake.feed(images.reduced(images.fake(slice(lo, hi))))
        ndb_real.feed(images.reduced(images.real(perm[half + lo:half + hi])))
    result = ndb_fake.result()
    result.update({name + "_real": value for name, value in ndb_real.result().items()})
    last = int(km.changed[-1])
    print(f"NDB: {bins} k-means bins fitted on {half} real images {images.space}; the last of {_NDB_ITERATIONS} iterations "
          f"changed {last} labels" + ("" if last == 0 else " (not converged: raise the iterations)"))
    if half < _NDB_PER_BIN * bins:
        print(f"NDB: fewer than {_NDB_PER_BIN} reference images per bin: the test has little power")
    for suffix in ("", "_real"):
        print(f"NDB [{'ndb' + suffix:>8}] = {result['ndb' + suffix]:.6f}, JSD [{'jsd' + suffix:>8}] = {result['jsd' + suffix]:.6f}")
    print("NDB: ndb well above ndb_real means the samples are spread over the corpus differently from the data: modes missing or "
          "over-produced; ndb_real is about 0.05 for a held-out half")
    return result


# metric: (its runner, the fewest images it works on, how it refuses fewer); nb_images >= 1 always holds
_RUNNERS = {
    "swd": (_swd, 1, None),
    "msssim": (_msssim, 2, "MS-SSIM needs at least 2 images to pair"),
    "nn": (_nn, 2, "nearest neighbours need at least 2 images (a real query may not match itself)"),
    "prdc": (_prdc, 2 * (_PRDC_K + 1), f"prdc needs at least {2 * (_PRDC_K + 1)} images (two halves of k + 1 = {_PRDC_K + 1})"),
    "ndb": (_ndb, _NDB_MIN_IMAGES, f"ndb needs at least {_NDB_MIN_IMAGES} images (two halves, two bins of two in each)"),
}
assert tuple(_RUNNERS) == METRICS_EVERY


def _check_sizes(metrics: Sequence[str], nb_images: int) -> None:
    for name, (_, least, refusal) in _RUNNERS.items():
        if name in metrics and nb_images < least:
            raise ValueError(f"{refusal}, got {nb_images}")


def _open(source, check_sizes, gen_dict_state: str, rand_channels: int, input_dataset: str, level: int, nb_images: int,
          batch_size: int, seed: int):
    """What every driver starts with: the generator, the dataset, one draw of latents and one seeded order of the dataset.
    `source`: the _Images class to draw from; `check_sizes(n)` refuses an image count.  Returns (images, nb_images clipped to the
    dataset, perm)."""
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
    check_sizes(nb_images)   # ... and for what the dataset holds

    print(f"Evaluate {nb_images} real and {nb_images} generated images of {side} x {side}...")
    rng = torch.Generator(device=device).manual_seed(seed)
    # every latent in one draw (a few MB): the samples do not depend on the batch size
    latents = torch.randn(nb_images, rand_channels, _LATENT_H, _LATENT_W, device=device, generator=rng)
    perm = torch.randperm(nb_images, generator=torch.Generator().manual_seed(seed)).tolist()
    return source(dataset, gen, latents, side, batch_size), nb_images, perm


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
    _check_sizes(metrics, nb_images)   # before any work ...
    images, nb_images, perm = _open(_Images, lambda n: _check_sizes(metrics, n), gen_dict_state, rand_channels, input_dataset, level,
                                    nb_images, batch_size, seed)
    result = {}
    for name in METRICS_EVERY:
        if name in metrics:
            result.update(_RUNNERS[name][0](images, nb_images, perm, seed))
    if output is not None:
        with open(output, "w") as f:
            json.dump(result, f, indent=1)
    return result

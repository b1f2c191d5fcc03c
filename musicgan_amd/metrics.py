"""Evaluation metrics.  (1) The sliced Wasserstein distance (SWD) between local patches of Laplacian-pyramid levels of two image sets
(Karras et al., "Progressive Growing of GANs", ICLR 2018).  One number per pyramid level says how far the generated spectrograms
are from the data at that scale; it needs no pretrained network and works on any channel count.  The definition is stated in
DESIGN.md ("Evaluation: sliced Wasserstein distance"); every step runs in the HIP kernels of csrc/swd.hip.

    swd = SWD(512, 512, images=8192)
    for batch in real:  swd.feed_real(batch)      # float32 cuda (n, C, H, W), any split
    for batch in fake:  swd.feed_fake(batch)
    swd.result()                                   # {"512": .., "256": .., ..., "16": .., "avg": ..}, x 1000 as in the paper

All random draws (patch centres, directions) come from one CPU generator when the object is built, so a result depends on the
seed and the images alone.  The two sets get independent centres, so SWD(A, B) and SWD(B, A) differ by sampling noise;
sliced_wasserstein() itself is exactly symmetric.

(2) MS-SSIM between pairs of images of ONE set (the other number Karras et al. report): how much the samples differ from each
other.  A generator that repeats itself scores well on SWD and high here.  Definition: DESIGN.md ("Evaluation: MS-SSIM sample
diversity"); kernels: csrc/ssim.hip through musicgan_amd/ssim_ops.py.

    ms = MSSSIM(512, 512, pairs=4096)
    for a, b in pairs_of_batches:  ms.feed(a, b)  # float32 cuda (n, C, H, W) each, values in [-1, 1], any split
    ms.result()                                   # the mean over the pairs, 1 = identical images; ms.values: one per pair

(3) Nearest training neighbours in pixel space (the third check of Karras et al.): did the generator copy its corpus?  Squared L2
distances between flattened float32 images, exact to a derived bound at any size.  Definition and error analysis: DESIGN.md
("Evaluation: nearest training neighbours"); kernels: csrc/nn.hip through musicgan_amd/nn_ops.py.

    nn = NearestNeighbours(queries, k=1)          # float32 cuda (Q, ...), kept resident; query_ids: leave-one-out
    for batch, ids in dataset:  nn.feed(batch, ids)   # (B, ...) of the same trailing shape, B distinct ids >= 0, any split / order
    dist, idx = nn.result()                       # (Q, k) float64 squared distances ascending, (Q, k) int64 ids; both cuda
    pairwise_sqdist(a, b)                         # the (Na, Nb) float64 distance matrix on its own

(4) Precision / recall (Kynkaanniemi et al., NeurIPS 2019) and density / coverage (Naeem et al., ICML 2020) in pixel space: which
way is a generator wrong -- samples off the data manifold, or on it but covering only part of it?  Definition: DESIGN.md 4.14;
kernels: csrc/prdc.hip (and the merge of csrc/nn.hip) through musicgan_amd/nn_ops.py.

    prdc = PRDC(k=3)
    for batch in real:  prdc.feed_real(batch)     # float32 cuda (B, ...), one trailing shape, any split, any interleaving
    for batch in fake:  prdc.feed_fake(batch)
    prdc.result()                                 # {"precision": .., "recall": .., "density": .., "coverage": ..}
    prdc.per_sample()                             # the radii, ball counts and nearest-fake distances behind them, on the device

(5) NDB / JSD over k-means bins (Richardson & Weiss, "On GANs and GMMs", NeurIPS 2018; the numbers GANSynth reports): how is the
probability mass of the samples spread over the corpus?  Bins are the Voronoi cells of a deterministic k-means on the reference
images; every bin's share of the queries is tested against its share of the reference.  Definition: DESIGN.md 4.15; kernels:
csrc/kmeans.hip through musicgan_amd/km_ops.py, distances through nn_ops.nn_sqdist_tiled.

    km = KMeans(bins=50)
    for batch in real:  km.feed(batch)            # float32 cuda (B, ...), one trailing shape, any split; the ORDER matters
    km.fit()                                      # launches only
    ndb = NDB(km)
    for batch in fake:  ndb.feed(batch)           # assigned and counted, not kept
    ndb.result()                                  # {"ndb": share of statistically different bins, "jsd": of the two histograms}

(6) A feature space other than pixels that needs no pretrained network: the log-mel spectrogram of what an image decodes to, and in
it the Frechet distance between the Gaussians fitted to two sets (the formula of FID).  Definition: DESIGN.md 4.19; kernels:
csrc/logmel.hip and csrc/moments.hip through musicgan_amd/mel_ops.py.

    rows = LogMel(512, 512, pools=8)              # (B, 2, 512, 512) float32 cuda -> (B, 64 * 8) float32 cuda
    fd = Frechet()
    for batch in real:  fd.feed_real(rows(batch)) # any (B, ...) float32 cuda batch, any split
    for batch in fake:  fd.feed_fake(rows(batch))
    fd.result()                                   # float; fd.moments(): the float64 means and covariances, on the device

(7) The Kernel Inception Distance in the same rows (Binkowski et al., "Demystifying MMD GANs", ICLR 2018): the unbiased estimate of
the squared maximum mean discrepancy under k(x, y) = (x.y / d + 1)^3, as mean and standard deviation over random subsets.  Its
expectation does not depend on the set sizes, which the Frechet distance's does.  Definition and error bound: DESIGN.md 4.20;
kernels: csrc/kid.hip through musicgan_amd/kid_ops.py -- no kernel matrix is stored.

    kid = KID(subsets=100, subset_size=1000)
    for batch in real:  kid.feed_real(rows(batch))  # any (B, ...) float32 cuda batch, any split, any interleaving
    for batch in fake:  kid.feed_fake(rows(batch))
    kid.result()                                  # {"kid": .., "kid_std": .., "kid_full": ..}; rows standardised by the real moments
    kid.per_sample()                              # (n_fake,) float64 cuda: the witness function at every generated row
    poly_mmd2(x, y)                               # the estimate for two row tensors as they are

(8) The same rows taken from waveforms, where the phase counts: WaveLogMel.  Definition and error bound: DESIGN.md 4.21; kernels:
csrc/melspec.hip through mel_ops.mel_power and mel_ops.logmel_pool.

    rows = WaveLogMel(pools=8)(waves)             # (B, L) float32 cuda -> (B * W, 64 * 8): a row per window of 512 frames

(9) The perceptual path length (Karras et al., "A Style-Based Generator Architecture for GANs", CVPR 2019) with the squared distance
of those rows in the place of LPIPS: how fast the output moves when the latent moves a small step along an interpolation arc.
It needs a generator only, no data.  Definition and error bounds: DESIGN.md 4.22; kernels: csrc/ppl.hip through musicgan_amd/ppl_ops.py.

    ppl = PPL(rows_of, rand_channels=32)          # rows_of: latents (B, 32, 2, 2) float32 cuda -> rows (B, D) float32 cuda
    ppl.feed(8192)                                # pairs; any split
    ppl.result()                                  # {"ppl": .., "ppl_mean": .., "ppl_chord": .., "ppl_ratio": .., "ppl_pairs": ..}
    ppl.per_pair()                                # (pairs,) float64 cuda"""
from __future__ import annotations

import math
import operator
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import kid_ops, km_ops, mel_ops, nn_ops, ops, ppl_ops, ssim_ops


def pyramid_sides(side_h: int, side_w: int, min_side: int = 16) -> List[Tuple[int, int]]:
    """(height, width) of every level, finest first: halved while the short side stays >= min_side"""
    if side_h < 1 or side_w < 1 or min_side < 1:
        raise ValueError(f"positive sides expected, got {side_h} x {side_w}, min_side {min_side}")
    if min(side_h, side_w) < min_side:
        raise ValueError(f"a {side_h} x {side_w} image is smaller than the smallest pyramid level ({min_side})")
    sides = [(side_h, side_w)]
    while min(sides[-1]) // 2 >= min_side and sides[-1][0] % 2 == 0 and sides[-1][1] % 2 == 0:
        sides.append((sides[-1][0] // 2, sides[-1][1] // 2))
    return sides


def _check_pyramid(h: int, w: int, levels: int) -> None:
    if levels < 1:
        raise ValueError(f"levels must be >= 1, got {levels}")
    f = 1 << (levels - 1)
    if h % f or w % f:
        raise ValueError(f"a {levels}-level pyramid needs sides divisible by {f}, got {h} x {w}")
    if levels > 1 and min(h, w) // f < 2:
        raise ValueError(f"the coarsest of {levels} levels of a {h} x {w} image is smaller than 2")


def laplacian_pyramid(x: torch.Tensor, levels: int) -> List[torch.Tensor]:
    """Laplacian pyramid of a float32 cuda batch (N, C, H, W), finest level first; the last entry is the Gaussian residual."""
    if x.dim() != 4:
        raise ValueError(f"(N, C, H, W) expected, got {tuple(x.shape)}")
    _check_pyramid(x.shape[2], x.shape[3], levels)
    out, g = [], x
    for _ in range(levels - 1):
        nxt = ops.swd_pyr_down(g)
        out.append(ops.swd_pyr_lap(g, nxt))
        g = nxt
    if levels == 1:
        ops._chk_typed("laplacian_pyramid", x)
    out.append(g)
    return out


def patch_descriptors(level: torch.Tensor, centres: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                      row: int = 0, patch: int = 7) -> Tuple[torch.Tensor, torch.Tensor]:
    """The (C, patch, patch) neighbourhoods of `level` (N, C, H, W) around `centres` (N, P, 2) int32 (row, column), flattened
    channel-major.  Returns (desc, stats): desc (M, C patch^2) raw descriptors, stats (M / P, C, 2) float64 per-image sums and
    sums of squares.  `out` = such a pair to append to: this batch fills rows row .. row + N P (row a multiple of P)."""
    if level.dim() != 4 or centres.dim() != 3 or centres.shape[0] != level.shape[0] or centres.shape[2] != 2:
        raise ValueError(f"level (N, C, H, W) and centres (N, P, 2) expected, got {tuple(level.shape)}, {tuple(centres.shape)}")
    n, c, h, w = level.shape
    p = centres.shape[1]
    if patch < 1 or patch % 2 == 0 or patch > min(h, w):
        raise ValueError(f"an odd patch size <= {min(h, w)} expected for a {h} x {w} level, got {patch}")
    if row % p:
        raise ValueError(f"row offset {row} is not a multiple of the {p} patches per image")
    if out is None:
        if row:
            raise ValueError("a row offset needs the buffers to append to")
        ops._chk_typed("patch_descriptors", level)
        out = (torch.empty((n * p, c * patch * patch), dtype=torch.float32, device=level.device),
               torch.empty((n, c, 2), dtype=torch.float64, device=level.device))
    desc, stats = out
    if desc.dim() != 2 or desc.shape[1] != c * patch * patch or row + n * p > desc.shape[0] or \
            tuple(stats.shape) != (desc.shape[0] // p, c, 2):
        raise ValueError(f"rows {row} .. {row + n * p} of {c * patch * patch} numbers do not fit buffers of shape "
                         f"{tuple(desc.shape)}, {tuple(stats.shape)}")
    ops.swd_gather(level, centres, desc, stats, patch, row)
    return desc, stats


def channel_stats(stats: torch.Tensor, per_image: int) -> torch.Tensor:
    """(images, C, 2) float64 sums -> (C, 3) float32 (mean, 1 / std, std), population statistics over images * per_image values
    per channel, added in an order that does not depend on how the images arrived"""
    return ops.swd_stats_finish(stats, per_image)


def segmented_sort_(x: torch.Tensor) -> torch.Tensor:
    """Sort every row of a contiguous float32 cuda (S, M) tensor ascending, in place.  Finite values and +-inf are totally
    ordered (-0.0 and +0.0 in either order); NaN is outside the contract."""
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"a non-empty (S, M) tensor expected, got {tuple(x.shape)}")
    return ops.swd_sort_segments_(x)


def sliced_wasserstein(desc_a: torch.Tensor, stats_a: torch.Tensor, desc_b: torch.Tensor, stats_b: torch.Tensor,
                       directions: torch.Tensor, *, patch: int = 7, out: Optional[torch.Tensor] = None,
                       work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One repeat of the distance: normalise both descriptor sets per channel, project them on the unit `directions` (D, K),
    sort every direction's projections and return the mean |sorted A - sorted B| as a 0-dim cuda tensor (not yet x 1000).
    `out`: a one-element float32 tensor to write to; `work`: a (2, D, M) float32 buffer to reuse."""
    if desc_a.dim() != 2 or desc_a.shape != desc_b.shape:
        raise ValueError(f"two descriptor sets of one shape expected, got {tuple(desc_a.shape)} and {tuple(desc_b.shape)}")
    m, k = desc_a.shape
    if directions.dim() != 2 or directions.shape[1] != k:
        raise ValueError(f"directions (D, {k}) expected, got {tuple(directions.shape)}")
    if stats_a.shape != stats_b.shape or stats_a.dim() != 3 or k != stats_a.shape[1] * patch * patch or m % stats_a.shape[0]:
        raise ValueError(f"statistics (images, C, 2) with C * {patch}^2 = {k} expected, got {tuple(stats_a.shape)} and "
                         f"{tuple(stats_b.shape)}")
    d = directions.shape[0]
    per_image = (m // stats_a.shape[0]) * patch * patch
    ops._chk_typed("sliced_wasserstein", desc_a, desc_b, directions)
    if work is None:
        work = torch.empty((2, d, m), dtype=torch.float32, device=desc_a.device)
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=desc_a.device)
    ops.swd_project(desc_a, ops.swd_stats_finish(stats_a, per_image), directions, work[0], patch)
    ops.swd_project(desc_b, ops.swd_stats_finish(stats_b, per_image), directions, work[1], patch)
    ops.swd_sort_segments_(work.view(2 * d, m))
    ops.swd_distance(work[0], work[1], out)
    return out


def draw(sides: List[Tuple[int, int]], channels: int, images: int, patches_per_image: int, patch: int, dir_repeats: int,
         dirs_per_repeat: int, seed: int):
    """The random draws of one evaluation, from one CPU generator seeded with `seed`: for each level from finest to coarsest the
    (images, P, 2) centres of the first set (rows, then columns), those of the second set, then the (R, D, K) float32 standard
    normal directions, each divided by its norm.  Returns [(centres_a, centres_b, directions)] per level (int32, int32, float32)."""
    gen = torch.Generator().manual_seed(seed)
    half, k = patch // 2, channels * patch * patch
    out = []
    for h, w in sides:
        cen = []
        for _ in range(2):
            ys = torch.randint(half, h - half, (images, patches_per_image), generator=gen)
            xs = torch.randint(half, w - half, (images, patches_per_image), generator=gen)
            cen.append(torch.stack((ys, xs), dim=2).to(torch.int32))
        dirs = torch.randn(dir_repeats, dirs_per_repeat, k, generator=gen, dtype=torch.float32)
        out.append((cen[0], cen[1], dirs / dirs.norm(dim=2, keepdim=True)))
    return out


class SWD:
    """Sliced Wasserstein distance between `images` real and `images` generated (channels, side_h, side_w) images.  Descriptors of
    every level stay on the device (images * patches_per_image * channels * patch^2 floats per level and set), so each image is
    seen once; feeding launches kernels only, result() does the projections, sorts and the one copy to the host."""

    def __init__(self, side_h: int, side_w: int, channels: int = 2, images: int = 8192, patches_per_image: int = 128,
                 patch: int = 7, dir_repeats: int = 4, dirs_per_repeat: int = 128, min_side: int = 16, seed: int = 0) -> None:
        if channels < 1 or images < 1 or patches_per_image < 1 or dir_repeats < 1 or dirs_per_repeat < 1:
            raise ValueError("channels, images, patches_per_image, dir_repeats and dirs_per_repeat must be positive")
        if patch < 1 or patch % 2 == 0:
            raise ValueError(f"an odd patch size expected, got {patch}")
        if min_side < patch:
            raise ValueError(f"the smallest level ({min_side}) is smaller than the patch ({patch})")
        self.sides = pyramid_sides(side_h, side_w, min_side)
        _check_pyramid(side_h, side_w, len(self.sides))
        self.shape = (channels, side_h, side_w)
        self.images, self.patches, self.patch = images, patches_per_image, patch
        self.repeats, self.dirs = dir_repeats, dirs_per_repeat
        self.draws = draw(self.sides, channels, images, patches_per_image, patch, dir_repeats, dirs_per_repeat, seed)
        self._dev = None
        self._count = [0, 0]

    def _setup(self, device) -> None:
        c, k, m = self.shape[0], self.shape[0] * self.patch ** 2, self.images * self.patches
        self._dev = device
        self._centres = [(a.to(device), b.to(device)) for a, b, _ in self.draws]
        self._dirs = [d.to(device) for _, _, d in self.draws]
        self._desc = [[torch.empty((m, k), dtype=torch.float32, device=device) for _ in range(2)] for _ in self.sides]
        self._stats = [[torch.empty((self.images, c, 2), dtype=torch.float64, device=device) for _ in range(2)] for _ in self.sides]

    def _feed(self, which: int, batch: torch.Tensor) -> None:
        if batch.dim() != 4 or tuple(batch.shape[1:]) != self.shape:
            raise ValueError(f"(n, {', '.join(map(str, self.shape))}) expected, got {tuple(batch.shape)}")
        n, done = batch.shape[0], self._count[which]
        if done + n > self.images:
            raise ValueError(f"{done + n} images fed, the evaluation was sized for {self.images}")
        ops._chk_typed("SWD.feed", batch)
        if self._dev is None:
            self._setup(batch.device)
        for i, lvl in enumerate(laplacian_pyramid(batch, len(self.sides))):
            patch_descriptors(lvl, self._centres[i][which][done:done + n], (self._desc[i][which], self._stats[i][which]),
                              done * self.patches, self.patch)
        self._count[which] = done + n

    def feed_real(self, batch: torch.Tensor) -> None:
        self._feed(0, batch)

    def feed_fake(self, batch: torch.Tensor) -> None:
        self._feed(1, batch)

    def result(self) -> Dict[str, float]:
        """{"<short side of the level>": SWD x 1000, ..., "avg": their plain average} as Python floats"""
        if self._count != [self.images, self.images]:
            raise ValueError(f"{self._count[0]} real and {self._count[1]} generated images fed, {self.images} of each expected")
        m = self.images * self.patches
        work = torch.empty((2, self.dirs, m), dtype=torch.float32, device=self._dev)
        dist = torch.empty((len(self.sides), self.repeats), dtype=torch.float32, device=self._dev)
        for i in range(len(self.sides)):
            for r in range(self.repeats):
                sliced_wasserstein(self._desc[i][0], self._stats[i][0], self._desc[i][1], self._stats[i][1], self._dirs[i][r],
                                   patch=self.patch, out=dist[i, r], work=work)
        host = dist.cpu().double()
        out = {str(min(s)): float(host[i].mean() * 1000.0) for i, s in enumerate(self.sides)}
        out["avg"] = float(sum(out.values()) / len(out))
        return out


# ------------------------------------------------------------------ MS-SSIM
MSSSIM_WINDOW, MSSSIM_MAX_SCALES = 11, 5


def ms_ssim_scales(h: int, w: int) -> int:
    """The number of scales S of an h x w image: the largest S <= 5 with both sides divisible by 2^(S-1) and the short side of
    the coarsest scale >= 11 (5 at 512 x 512, 4 at 128, 3 at 64, 2 at 32, 1 at 16: plain SSIM)."""
    if min(h, w) < MSSSIM_WINDOW:
        raise ValueError(f"a {h} x {w} image is smaller than the {MSSSIM_WINDOW} x {MSSSIM_WINDOW} window")
    s = 1
    while s < MSSSIM_MAX_SCALES and h % (1 << s) == 0 and w % (1 << s) == 0 and (min(h, w) >> s) >= MSSSIM_WINDOW:
        s += 1
    return s


def _check_pairs(a: torch.Tensor, b: torch.Tensor) -> int:
    if a.dim() != 4 or a.shape != b.shape or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"two non-empty (n, C, H, W) batches of one shape expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    return ms_ssim_scales(a.shape[2], a.shape[3])


def ms_ssim_terms(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(n, S) float64: per pair the mean of cs over channels and valid pixels of the scales 0 .. S-2, then the mean of ssim of
    the last scale -- the factors of ms_ssim before the clamp and the weights"""
    scales = _check_pairs(a, b)
    ops._chk_typed("ms_ssim_terms", a, b)
    values = torch.empty(a.shape[0], dtype=torch.float64, device=a.device)
    terms = torch.empty((a.shape[0], scales), dtype=torch.float64, device=a.device)
    ssim_ops.ms_ssim_into(a, b, values, terms)
    return terms


def ms_ssim(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(n,) float64 cuda: MS-SSIM of every pair (a[i], b[i]) of two float32 cuda batches (n, C, H, W) with values in [-1, 1]; a
    pair's value depends on its own pixels alone.  A negative mean at any scale makes the pair's value exactly 0."""
    _check_pairs(a, b)
    ops._chk_typed("ms_ssim", a, b)
    values = torch.empty(a.shape[0], dtype=torch.float64, device=a.device)
    ssim_ops.ms_ssim_into(a, b, values)
    return values


class MSSSIM:
    """Mean MS-SSIM over `pairs` pairs of (channels, side_h, side_w) images.  Feeding launches kernels only; result() takes the
    mean on the device, in an order that depends on `pairs` alone, and makes the one copy to the host."""

    def __init__(self, side_h: int, side_w: int, channels: int = 2, pairs: int = 4096) -> None:
        if channels < 1 or pairs < 1:
            raise ValueError("channels and pairs must be positive")
        self.scales = ms_ssim_scales(side_h, side_w)
        self.shape = (channels, side_h, side_w)
        self.pairs = pairs
        self._values = None
        self._count = 0

    def feed(self, a: torch.Tensor, b: torch.Tensor) -> None:
        if a.dim() != 4 or a.shape != b.shape or tuple(a.shape[1:]) != self.shape or a.shape[0] < 1:
            raise ValueError(f"two batches (n, {', '.join(map(str, self.shape))}) expected, got {tuple(a.shape)} and {tuple(b.shape)}")
        n = a.shape[0]
        if self._count + n > self.pairs:
            raise ValueError(f"{self._count + n} pairs fed, the evaluation was sized for {self.pairs}")
        ops._chk_typed("MSSSIM.feed", a, b)
        if self._values is None:
            self._values = torch.empty(self.pairs, dtype=torch.float64, device=a.device)
        ssim_ops.ms_ssim_into(a, b, self._values, None, self._count)
        self._count += n

    @property
    def values(self) -> torch.Tensor:
        """the per-pair values fed so far, float64 on the device"""
        if self._values is None:
            raise ValueError("no pair fed yet")
        return self._values[:self._count]

    def result(self) -> float:
        if self._count != self.pairs:
            raise ValueError(f"{self._count} pairs fed, {self.pairs} expected")
        out = torch.empty(1, dtype=torch.float64, device=self._values.device)
        return float(ssim_ops.ssim_mean(self._values, out).cpu()[0])


# ------------------------------------------------------------------ nearest neighbours
_NN_WS_BYTES = 256 << 20   # the partial sums of one distance launch stay below this: longer reference batches go in pieces


def _rows(x: torch.Tensor, what: str) -> torch.Tensor:
    """(N, ...) -> (N, D), a view; N >= 1 and D >= 1"""
    if x.dim() < 2 or x.shape[0] < 1 or x[0].numel() < 1:
        raise ValueError(f"{what}: a non-empty batch (N, ...) expected, got {tuple(x.shape)}")
    ops._chk_typed(what, x)
    return x.view(x.shape[0], -1)


def _check_batch(batch: torch.Tensor, shape: Tuple[int, ...]) -> None:
    if batch.dim() < 2 or tuple(batch.shape[1:]) != shape or batch.shape[0] < 1:
        raise ValueError(f"a non-empty batch (B, {', '.join(map(str, shape))}) expected, got {tuple(batch.shape)}")


def _blocks(n: int, step: int):
    """(lo, hi) of the row blocks of at most `step` rows that make up 0 .. n"""
    for lo in range(0, n, step):
        yield lo, min(lo + step, n)


def _block_rows(block_bytes: int, nr: int, d: int) -> int:
    """the query rows whose distance block against nr rows of d numbers, with the kernel's workspace, fits block_bytes"""
    per_row = 8 * nr + nn_ops.nn_tiled_ws_bytes(1, nr, d)
    return max(1, block_bytes // per_row)


def _best_lists(n: int, k: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """the empty (n, k) lists nn_merge fills: float64 distances and int64 ids"""
    return (torch.full((n, k), nn_ops.EMPTY, dtype=torch.float64, device=device),
            torch.full((n, k), -1, dtype=torch.int64, device=device))


class _RowStore:
    """The rows `owner` (a class name, for the messages) was fed, kept on the device: every batch is flattened and cloned as it
    arrives, and the pieces are concatenated once, when the rows are first asked for."""

    def __init__(self, owner: str) -> None:
        self.owner, self.n, self._parts = owner, 0, []

    def add(self, batch: torch.Tensor, what: str, shape: Optional[Tuple[int, ...]]) -> Tuple[int, ...]:
        """keep a non-empty float32 cuda batch (B, ...) whose trailing shape is `shape` (None: any); returns that shape"""
        if batch.dim() < 2 or batch.shape[0] < 1 or batch[0].numel() < 1:
            raise ValueError(f"{what}: a non-empty batch (B, ...) expected, got {tuple(batch.shape)}")
        if shape is not None and tuple(batch.shape[1:]) != shape:
            raise ValueError(f"{what}: a batch (B, {', '.join(map(str, shape))}) expected, got {tuple(batch.shape)}")
        rows = _rows(batch, f"{self.owner}.{what}")
        self._parts.append(rows.clone())
        self.n += rows.shape[0]
        return tuple(batch.shape[1:])

    def rows(self) -> torch.Tensor:
        """(n, D) float32"""
        if len(self._parts) > 1:
            self._parts = [torch.cat(self._parts)]
        return self._parts[0]


def _sqdist(q: torch.Tensor, qn: torch.Tensor, r: torch.Tensor, out: torch.Tensor) -> None:
    """out (nq, nr) = the distances of every (q[i], r[j]); r goes through in pieces of rows (a pair's value does not depend on
    the piece it is in)"""
    nq, nr, d = q.shape[0], r.shape[0], q.shape[1]
    per_row = nn_ops.nn_ws_bytes(nq, 1, d)
    step = max(16, _NN_WS_BYTES // per_row // 16 * 16)
    if step >= nr:
        nn_ops.nn_sqdist(q, r, qn, nn_ops.nn_sqnorm(r), out)
        return
    for lo, hi in _blocks(nr, step):
        piece = r[lo:hi]
        out[:, lo:hi] = nn_ops.nn_sqdist(q, piece, qn, nn_ops.nn_sqnorm(piece))


def pairwise_sqdist(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(Na, Nb) float64 cuda: the squared L2 distance between every a[i] and b[j] of two float32 cuda batches (Na, ...) and
    (Nb, ...) with the same number of components per image; >= 0, and a pair's value depends on its two images alone."""
    if a.dim() < 2 or b.dim() < 2 or a.shape[1:] != b.shape[1:] or a.numel() < 1 or b.numel() < 1:
        raise ValueError(f"two non-empty batches of one trailing shape expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    a, b = _rows(a, "pairwise_sqdist"), _rows(b, "pairwise_sqdist")
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float64, device=a.device)
    _sqdist(a, nn_ops.nn_sqnorm(a), b, out)
    return out


def _id_list(ids, n: int, what: str) -> List[int]:
    try:
        ids = ids.tolist() if isinstance(ids, torch.Tensor) else [operator.index(i) for i in ids]
    except TypeError:
        raise ValueError(f"{what}: integers expected") from None
    if len(ids) != n or any(not isinstance(i, int) for i in ids):
        raise ValueError(f"{what}: {n} integers expected, got {len(ids)} entries")
    return ids


def _ids_to(ids: List[int], device) -> torch.Tensor:
    """int64 on the device, through pinned memory: the copy does not make the host wait"""
    return torch.tensor(ids, dtype=torch.int64).pin_memory().to(device, non_blocking=True)


class NearestNeighbours:
    """The k nearest of everything fed, by squared L2 distance, for each of Q resident query images.  `query_ids`: one integer
    per query (-1: none); a fed image with a query's own id is not its neighbour (leave-one-out for queries taken from the fed
    set).  The ids of all fed images are distinct and >= 0; ties in the distance go to the smaller id, so the result is the same
    bit for bit for any split of the references into batches and any order of the batches.  Feeding launches kernels only."""

    def __init__(self, queries: torch.Tensor, k: int = 1, query_ids=None) -> None:
        if not isinstance(k, int) or not 1 <= k <= nn_ops.MAX_K:
            raise ValueError(f"k in 1 .. {nn_ops.MAX_K} expected, got {k}")
        self._q = _rows(queries, "NearestNeighbours")
        self.k, self.shape = k, tuple(queries.shape[1:])
        nq, dev = self._q.shape[0], queries.device
        self._qid = None
        if query_ids is not None:
            ids = _id_list(query_ids, nq, "query_ids")
            if any(i < -1 for i in ids):
                raise ValueError("query_ids: ids >= 0, or -1 for a query without one, expected")
            self._qid = _ids_to(ids, dev)
        self._qn = nn_ops.nn_sqnorm(self._q)
        self._best_d, self._best_i = _best_lists(nq, k, dev)
        self._fed = 0

    def feed(self, batch: torch.Tensor, ids) -> None:
        _check_batch(batch, self.shape)
        ids = _id_list(ids, batch.shape[0], "ids")
        if len(set(ids)) != len(ids) or min(ids) < 0:
            raise ValueError("ids: distinct integers >= 0 expected")
        r = _rows(batch, "NearestNeighbours.feed")
        dist = torch.empty((self._q.shape[0], r.shape[0]), dtype=torch.float64, device=r.device)
        _sqdist(self._q, self._qn, r, dist)
        nn_ops.nn_merge(dist, _ids_to(ids, r.device), self._best_d, self._best_i, self._qid)
        self._fed += r.shape[0]

    def result(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(dist, idx): (Q, k) float64 squared distances, ascending, and the (Q, k) int64 ids they belong to; copies, on the device"""
        if self._fed < self.k:
            raise ValueError(f"{self._fed} references fed, at least {self.k} expected")
        if bool((self._best_i[:, -1] < 0).any()):   # a query whose own id was among fewer than k + 1 references
            raise ValueError(f"{self._fed} references fed: some query has fewer than {self.k} neighbours that are not itself")
        return self._best_d.clone(), self._best_i.clone()


# ------------------------------------------------------------------ precision / recall / density / coverage
class PRDC:
    """k-nearest-neighbour manifold metrics between a real and a fake set of images, on squared L2 distances in pixel space.
    radius(x) = the distance from x to its k-th nearest OTHER member of its own set (leave-one-out by position);
    precision = the share of fakes inside some real ball, recall = the share of reals inside some fake ball,
    density = the number of real balls a fake lies in, averaged and divided by k, coverage = the share of reals whose nearest
    fake is inside their own ball.  Feeding keeps a device copy and launches nothing else; the matrices real x real, fake x fake,
    fake x real and real x fake go through nn_sqdist_tiled in row blocks of at most `block_bytes` (distance block plus kernel
    workspace) when the result is first asked for.  A pair's distance depends on its two rows alone, the radii come from a merge
    ordered by (distance, position), counts are integers and minima exact: every output is the same bit for bit for any split
    and order of the feeds and any `block_bytes`."""

    KEYS = ("precision", "recall", "density", "coverage")

    def __init__(self, k: int = 3, block_bytes: int = 256 << 20) -> None:
        if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= nn_ops.MAX_K:
            raise ValueError(f"k in 1 .. {nn_ops.MAX_K} expected, got {k}")
        if block_bytes < 1:
            raise ValueError(f"block_bytes must be positive, got {block_bytes}")
        self.k, self.block_bytes, self.shape = k, int(block_bytes), None
        self._real, self._fake = _RowStore("PRDC"), _RowStore("PRDC")   # the two sets share the one trailing shape
        self._per_sample = None

    def _feed(self, store: _RowStore, what: str, batch: torch.Tensor) -> None:
        self.shape = store.add(batch, what, self.shape)
        self._per_sample = None

    def feed_real(self, batch: torch.Tensor) -> None:
        self._feed(self._real, "feed_real", batch)

    def feed_fake(self, batch: torch.Tensor) -> None:
        self._feed(self._fake, "feed_fake", batch)

    def _radius(self, x: torch.Tensor, xn: torch.Tensor) -> torch.Tensor:
        """every row's distance to its k-th nearest other row of x"""
        n, d, dev = x.shape[0], x.shape[1], x.device
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        best_d, best_i = _best_lists(n, self.k, dev)
        for lo, hi in _blocks(n, _block_rows(self.block_bytes, n, d)):
            dist = nn_ops.nn_sqdist_tiled(x[lo:hi], x, xn[lo:hi], xn)
            nn_ops.nn_merge(dist, ids, best_d[lo:hi], best_i[lo:hi], ids[lo:hi])
        return best_d[:, self.k - 1].contiguous()

    def _scan(self, q: torch.Tensor, qn: torch.Tensor, r: torch.Tensor, rn: torch.Tensor, radius: torch.Tensor):
        """(count, rowmin) of every row of q against the balls of r"""
        nq, nr, d, dev = q.shape[0], r.shape[0], q.shape[1], q.device
        count = torch.zeros(nq, dtype=torch.int64, device=dev)
        rowmin = torch.full((nq,), float("inf"), dtype=torch.float64, device=dev)
        for lo, hi in _blocks(nq, _block_rows(self.block_bytes, nr, d)):
            dist = nn_ops.nn_sqdist_tiled(q[lo:hi], r, qn[lo:hi], rn)
            nn_ops.prdc_scan(dist, radius, count[lo:hi], rowmin[lo:hi])
        return count, rowmin

    def per_sample(self) -> Dict[str, torch.Tensor]:
        """device tensors: radius_real / radius_fake (float64, the k-th nearest other member of the own set), count_fake (int64,
        per fake: the real balls it lies in), count_real (int64, per real: the fake balls it lies in), nearest_fake (float64, per
        real: the distance to the nearest fake)"""
        if min(self._real.n, self._fake.n) < self.k + 1:
            raise ValueError(f"{self._real.n} real and {self._fake.n} fake images fed, at least k + 1 = {self.k + 1} of each "
                             "expected")
        if self._per_sample is None:
            real, fake = self._real.rows(), self._fake.rows()
            rn, fn = nn_ops.nn_sqnorm(real), nn_ops.nn_sqnorm(fake)
            radius_real, radius_fake = self._radius(real, rn), self._radius(fake, fn)
            count_fake, _ = self._scan(fake, fn, real, rn, radius_real)
            count_real, nearest_fake = self._scan(real, rn, fake, fn, radius_fake)
            self._per_sample = dict(radius_real=radius_real, radius_fake=radius_fake, count_fake=count_fake, count_real=count_real,
                                    nearest_fake=nearest_fake)
        return dict(self._per_sample)

    def result(self) -> Dict[str, float]:
        p = self.per_sample()
        n_real, n_fake = self._real.n, self._fake.n
        # four integer sums on the device, one copy, the divisions on the host: exact counts over exact divisors
        inside, seen, balls, covered = torch.stack([(p["count_fake"] > 0).sum(), (p["count_real"] > 0).sum(), p["count_fake"].sum(),
                                                    (p["nearest_fake"] <= p["radius_real"]).sum()]).tolist()
        return {"precision": inside / n_fake, "recall": seen / n_real, "density": balls / (self.k * n_fake),
                "coverage": covered / n_real}


# ------------------------------------------------------------------ NDB / JSD over k-means bins
NDB_Z = 1.959963984540054   # |z| beyond which a bin is different: two-sided at 0.05, the paper's level


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def ndb_statistics(reference: Sequence[int], query: Sequence[int]) -> Dict[str, object]:
    """The statistics of DESIGN.md 4.15 from the bin counts of the reference set and of the query set, in host float64: per bin the
    two-proportion z value (0 where the pooled standard error is 0), `different` = the bins with |z| > NDB_Z, `ndb` = different / K,
    `jsd` = the Jensen-Shannon divergence of the two histograms (natural logarithm).  {"ndb", "jsd", "different", "z"}."""
    try:
        a, b = [operator.index(v) for v in reference], [operator.index(v) for v in query]
    except TypeError:
        raise ValueError("bin counts: integers expected") from None
    if len(a) != len(b) or len(a) < 1 or min(a + b) < 0:
        raise ValueError(f"two vectors of non-negative counts over the same bins expected, got {len(a)} and {len(b)} entries")
    n_a, n_b = sum(a), sum(b)
    if n_a < 1 or n_b < 1:
        raise ValueError(f"{n_a} reference and {n_b} query samples counted, at least one of each expected")
    z, jsd = [], 0.0
    for a_j, b_j in zip(a, b):
        big_p, big_q, p = a_j / n_a, b_j / n_b, (a_j + b_j) / (n_a + n_b)
        se = math.sqrt(p * (1.0 - p) * (1.0 / n_a + 1.0 / n_b))
        z.append((big_p - big_q) / se if se > 0.0 else 0.0)
        m = 0.5 * (big_p + big_q)
        if big_p > 0.0:
            jsd += 0.5 * big_p * math.log(big_p / m)
        if big_q > 0.0:
            jsd += 0.5 * big_q * math.log(big_q / m)
    different = sum(1 for v in z if abs(v) > NDB_Z)
    return {"ndb": different / len(a), "jsd": max(jsd, 0.0), "different": different, "z": z}


class KMeans:
    """Deterministic k-means (Lloyd) on squared L2 distances in pixel space: `bins` centroids, `iterations` rounds of assignment and
    update, then one final assignment; no early stop.  The initial centroids are the fed rows `init_ids` (distinct positions), or
    the first `bins` entries of torch.randperm(n) from a CPU generator seeded with `seed`.  Feeding keeps a device copy; fit()
    launches kernels only.  Distances go through nn_sqdist_tiled in row blocks of at most `block_bytes` (distance block plus kernel
    workspace); a pair's value depends on its two rows alone, ties go to the smaller bin, a centroid is a float64 sum over its
    members in ascending position: every output is the same bit for bit for any split of the feeds and any `block_bytes`.  The
    ORDER of the feeds is part of the input: it sets the positions, with them the initial centroids and the order of every sum."""

    def __init__(self, bins: int, iterations: int = 25, seed: int = 0, init_ids=None, block_bytes: int = 256 << 20) -> None:
        if not _is_int(bins) or not 2 <= bins <= km_ops.MAX_K:
            raise ValueError(f"bins in 2 .. {km_ops.MAX_K} expected, got {bins}")
        if not _is_int(iterations) or iterations < 1:
            raise ValueError(f"iterations >= 1 expected, got {iterations}")
        if not _is_int(seed):
            raise ValueError(f"an integer seed expected, got {seed}")
        if not _is_int(block_bytes) or block_bytes < 1:
            raise ValueError(f"block_bytes must be positive, got {block_bytes}")
        if init_ids is not None:
            init_ids = _id_list(init_ids, bins, "init_ids")
            if len(set(init_ids)) != bins or min(init_ids) < 0:
                raise ValueError(f"init_ids: {bins} distinct positions >= 0 expected")
        self.bins, self.iterations, self.seed, self.init_ids, self.block_bytes = bins, iterations, seed, init_ids, block_bytes
        self.shape = None
        self._fed, self._out = _RowStore("KMeans"), None

    def feed(self, batch: torch.Tensor) -> None:
        self.shape = self._fed.add(batch, "feed", self.shape)
        self._out = None

    def _assign(self, x: torch.Tensor, xn: torch.Tensor, c: torch.Tensor, labels: torch.Tensor, mind: torch.Tensor,
                changed: torch.Tensor) -> None:
        """labels, mind and the one-element changed of every row of x against the centroids c"""
        n, cn, step = x.shape[0], nn_ops.nn_sqnorm(c), _block_rows(self.block_bytes, self.bins, x.shape[1])
        if step >= n:
            km_ops.km_assign(nn_ops.nn_sqdist_tiled(x, c, xn, cn), labels, mind, changed)
            return
        part = torch.empty((n + step - 1) // step, dtype=torch.int64, device=x.device)
        for b, (lo, hi) in enumerate(_blocks(n, step)):
            km_ops.km_assign(nn_ops.nn_sqdist_tiled(x[lo:hi], c, xn[lo:hi], cn), labels[lo:hi], mind[lo:hi], part[b:b + 1])
        changed.copy_(part.sum().reshape(1))

    def fit(self) -> "KMeans":
        """everything from the initial centroids to the final assignment, as launches on the current stream; the host does not wait"""
        if self._out is not None:
            return self
        n, k = self._fed.n, self.bins
        if n < k:
            raise ValueError(f"{n} images fed, at least as many as the {k} bins expected")
        if n > km_ops.MAX_N:
            raise ValueError(f"{n} images fed, at most {km_ops.MAX_N} expected")
        ids = self.init_ids if self.init_ids is not None else \
            torch.randperm(n, generator=torch.Generator().manual_seed(self.seed))[:k].tolist()
        if max(ids) >= n:
            raise ValueError(f"init_ids: positions below the {n} images fed expected, got {max(ids)}")
        x = self._fed.rows()
        dev = x.device
        xn = nn_ops.nn_sqnorm(x)
        c = x.index_select(0, _ids_to(ids, dev)).contiguous()
        labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
        mind = torch.empty(n, dtype=torch.float64, device=dev)
        changed = torch.zeros(self.iterations + 1, dtype=torch.int64, device=dev)
        start = torch.empty(k + 1, dtype=torch.int32, device=dev)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        for t in range(self.iterations + 1):
            self._assign(x, xn, c, labels, mind, changed[t:t + 1])
            if t < self.iterations:
                km_ops.km_order(labels, k, start, order)
                km_ops.km_update(x, order, start, c)
        counts = km_ops.km_count(labels, torch.zeros(k, dtype=torch.int64, device=dev))
        self._out = dict(centroids=c, labels=labels, dist=mind, counts=counts, changed=changed)
        return self

    def _fitted(self, name: str) -> torch.Tensor:
        if self._out is None:
            if not self._fed.n:
                raise ValueError("no image fed yet")
            self.fit()
        return self._out[name]

    @property
    def centroids(self) -> torch.Tensor:
        """(bins, D) float32 on the device"""
        return self._fitted("centroids")

    @property
    def labels(self) -> torch.Tensor:
        """(n,) int32: the bin of every fed image, by position"""
        return self._fitted("labels")

    @property
    def counts(self) -> torch.Tensor:
        """(bins,) int64: the bin sizes of the fed images"""
        return self._fitted("counts")

    @property
    def changed(self) -> torch.Tensor:
        """(iterations + 1,) int64 on the device: the labels each assignment changed (the first one: all n); 0 from convergence on"""
        return self._fitted("changed")

    def assign(self, batch: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(labels (B,) int32, dist (B,) float64) of other images against the fitted centroids: the nearest bin (ties: the smaller
        bin) and the squared distance to its centroid"""
        if self.shape is None:
            raise ValueError("no image fed yet")
        _check_batch(batch, self.shape)
        rows = _rows(batch, "KMeans.assign")
        c, dev = self.centroids, rows.device
        labels = torch.full((rows.shape[0],), -1, dtype=torch.int32, device=dev)
        mind = torch.empty(rows.shape[0], dtype=torch.float64, device=dev)
        self._assign(rows, nn_ops.nn_sqnorm(rows), c, labels, mind, torch.empty(1, dtype=torch.int64, device=dev))
        return labels, mind


class NDB:
    """Number of statistically Different Bins and the Jensen-Shannon divergence between the bin histogram of the images `kmeans` was
    fitted on (the reference) and that of everything fed here.  feed() assigns a batch to its bins and adds to K counters on the
    device; the batch is not kept and the host does not wait.  Counts are integers, so the result is the same for any split."""

    KEYS = ("ndb", "jsd")

    def __init__(self, kmeans: KMeans) -> None:
        if not isinstance(kmeans, KMeans):
            raise ValueError(f"a KMeans expected, got {type(kmeans).__name__}")
        self.kmeans = kmeans
        self._count, self._fed = None, 0

    def feed(self, batch: torch.Tensor) -> None:
        labels, _ = self.kmeans.assign(batch)
        if self._count is None:
            self._count = torch.zeros(self.kmeans.bins, dtype=torch.int64, device=labels.device)
        km_ops.km_count(labels, self._count)
        self._fed += labels.shape[0]

    def per_bin(self) -> Dict[str, List]:
        """{"reference": the K bin counts of the fitted set, "query": those of the fed set, "z": the K z values}; the one copy of
        2 K integers to the host"""
        if not self._fed:
            raise ValueError("no image fed yet")
        a, b = torch.stack([self.kmeans.counts, self._count]).tolist()
        return {"reference": a, "query": b, "z": ndb_statistics(a, b)["z"]}

    def result(self) -> Dict[str, float]:
        per = self.per_bin()
        st = ndb_statistics(per["reference"], per["query"])
        return {"ndb": st["ndb"], "jsd": st["jsd"]}


# ------------------------------------------------------------------ log-mel feature space, Frechet distance
_MEL_RATE, _MEL_BINS = 44100.0, 512   # the codec's sample rate and the STFT bins an image row stands for (N_FFT / 2)


def mel_filterbank(rows: int, bands: int, f_min: float = 0.0, f_max: float = 22050.0):
    """Triangular HTK mel filters over the rows of a magnitude image, in host float64.  `rows`: a power of two in
    8 .. 512; with q = 512 // rows, row r stands for the STFT bins r q .. r q + q - 1 and has the frequency
    f_r = (r q + (q - 1) / 2) * 44100 / 1024 Hz.  The bands + 2 points p are equally spaced on the mel scale
    2595 log10(1 + f / 700) between f_min and f_max, and
        w[m, r] = max(0, min((f_r - p_m) / (p_{m+1} - p_m), (p_{m+2} - f_r) / (p_{m+2} - p_{m+1})))
    which is torchaudio.functional.melscale_fbanks(norm=None, mel_scale="htk") evaluated at those frequencies.  Returns (weight
    float32 (bands, rows), lo int32 (bands,), hi int32 (bands,)) on the host: [lo, hi) is the tightest row range that holds a
    band's non-zero weights.  A band without a non-zero weight raises ValueError (too many bands for so few rows)."""
    if not _is_int(rows) or not 8 <= rows <= _MEL_BINS or rows & (rows - 1):
        raise ValueError(f"rows: a power of two in 8 .. {_MEL_BINS} expected, got {rows}")
    if not _is_int(bands) or bands < 1:
        raise ValueError(f"bands >= 1 expected, got {bands}")
    f_min, f_max = float(f_min), float(f_max)
    if not 0.0 <= f_min < f_max <= _MEL_RATE / 2:
        raise ValueError(f"0 <= f_min < f_max <= {_MEL_RATE / 2} expected, got {f_min}, {f_max}")
    q = _MEL_BINS // rows
    f = (torch.arange(rows, dtype=torch.float64) * q + (q - 1) / 2) * (_MEL_RATE / (2 * _MEL_BINS))
    mel = torch.linspace(2595.0 * math.log10(1.0 + f_min / 700.0), 2595.0 * math.log10(1.0 + f_max / 700.0), bands + 2,
                         dtype=torch.float64)
    p = 700.0 * (torch.pow(10.0, mel / 2595.0) - 1.0)
    up = (f[None, :] - p[:-2, None]) / (p[1:-1] - p[:-2])[:, None]
    down = (p[2:, None] - f[None, :]) / (p[2:] - p[1:-1])[:, None]
    w = torch.minimum(up, down).clamp_min(0.0).to(torch.float32)
    nonzero = w > 0
    empty = (~nonzero.any(1)).nonzero().reshape(-1).tolist()
    if empty:
        raise ValueError(f"{len(empty)} of {bands} mel bands hold no row of {rows} (the first: band {empty[0]}): fewer bands expected")
    first = nonzero.to(torch.int8).argmax(1)
    last = rows - 1 - nonzero.flip(1).to(torch.int8).argmax(1)
    return w.contiguous(), first.to(torch.int32), (last + 1).to(torch.int32)


class LogMel:
    """The log-mel spectrogram of what a (magnitude, phase-delta) image decodes to, pooled over time: the feature space of
    evaluate_mel.  Channel 0 is decoded as the codec does ((x + 1) / 2, bark un-scaling; with fewer than 512 rows
    a row's bark weight is the mean over the STFT bins it stands for), squared to power -- non-negative for any x, so generator
    outputs outside [-1, 1] are legal --, weighted by mel_filterbank(side_h, bands, f_min, f_max), and log(. + floor) is averaged
    over side_w / pools columns per pool.  Defaults: side_h // 8 bands, min(32, side_w // 8) pools.

    `floor` = 1e-6 is an unmeasured default: it sets how far below a band's usual power the logarithm still tells values apart (a
    full-scale band is near 1e-1 .. 1e1 here) and no corpus was used to choose it.

        rows = LogMel(512, 512)(batch)            # (B, 2, 512, 512) float32 cuda -> (B, 64 * 32) float32 cuda

    One launch of csrc/logmel.hip per call; a row depends on its image alone."""

    def __init__(self, side_h: int, side_w: int, bands: Optional[int] = None, pools: Optional[int] = None, f_min: float = 0.0,
                 f_max: float = 22050.0, floor: float = 1e-6) -> None:
        if not _is_int(side_h) or not _is_int(side_w) or side_h < 64 or side_w < 1:
            raise ValueError(f"side_h >= 64 and side_w >= 1 expected, got {side_h} x {side_w}")
        bands = side_h // 8 if bands is None else bands
        pools = min(32, max(1, side_w // 8)) if pools is None else pools
        if not _is_int(pools) or pools < 1 or side_w % pools:
            raise ValueError(f"a pool count that divides side_w = {side_w} expected, got {pools}")
        if not 0.0 < float(floor) < float("inf"):
            raise ValueError(f"a finite floor > 0 expected, got {floor}")
        self.weight, self.lo, self.hi = mel_filterbank(side_h, bands, f_min, f_max)
        from .audio.functions import _bark_vector   # the codec's own vector (importing it needs no device)
        bark = _bark_vector(_MEL_BINS, "cpu").double().view(side_h, _MEL_BINS // side_h).mean(1)
        self.scale = (1.0 / (2.0 * bark)).to(torch.float32).contiguous()
        self.side_h, self.side_w, self.bands, self.pools, self.floor = side_h, side_w, bands, pools, float(floor)
        self.dims = bands * pools
        self._dev = {}   # device -> (scale, weight) on it

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4 or tuple(x.shape[1:]) != (2, self.side_h, self.side_w) or x.shape[0] < 1:
            raise ValueError(f"a non-empty batch (B, 2, {self.side_h}, {self.side_w}) expected, got {tuple(x.shape)}")
        ops._chk_typed("LogMel", x)
        if x.device not in self._dev:
            self._dev[x.device] = (self.scale.to(x.device), self.weight.to(x.device))
        scale, weight = self._dev[x.device]
        return mel_ops.logmel_rows(x, 0, scale, weight, self.lo, self.hi, self.floor, self.pools)


class WaveLogMel:
    """The pooled log-mel rows of waveforms: LogMel's feature space taken from the sound instead of from an image's channel 0, so that
    the phase counts.  A waveform (B, L) at 44.1 kHz is framed as the codec frames it (1024 / 256, reflect padding,
    periodic Hann / sqrt(384)), |X|^2 is weighted by mel_filterbank(512, bands, f_min, f_max), and log(. + floor) is averaged over
    window / pools frames per pool, for every window of `window` frames at every `hop` frames (the tail is dropped).  Defaults: 64
    bands, 32 pools, windows of 512 frames every 512 -- what a 512 x 512 image spans; 130 816 samples are exactly one window.

    `floor` = 1e-6 is the same unmeasured default as LogMel's: no corpus was used to choose it.

        rows = WaveLogMel()(waves)                # (B, L) float32 cuda -> (B * W, 64 * 32) float32 cuda, W = (1 + L // 256 - 512) // 512 + 1

    Two launches of csrc/melspec.hip per call (mel power, then pooling); a row depends on its window's samples alone."""

    def __init__(self, bands: int = 64, pools: int = 32, window: int = 512, hop: int = 512, f_min: float = 0.0,
                 f_max: float = 22050.0, floor: float = 1e-6) -> None:
        for name, v in (("pools", pools), ("window", window), ("hop", hop)):
            if not _is_int(v) or v < 1:
                raise ValueError(f"{name}: an integer >= 1 expected, got {v!r}")
        if window % pools:
            raise ValueError(f"a pool count that divides window = {window} expected, got {pools}")
        if not 0.0 < float(floor) < float("inf"):
            raise ValueError(f"a finite floor > 0 expected, got {floor}")
        self.weight, self.lo, self.hi = mel_filterbank(_MEL_BINS, bands, f_min, f_max)
        self.bands, self.pools, self.window, self.hop, self.floor = bands, pools, window, hop, float(floor)
        self.dims = bands * pools
        self._dev = {}   # device -> weight on it

    def windows(self, length: int) -> int:
        """rows a waveform of `length` samples gives (0: shorter than one window)"""
        return mel_ops.pool_windows(mel_ops.mel_frames(length), self.window, self.hop)

    def power(self, waves: torch.Tensor) -> torch.Tensor:
        """(B, L) float32 cuda -> the mel power (B, bands, 1 + L // 256)"""
        if not isinstance(waves, torch.Tensor) or waves.dim() != 2 or waves.shape[0] < 1:
            raise ValueError(f"waveforms (B, L) expected, got {tuple(waves.shape) if isinstance(waves, torch.Tensor) else waves!r}")
        if self.windows(waves.shape[1]) < 1:
            raise ValueError(f"{waves.shape[1]} samples are fewer than one window of {self.window} frames "
                             f"({256 * (self.window - 1)} samples)")
        ops._chk_typed("WaveLogMel", waves)
        if waves.device not in self._dev:
            self._dev[waves.device] = self.weight.to(waves.device)
        return mel_ops.mel_power(waves, self._dev[waves.device], self.lo, self.hi)

    def pool(self, power: torch.Tensor) -> torch.Tensor:
        """the mel power (B, bands, T) of `power()` -> rows (B * W, bands * pools)"""
        return mel_ops.logmel_pool(power, self.window, self.hop, self.pools, self.floor)

    def __call__(self, waves: torch.Tensor) -> torch.Tensor:
        return self.pool(self.power(waves))


def _sym_f64(name: str, mean, cov) -> int:
    if not all(isinstance(t, torch.Tensor) and t.dtype == torch.float64 and not t.is_cuda for t in (mean, cov)):
        raise ValueError(f"frechet_distance: {name}: float64 host tensors expected")
    if mean.dim() != 1 or mean.shape[0] < 1 or tuple(cov.shape) != (mean.shape[0], mean.shape[0]):
        raise ValueError(f"frechet_distance: {name}: a mean (d,) and a covariance (d, d) expected, got {tuple(mean.shape)} and "
                         f"{tuple(cov.shape)}")
    return mean.shape[0]


def frechet_distance(mean1: torch.Tensor, cov1: torch.Tensor, mean2: torch.Tensor, cov2: torch.Tensor) -> float:
    """The Frechet distance between the Gaussians N(mean1, cov1) and N(mean2, cov2) (Dowson & Landau 1982; the formula of FID), in
    host float64: |mean1 - mean2|^2 + tr cov1 + tr cov2 - 2 sum sqrt(max(l, 0)) over the eigenvalues l of S cov2 S, where S is
    the positive-semidefinite square root of cov1 from torch.linalg.eigh with negative eigenvalues clamped to 0.  S cov2 S is
    symmetric and has the eigenvalues of cov1 cov2, so no square root of a non-symmetric matrix is taken; singular covariances
    (fewer rows than dimensions) are legal.  With cov1 = V diag(a) V^T, the eigenvalues of S cov2 S that are not zero by the rank of
    cov1 are those of the r x r matrix diag(sqrt a_r) V_r^T cov2 V_r diag(sqrt a_r) over the r eigenpairs with a > d eps max(a) (the
    numerical rank): that matrix is what is decomposed, so that the d - r known zeros are not computed as rounding noise, whose
    square root would be 1e-8 of the scale each.  Rounding can leave the result a few 1e-16 (tr cov1 + tr cov2) below 0 for
    covariances of full rank, and up to 1e-9 of it for singular ones."""
    d = _sym_f64("the first set", mean1, cov1)
    if d != _sym_f64("the second set", mean2, cov2):
        raise ValueError(f"frechet_distance: two sets of one dimension expected, got {mean1.shape[0]} and {mean2.shape[0]}")
    lam, vec = torch.linalg.eigh((cov1 + cov1.T) / 2)
    keep = lam > d * torch.finfo(torch.float64).eps * lam.max()          # none for a covariance that is not positive anywhere
    half = vec[:, keep] * lam[keep].sqrt()
    inner = half.T @ ((cov2 + cov2.T) / 2) @ half
    cross = torch.linalg.eigvalsh((inner + inner.T) / 2).clamp_min(0.0).sqrt().sum() if bool(keep.any()) else 0.0
    delta = mean1 - mean2
    return float(delta @ delta + torch.trace(cov1) + torch.trace(cov2) - 2.0 * cross)


class Frechet:
    """The Frechet distance between everything fed as real and everything fed as fake, in whatever space the rows are in (LogMel
    rows in evaluate_mel).  Feeding keeps a device copy; moments() runs mel_ops.moments over all rows of a set at once, so the
    result is the same bit for bit for any split of the feeds; result() copies the two means and covariances to the host and
    evaluates frechet_distance there.  At most 4096 numbers per row."""

    def __init__(self) -> None:
        self.shape = None
        self._real, self._fake = _RowStore("Frechet"), _RowStore("Frechet")
        self._moments = None

    def _feed(self, store: _RowStore, what: str, batch: torch.Tensor) -> None:
        self.shape = store.add(batch, what, self.shape)
        self._moments = None

    def feed_real(self, batch: torch.Tensor) -> None:
        self._feed(self._real, "feed_real", batch)

    def feed_fake(self, batch: torch.Tensor) -> None:
        self._feed(self._fake, "feed_fake", batch)

    def moments(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(mean_real (d,), cov_real (d, d), mean_fake, cov_fake): float64 on the device"""
        if min(self._real.n, self._fake.n) < 2:
            raise ValueError(f"{self._real.n} real and {self._fake.n} fake rows fed, at least 2 of each expected")
        if self._moments is None:
            self._moments = mel_ops.moments(self._real.rows()) + mel_ops.moments(self._fake.rows())
        return self._moments

    def result(self) -> float:
        return frechet_distance(*(t.cpu() for t in self.moments()))


# ------------------------------------------------------------------ kernel distance (KID)
def _kid_rows(x, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] < 2 or not 1 <= x.shape[1] <= kid_ops.MAX_D:
        raise ValueError(f"{what}: at least 2 rows (n, d) of 1 .. {kid_ops.MAX_D} numbers expected, got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else x!r}")
    return x


def _mmd2_sums(x: torch.Tensor, y: torch.Tensor, ix: Optional[torch.Tensor] = None, iy: Optional[torch.Tensor] = None):
    """three fused launches: the row sums of k over x x x and y x y without their diagonals and over y x x, per subset.  Returns
    ((subsets, 3) float64: their totals per subset, the y x y row sums, the y x x row sums), all on the device."""
    xx = kid_ops.polyk_rowsums(x, x, ix, ix, skip_diag=True)
    yy = kid_ops.polyk_rowsums(y, y, iy, iy, skip_diag=True)
    yx = kid_ops.polyk_rowsums(y, x, iy, ix)
    return torch.stack([xx.sum(1), yy.sum(1), yx.sum(1)], 1), yy, yx


def _mmd2(totals: Sequence[float], m: int, n: int) -> float:
    """the unbiased estimate from the three totals of a subset of m and n rows, in host float64"""
    sxx, syy, syx = totals
    return sxx / (m * (m - 1)) + syy / (n * (n - 1)) - 2.0 * syx / (m * n)


def poly_mmd2(x: torch.Tensor, y: torch.Tensor) -> float:
    """The unbiased estimate of the squared maximum mean discrepancy between the rows x (m, d) and y (n, d) (float32 cuda, m, n
    >= 2, d <= 4096) under k(a, b) = (a.b / d + 1)^3:
        sum_{i != j} k(x_i, x_j) / (m (m - 1)) + sum_{i != j} k(y_i, y_j) / (n (n - 1)) - 2 sum_{i, j} k(y_i, x_j) / (m n).
    It can be negative.  The rows are taken as they are (KID standardises them first).  Three kid_ops.polyk_rowsums launches, the
    float64 row sums are added on the device and read back once; the same bits in every run."""
    x, y = _kid_rows(x, "poly_mmd2"), _kid_rows(y, "poly_mmd2")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"poly_mmd2: rows of one length expected, got {x.shape[1]} and {y.shape[1]}")
    totals, _, _ = _mmd2_sums(x, y)
    return _mmd2(totals[0].tolist(), x.shape[0], y.shape[0])


def _kid_counts(subsets, subset_size, seed) -> None:
    for name, v, least, most in (("subsets", subsets, 1, kid_ops.MAX_SUBSETS), ("subset_size", subset_size, 2, kid_ops.MAX_ROWS)):
        if isinstance(v, bool) or not isinstance(v, int) or not least <= v <= most:
            raise ValueError(f"{name} in {least} .. {most} expected, got {v!r}")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"an integer seed expected, got {seed!r}")


def kid_subsets(x: torch.Tensor, y: torch.Tensor, subsets: int = 100, subset_size: int = 1000, seed: int = 0) -> Tuple[float, float]:
    """(mean, population standard deviation) of poly_mmd2 over `subsets` random subsets of m = min(subset_size, rows of x, rows of
    y) rows of each set (the protocol of Binkowski et al.).  Subset s takes the first m entries of a permutation of each set from
    one CPU generator seeded with `seed`: x's permutation of subset 0, y's of subset 0, x's of subset 1, ...  If m is the size of
    both sets the one subset there is is run, and the deviation is 0.0.  All subsets go through three batched launches."""
    x, y = _kid_rows(x, "kid_subsets"), _kid_rows(y, "kid_subsets")
    _kid_counts(subsets, subset_size, seed)
    m = min(subset_size, x.shape[0], y.shape[0])
    if m == x.shape[0] == y.shape[0]:
        return poly_mmd2(x, y), 0.0
    gen = torch.Generator().manual_seed(seed)
    ix, iy = [], []
    for _ in range(subsets):
        ix.append(torch.randperm(x.shape[0], generator=gen)[:m])
        iy.append(torch.randperm(y.shape[0], generator=gen)[:m])
    ix, iy = (torch.stack(lists).to(torch.int32).to(x.device) for lists in (ix, iy))
    totals, _, _ = _mmd2_sums(x, y, ix, iy)
    values = [_mmd2(row, m, m) for row in totals.tolist()]
    mean = math.fsum(values) / subsets
    return mean, math.sqrt(math.fsum((v - mean) ** 2 for v in values) / subsets)


class KID:
    """The Kernel Inception Distance between everything fed as real and everything fed as fake, in whatever space the rows are in
    (LogMel rows in evaluate_mel).  Feeding keeps a device copy.  result() standardises both sets by the real rows' float64 mean
    and standard deviation (mel_ops.moments; a column without variance becomes 0) -- without that the polynomial kernel sees
    little but the common offset of log-mel rows -- and returns `kid` / `kid_std`, the mean and population standard deviation of
    the unbiased estimate over `subsets` random subsets of min(subset_size, n_real, n_fake) rows (kid_subsets), and `kid_full`,
    the estimate on the whole sets.  per_sample(): the witness function at every generated row.  Every sum is float64 in a fixed
    order and the rows of a set are concatenated before anything is launched: every output is the same bit for bit for any split
    and interleaving of the feeds.  At most 4096 numbers per row."""

    KEYS = ("kid", "kid_std", "kid_full")

    def __init__(self, subsets: int = 100, subset_size: int = 1000, seed: int = 0) -> None:
        _kid_counts(subsets, subset_size, seed)
        self.subsets, self.subset_size, self.seed, self.shape = subsets, subset_size, seed, None
        self._real, self._fake = _RowStore("KID"), _RowStore("KID")
        self._rows = self._full = None

    def _feed(self, store: _RowStore, what: str, batch: torch.Tensor) -> None:
        self.shape = store.add(batch, what, self.shape)
        self._rows = self._full = None

    def feed_real(self, batch: torch.Tensor) -> None:
        self._feed(self._real, "feed_real", batch)

    def feed_fake(self, batch: torch.Tensor) -> None:
        self._feed(self._fake, "feed_fake", batch)

    def standardised(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(real (n_real, d), fake (n_fake, d)) float32 on the device: the rows the kernel sees"""
        if min(self._real.n, self._fake.n) < 2:
            raise ValueError(f"{self._real.n} real and {self._fake.n} fake rows fed, at least 2 of each expected")
        if self._rows is None:
            real, fake = self._real.rows(), self._fake.rows()
            if real.shape[1] > kid_ops.MAX_D:
                raise ValueError(f"KID: at most {kid_ops.MAX_D} numbers per row, got {real.shape[1]}")
            mean, cov = mel_ops.moments(real)
            sd = cov.diagonal().sqrt().contiguous()
            self._rows = kid_ops.standardise_rows(real, mean, sd), kid_ops.standardise_rows(fake, mean, sd)
        return self._rows

    def _whole(self):
        if self._full is None:
            real, fake = self.standardised()
            totals, yy, yx = _mmd2_sums(real, fake)
            self._full = _mmd2(totals[0].tolist(), real.shape[0], fake.shape[0]), yy[0], yx[0]
        return self._full

    def per_sample(self) -> torch.Tensor:
        """(n_fake,) float64 on the device: for every generated row y_i the witness function of the two whole sets,
        mean_j k(y_i, x_j) - mean_{j != i} k(y_i, y_j): positive where the data is denser around y_i than the samples are.  The
        smallest values name the samples least like the data."""
        _, yy, yx = self._whole()
        return yx / self._real.n - yy / (self._fake.n - 1)

    def result(self) -> Dict[str, float]:
        real, fake = self.standardised()
        full = self._whole()[0]
        if min(self.subset_size, real.shape[0], fake.shape[0]) == real.shape[0] == fake.shape[0]:
            return {"kid": full, "kid_std": 0.0, "kid_full": full}    # the one subset there is: the whole sets
        kid, std = kid_subsets(real, fake, self.subsets, self.subset_size, self.seed)
        return {"kid": kid, "kid_std": std, "kid_full": full}


# ------------------------------------------------------------------ perceptual path length (PPL)
def ppl_trim(values: Sequence[float]) -> Tuple[float, float]:
    """(lo, hi) of the StyleGAN protocol for the finite-count list `values`: the elements of rank floor(0.01 (n - 1)) and
    ceil(0.99 (n - 1)) of the sorted list -- numpy.percentile(values, 1, 'lower') and numpy.percentile(values, 99, 'higher'), in
    integer arithmetic"""
    ordered, last = sorted(values), len(values) - 1
    return ordered[last // 100], ordered[-((-99 * last) // 100)]


class PPL:
    """The perceptual path length of a generator (Karras et al. 2019) in whatever space `rows_of` maps latents to (the log-mel rows
    of the generated images in path_length).  For pair i: z0_i, z1_i ~ N(0, I) of shape (rand_channels, 2, 2) and
    t_i ~ U[0, 1) (`sampling` "full") or t_i = 0 ("end"), za_i = slerp(z0_i, z1_i, t_i), zb_i = slerp(z0_i, z1_i, t_i + epsilon)
    (ppl_ops.slerp_pairs: project.slerp's definition), and with D the row length
        d_i = |rows_of(za_i) - rows_of(zb_i)|^2 / (D epsilon^2)                     (ppl_ops.rows_sqdist, float64).
    `rows_of(latents (B, rand_channels, 2, 2) float32 cuda) -> (B, D) float32 cuda` is any callable.  It is always called with 16
    latents (the last call: the rest), za_i and zb_i next to each other: a generator's kernels are chosen by the batch size, and
    the two images of a pair must come from the same launches.

    `feed(n_pairs)` only counts: z0, z1 and t are one draw each, of all pairs fed, from one device generator seeded with `seed`, so
    the draws need the total and every launch waits for per_pair() / result().  Any split of the feeds gives the same bits.

    result(): `ppl` = the mean of the d_i with lo <= d_i <= hi (ppl_trim), `ppl_mean` = the mean of all d_i, and with "full"
    sampling `ppl_chord` = the mean of |rows_of(z0_i) - rows_of(z1_i)|^2 / D and `ppl_ratio` = ppl_mean / ppl_chord, which is >= 1
    in expectation and 1 for straight paths of constant speed in row space (NaN when ppl_chord is 0); `ppl_pairs` = the pairs
    used: a pair whose ends are antipodal (an angle within 1e-6 of pi) has no single shortest arc and is left out of every mean.
    All values reach the host in one copy; the means are math.fsum(kept) / count there: exactly rounded, whatever the order."""

    PAIRS_PER_CALL = 8   # 16 images per call of rows_of

    def __init__(self, rows_of, epsilon: float = 1e-4, sampling: str = "full", seed: int = 0, *, rand_channels: int) -> None:
        if not callable(rows_of):
            raise ValueError(f"rows_of: a callable (B, C, 2, 2) -> (B, D) expected, got {rows_of!r}")
        if not _is_int(rand_channels) or rand_channels < 1:
            raise ValueError(f"rand_channels >= 1 expected, got {rand_channels!r}")
        if isinstance(epsilon, bool) or not isinstance(epsilon, (int, float)) or not 0.0 < epsilon <= 0.1:
            raise ValueError(f"epsilon in (0, 0.1] expected, got {epsilon!r}")
        if sampling not in ("full", "end"):
            raise ValueError(f"sampling: \"full\" or \"end\" expected, got {sampling!r}")
        if not _is_int(seed):
            raise ValueError(f"an integer seed expected, got {seed!r}")
        self.rows_of, self.rand_channels, self.epsilon, self.sampling, self.seed = rows_of, rand_channels, float(epsilon), sampling, seed
        self.pairs, self.dims, self._values = 0, None, None

    def feed(self, n_pairs: int) -> None:
        if not _is_int(n_pairs) or n_pairs < 1:
            raise ValueError(f"feed: a number of pairs >= 1 expected, got {n_pairs!r}")
        self.pairs += n_pairs
        self._values = None

    def _distances(self, first: torch.Tensor, second: torch.Tensor, scale_of) -> torch.Tensor:
        """(n,) float64: scale_of(D) |rows_of(first_i) - rows_of(second_i)|^2, the two latents of a pair adjacent in their call"""
        n, per = first.shape[0], self.PAIRS_PER_CALL
        a = b = None
        for lo in range(0, n, per):
            hi = min(lo + per, n)
            latents = torch.stack([first[lo:hi], second[lo:hi]], 1).reshape(2 * (hi - lo), self.rand_channels, 2, 2)
            rows = self.rows_of(latents.contiguous())
            if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[0] != 2 * (hi - lo) or rows.shape[1] < 1:
                raise ValueError(f"PPL: rows_of: rows ({2 * (hi - lo)}, D) expected, got "
                                 f"{tuple(rows.shape) if isinstance(rows, torch.Tensor) else rows!r}")
            if a is None:
                self.dims = int(rows.shape[1])
                a = torch.empty((n, self.dims), dtype=torch.float32, device=rows.device)
                b = torch.empty((n, self.dims), dtype=torch.float32, device=rows.device)
            elif rows.shape[1] != self.dims:
                raise ValueError(f"PPL: rows_of: rows of {self.dims} numbers expected, got {rows.shape[1]}")
            pairs = rows.view(hi - lo, 2, self.dims)
            a[lo:hi].copy_(pairs[:, 0])
            b[lo:hi].copy_(pairs[:, 1])
        return ppl_ops.rows_sqdist(a, b, scale_of(self.dims))

    def _run(self):
        if self._values is None:
            if self.pairs < 1:
                raise ValueError("PPL: no pairs fed")
            n, d = self.pairs, self.rand_channels * 4
            device = torch.device("cuda", torch.cuda.current_device())
            rng = torch.Generator(device=device).manual_seed(self.seed)
            z0 = torch.randn(n, d, device=device, generator=rng)
            z1 = torch.randn(n, d, device=device, generator=rng)
            if self.sampling == "full":
                t = torch.rand(n, dtype=torch.float64, device=device, generator=rng)
            else:
                t = torch.zeros(n, dtype=torch.float64, device=device)
            za, zb, flag = ppl_ops.slerp_pairs(z0, z1, t, self.epsilon)
            step = self._distances(za, zb, lambda dims: 1.0 / (dims * self.epsilon * self.epsilon))
            chord = self._distances(z0, z1, lambda dims: 1.0 / dims) if self.sampling == "full" else None
            self._values = step, chord, flag
        return self._values

    def per_pair(self) -> torch.Tensor:
        """(pairs,) float64 on the device: d_i, NaN for a pair that is left out"""
        step, _, flag = self._run()
        return torch.where(flag != 0, torch.full_like(step, float("nan")), step)

    def per_pair_chord(self) -> Optional[torch.Tensor]:
        """(pairs,) float64 on the device: |rows_of(z0_i) - rows_of(z1_i)|^2 / D, NaN for a pair that is left out; None with "end"
        sampling"""
        _, chord, flag = self._run()
        return None if chord is None else torch.where(flag != 0, torch.full_like(chord, float("nan")), chord)

    def flags(self) -> torch.Tensor:
        """(pairs,) int32 on the device: 1 for a pair that is left out (antipodal ends)"""
        return self._run()[2]

    def result(self) -> Dict[str, float]:
        step, chord, flag = self._run()
        columns = [step, flag.to(torch.float64)] + ([chord] if chord is not None else [])
        host = torch.stack(columns).cpu().tolist()   # the one copy
        return ppl_aggregate(host[0], host[1], host[2] if chord is not None else None)


def ppl_aggregate(step: Sequence[float], flag: Sequence[float], chord: Optional[Sequence[float]] = None) -> Dict[str, float]:
    """PPL.result()'s keys from the per-pair values on the host (float64 lists; flag != 0: the pair is left out)"""
    kept = [v for v, f in zip(step, flag) if not f]
    if not kept:
        raise ValueError("PPL: every pair was left out (antipodal ends)")
    lo, hi = ppl_trim(kept)
    inner = [v for v in kept if lo <= v <= hi]
    result = {"ppl": math.fsum(inner) / len(inner) if inner else float("nan"), "ppl_mean": math.fsum(kept) / len(kept)}
    if chord is not None:
        result["ppl_chord"] = math.fsum(v for v, f in zip(chord, flag) if not f) / len(kept)
        result["ppl_ratio"] = result["ppl_mean"] / result["ppl_chord"] if result["ppl_chord"] > 0.0 else float("nan")
    result["ppl_pairs"] = len(kept)
    return result

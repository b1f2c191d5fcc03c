"""The sliced Wasserstein distance between patches of Laplacian-pyramid levels (Karras et al., ICLR 2018) restated on the CPU with
plain torch operators, in float64 (the yardstick of test_swd_gpu.py) or float32 (to measure float32's own error).  Centres and
directions are arguments, so the GPU code and this helper can be handed the very same draws.  Definition: DESIGN.md."""
import torch
import torch.nn.functional as F

K5 = [1.0, 4.0, 6.0, 4.0, 1.0]
U = 2.0 ** -24


def _g(dtype):
    k = torch.tensor(K5, dtype=dtype) / 16
    return torch.outer(k, k)


def _filter(x, g):
    c = x.shape[1]
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), g[None, None].repeat(c, 1, 1, 1), groups=c)


def down(x):
    return _filter(x, _g(x.dtype))[:, :, ::2, ::2]


def up(x):
    z = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3], dtype=x.dtype)
    z[:, :, ::2, ::2] = x
    return _filter(z, 4 * _g(x.dtype))


def pyramid(x, levels):
    out, g = [], x
    for _ in range(levels - 1):
        nxt = down(g)
        out.append(g - up(nxt))
        g = nxt
    return out + [g]


def reconstruct(levels):
    x = levels[-1]
    for lap in reversed(levels[:-1]):
        x = lap + up(x)
    return x


def descriptors(level, centres, patch=7):
    """(N, C, H, W), (N, P, 2) -> raw (N P, C patch^2), channel-major"""
    n, c = level.shape[:2]
    h = patch // 2
    o = torch.arange(-h, h + 1)
    cen = centres.long()
    y = cen[:, :, 0, None, None, None] + o[None, None, None, :, None]   # N P 1 p 1
    x = cen[:, :, 1, None, None, None] + o[None, None, None, None, :]   # N P 1 1 p
    d = level[torch.arange(n)[:, None, None, None, None], torch.arange(c)[None, None, :, None, None], y, x]  # N P C p p
    return d.reshape(n * cen.shape[1], c * patch * patch)


def channel_stats(desc, channels):
    """population mean and standard deviation per channel: (C,), (C,)"""
    d = desc.reshape(desc.shape[0], channels, -1)
    return d.mean((0, 2)), d.std((0, 2), unbiased=False)


def normalise(desc, channels):
    mean, std = channel_stats(desc, channels)
    d = desc.reshape(desc.shape[0], channels, -1)
    return ((d - mean[None, :, None]) / std[None, :, None]).reshape(desc.shape)


def sliced_distance(a, b, directions):
    """step 4 for one repeat on descriptors that are already normalised (or not, for the closed-form tests): mean over all
    entries of |sort(a d^T) - sort(b d^T)|, every column sorted ascending"""
    pa = (a @ directions.to(a.dtype).T).sort(0).values
    pb = (b @ directions.to(b.dtype).T).sort(0).values
    return (pa - pb).abs().mean()


def swd(images_a, images_b, draws, patch=7, dtype=torch.float64):
    """draws = [(centres_a, centres_b, directions (R, D, K))] per level, finest first -> ({side: swd x 1000, "avg": ..},
    [per level: the two normalised descriptor sets], for the error bounds of the tests)"""
    c = images_a.shape[1]
    pa, pb = pyramid(images_a.to(dtype), len(draws)), pyramid(images_b.to(dtype), len(draws))
    out, sets = {}, []
    for la, lb, (ca, cb, dirs) in zip(pa, pb, draws):
        da, db = normalise(descriptors(la, ca, patch), c), normalise(descriptors(lb, cb, patch), c)
        vals = [sliced_distance(da, db, dirs[r]) for r in range(dirs.shape[0])]
        out[str(min(la.shape[2:]))] = float(torch.stack(vals).double().mean() * 1000.0)
        sets.append((da, db))
    out["avg"] = sum(out.values()) / len(out)
    return out, sets


def projection_bound(a_norm, directions):
    """textbook bound of a float32 dot product of length K in any order, (K + 2) u / (1 - (K + 2) u) * sum |a_i d_i|, per entry:
    (M, D); a_norm (M, K) and directions (D, K) as float64 copies of the float32 operands"""
    k = a_norm.shape[1]
    gamma = (k + 2) * U / (1 - (k + 2) * U)
    return gamma * (a_norm.abs().double() @ directions.abs().double().T)


def smooth_noise(n, c, h, w, passes, gen):
    """tanh of binomially smoothed white noise: `passes` sets the correlation length, i.e. the distribution"""
    x = torch.randn(n, c, h, w, generator=gen, dtype=torch.float64)
    for _ in range(passes):
        x = _filter(x, _g(torch.float64))
    return torch.tanh(2 * x * (2.0 ** passes)).float()

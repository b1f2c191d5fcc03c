"""The float64 definition of the kernel distance of musicgan_amd.metrics (Binkowski et al., "Demystifying MMD GANs",
ICLR 2018), the derived error bound of the GPU evaluation, and the inputs the tests use.  Nothing here needs a GPU.

    z_ij = float32((float64(x_ij) - mean_j) / sd_j), 0 in a column whose sd is 0 or not finite
    k(x, y) = (x.y / d + 1)^3
    mmd2 = sum_{i != j} k(x_i, x_j) / (m (m - 1)) + sum_{i != j} k(y_i, y_j) / (n (n - 1)) - 2 sum_{i, j} k(x_i, y_j) / (m n)

The GPU's only float32 arithmetic is the dot product inside a chunk of 256 components (tests/nn_ref.py: a chain of fused
multiply-adds from zero, |error| <= gamma_c sum |x_c y_c| for any order); the chunks are added and everything else is done in
float64.  With gamma = nn_ref.gamma(d, 256) and delta = gamma sum_c |x_c y_c| / d the device's u' = x.y / d + 1 is within delta of
u, and |u'^3 - u^3| = |u' - u| |u'^2 + u' u + u^2| <= 3 (|u| + delta)^2 delta.  A float64 sum of N terms in any order is within
(N - 1) 2^-53 (1 + ...) of the sum of absolute values; the cube and the final weights add a few roundings more: (N + 16) 2^-53
covers them."""
import torch

from nn_ref import U64, gamma

CHUNK = 256


def standardise(x: torch.Tensor, mean: torch.Tensor, sd: torch.Tensor) -> torch.Tensor:
    """float32 rows from float32 rows and float64 moments, every step as the definition states it"""
    z = ((x.double() - mean.double()) / sd.double()).float()
    z[:, ~(torch.isfinite(sd) & (sd != 0))] = 0.0
    return z


def kernel(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """(m, n) float64"""
    u = x.double() @ y.double().T / x.shape[1] + 1.0
    return u * u * u


def kernel_f32_chunks(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """the device's arithmetic in torch CPU operators: float32 dot products over chunks of 256, the rest in float64"""
    dot = torch.zeros(x.shape[0], y.shape[0], dtype=torch.float64)
    for lo in range(0, x.shape[1], CHUNK):
        dot += (x[:, lo:lo + CHUNK].float() @ y[:, lo:lo + CHUNK].float().T).double()
    u = dot / x.shape[1] + 1.0
    return u * u * u


def kernel_bound(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """(m, n) float64: the derived bound of every kernel value"""
    d = x.shape[1]
    delta = gamma(d, CHUNK) * (x.double().abs() @ y.double().abs().T) / d
    u = x.double() @ y.double().T / d + 1.0
    return 3.0 * (u.abs() + delta) ** 2 * delta


def _off_diagonal(k: torch.Tensor, skip_diag: bool) -> torch.Tensor:
    if skip_diag:
        k = k.clone()
        k.fill_diagonal_(0.0)
    return k


def rowsums(a: torch.Tensor, b: torch.Tensor, ia=None, ib=None, skip_diag: bool = False, kernel_fn=kernel) -> torch.Tensor:
    """(subsets, ma) float64: out[s, i] = sum_j k(a[ia[s, i]], b[ib[s, j]]), without j = i if skip_diag; ia, ib: lists of lists of
    row numbers, None = all rows in their order"""
    subsets = len(ia) if ia is not None else len(ib) if ib is not None else 1
    out = []
    for s in range(subsets):
        rows = a if ia is None else a[torch.as_tensor(ia[s], dtype=torch.long)]
        cols = b if ib is None else b[torch.as_tensor(ib[s], dtype=torch.long)]
        out.append(_off_diagonal(kernel_fn(rows, cols), skip_diag).sum(1))
    return torch.stack(out)


def rowsums_bound(a: torch.Tensor, b: torch.Tensor, ia=None, ib=None, skip_diag: bool = False) -> torch.Tensor:
    """(subsets, ma) float64: the bound of every row sum"""
    slack = lambda rows, cols: (cols.shape[0] + 16) * U64 * kernel(rows, cols).abs()   # noqa: E731
    return rowsums(a, b, ia, ib, skip_diag, kernel_fn=lambda r, c: kernel_bound(r, c) + slack(r, c))


def mmd2(x: torch.Tensor, y: torch.Tensor, kernel_fn=kernel) -> float:
    m, n = x.shape[0], y.shape[0]
    xx = _off_diagonal(kernel_fn(x, x), True).sum()
    yy = _off_diagonal(kernel_fn(y, y), True).sum()
    return float(xx / (m * (m - 1)) + yy / (n * (n - 1)) - 2.0 * kernel_fn(x, y).sum() / (m * n))


def mmd2_bound(x: torch.Tensor, y: torch.Tensor) -> float:
    """the same weighted sum of the kernel bounds, plus (number of terms + 16) 2^-53 times the weighted sum of absolute values"""
    m, n = x.shape[0], y.shape[0]
    terms = m * (m - 1) + n * (n - 1) + m * n
    total = 0.0
    for p, q, skip, weight in ((x, x, True, 1.0 / (m * (m - 1))), (y, y, True, 1.0 / (n * (n - 1))), (x, y, False, 2.0 / (m * n))):
        both = kernel_bound(p, q) + (terms + 16) * U64 * kernel(p, q).abs()
        total += weight * float(_off_diagonal(both, skip).sum())
    return total


def witness(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """(n,) float64: mean_j k(y_i, x_j) - mean_{j != i} k(y_i, y_j)"""
    return kernel(y, x).sum(1) / x.shape[0] - _off_diagonal(kernel(y, y), True).sum(1) / (y.shape[0] - 1)


def witness_bound(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return rowsums_bound(y, x)[0] / x.shape[0] + rowsums_bound(y, y, skip_diag=True)[0] / (y.shape[0] - 1)


def gaussian(n: int, d: int, seed: int, shift: float = 0.0) -> torch.Tensor:
    """n rows of d independent standard normal numbers + shift, float32"""
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed)) + shift


def logmel_like(n: int, d: int, seed: int, shift: float = 0.0) -> torch.Tensor:
    """rows like log-mel rows: a common offset of -8 .. -13 per column, column scales of 0.1 .. 1.1, float32; `shift` in units of
    the column scale"""
    gen = torch.Generator().manual_seed(1000 + d)
    offset, scale = -8.0 - 5.0 * torch.rand(d, generator=gen), 0.1 + torch.rand(d, generator=gen)
    return (torch.randn(n, d, generator=torch.Generator().manual_seed(seed)) + shift) * scale + offset


def moments(x: torch.Tensor):
    """(mean, sd) float64 of float32 rows: two passes, the unbiased variance"""
    x = x.double()
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).sum(0).div(x.shape[0] - 1).sqrt()

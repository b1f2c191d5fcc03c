"""Float64 numpy restatements of DESIGN.md 4.19, the yardsticks of test_logmel_cpu.py and test_logmel_gpu.py: the HTK mel filterbank
over image rows (written from the formula, not from musicgan_amd.metrics), the log-mel rows, the two-pass moments with the
quantities their error bounds need, and the Frechet distance through scipy.linalg.sqrtm.  No GPU, no musicgan_amd import."""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53


def gamma(k: int, u: float) -> float:
    return k * u / (1.0 - k * u)


def row_frequencies(rows: int) -> np.ndarray:
    q = 512 // rows
    return np.array([(r * q + (q - 1) / 2.0) * 44100.0 / 1024.0 for r in range(rows)])


def filterbank(rows: int, bands: int, f_min: float = 0.0, f_max: float = 22050.0):
    """(w float64 (bands, rows), lo, hi, empty bands): element by element from the formula"""
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)  # noqa: E731
    m_lo, m_hi = mel(f_min), mel(f_max)
    p = [700.0 * (10.0 ** ((m_lo + (m_hi - m_lo) * i / (bands + 1)) / 2595.0) - 1.0) for i in range(bands + 2)]
    f = row_frequencies(rows)
    w = np.zeros((bands, rows))
    for m in range(bands):
        for r in range(rows):
            w[m, r] = max(0.0, min((f[r] - p[m]) / (p[m + 1] - p[m]), (p[m + 2] - f[r]) / (p[m + 2] - p[m + 1])))
    lo, hi, empty = [], [], 0
    for m in range(bands):
        nz = np.nonzero(w[m].astype(np.float32))[0]
        if nz.size == 0:
            empty += 1
            lo.append(0)
            hi.append(0)
        else:
            lo.append(int(nz[0]))
            hi.append(int(nz[-1]) + 1)
    return w, lo, hi, empty


def logmel(x, c, scale, weight, lo, hi, floor, pools):
    """x (N, C, H, W), scale (H,), weight (M, H) as float32 arrays -> (N, M * pools) float64: the definition with every operation
    in float64 (the float32 inputs taken exactly)"""
    x, scale, weight = (np.asarray(a, dtype=np.float64) for a in (x, scale, weight))
    n, _, h, w = x.shape
    m_ = weight.shape[0]
    p = (x[:, c] * scale[None, :, None] + scale[None, :, None]) ** 2           # (N, H, W)
    out = np.empty((n, m_, pools))
    for m in range(m_):
        s = np.einsum("h,nhw->nw", weight[m, lo[m]:hi[m]], p[:, lo[m]:hi[m]]) if hi[m] > lo[m] else np.zeros((n, w))
        out[:, m] = np.log(s + floor).reshape(n, pools, w // pools).mean(2)
    return out.reshape(n, m_ * pools)


def logmel_f32(x, c, scale, weight, lo, hi, floor, pools):
    """the same definition in the kernel's own precisions (float32 up to s, ascending h, product and sum rounded apart; float64 from
    the logarithm on): what a correct float32 evaluation gives, for the margin against the bound"""
    x, scale, weight = (np.asarray(a, dtype=np.float32) for a in (x, scale, weight))
    n, _, h, w = x.shape
    m_ = weight.shape[0]
    t = x[:, c] * scale[None, :, None]
    t = t + scale[None, :, None]
    p = t * t
    out = np.empty((n, m_, pools))
    for m in range(m_):
        s = np.zeros((n, w), dtype=np.float32)
        for r in range(lo[m], hi[m]):
            s = s + weight[m, r] * p[:, r]
        out[:, m] = np.log(s.astype(np.float64) + floor).reshape(n, pools, w // pools).mean(2)
    return out.reshape(n, m_ * pools)


def logmel_bound(ref, lo, hi):
    """|out - ref| <= 1.01 gamma_k + u |ref| + 1e-12 with k = 2 K + 4, K the longest band (the issue's derivation: every term of s
    is non-negative, so its float32 evaluation is within gamma_k relatively, fused or not; the logarithm makes that an absolute
    gamma_k s / (s + floor) <= gamma_k, which the mean keeps; u |ref| is the final rounding)"""
    k = 2 * max(b - a for a, b in zip(lo, hi)) + 4
    return 1.01 * gamma(k, U32) + U32 * np.abs(ref) + 1e-12


def moments(x):
    """x (n, d) float32 -> (mean, cov, bound on the mean, bound on cov): two passes in float64 and
    2 gamma64_{n+6} sum_i |x_ij - mean_j| |x_ik - mean_k| / (n - 1) + 1e-300 (the factor 2: this restatement rounds too)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mean = x.sum(0) / n
    c = x - mean[None, :]
    cov = c.T @ c / (n - 1)
    g = 2.0 * gamma(n + 6, U64)
    return mean, cov, g * np.abs(x).sum(0) / n + 1e-300, g * (np.abs(c).T @ np.abs(c)) / (n - 1) + 1e-300


def frechet(mean1, cov1, mean2, cov2) -> float:
    """|dmu|^2 + tr C1 + tr C2 - 2 tr sqrtm(C1 C2): the textbook form, as FID implementations evaluate it"""
    from scipy.linalg import sqrtm
    mean1, cov1, mean2, cov2 = (np.asarray(a, dtype=np.float64) for a in (mean1, cov1, mean2, cov2))
    root = sqrtm(cov1 @ cov2)
    d = mean1 - mean2
    return float(d @ d + np.trace(cov1) + np.trace(cov2) - 2.0 * np.trace(root).real)


def frechet_diagonal(mean1, a, mean2, b) -> float:
    """closed form for diagonal covariances diag(a), diag(b)"""
    d = np.asarray(mean1, dtype=np.float64) - np.asarray(mean2, dtype=np.float64)
    return float(d @ d + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum())

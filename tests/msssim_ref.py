"""MS-SSIM between pairs of images ("Evaluation: MS-SSIM sample diversity") restated on the CPU with plain torch
operators, in float64 (the yardstick of test_msssim_gpu.py) or float32 (to measure float32's own error), and an a-priori bound
of the rounding error of ANY float32 evaluation of that definition, evaluated in float64 on the data (`term_bounds`).

The bound, with u = 2^-24 and gamma(k) = k u / (1 - k u).  Every elementary float32 operation is correctly rounded (relative
error <= u; so is the division the kernels are compiled with).  Hats are computed values, plain letters exact ones.

  inputs    At scale 0 both evaluations read the same float32 pixels: e_a = e_b = 0.  The 2 x 2 mean is three additions and an
            exact scaling, so the next scale's pixels carry  e_a' = pool(e_a) + gamma(3) pool(|a| + e_a).
  filter    The separable window has positive taps.  A value passes one multiplication and at most ten additions per pass in
            any order (fewer roundings with fused multiply-adds), so  |^filt(^x) - filt(x)| <= filt(e_x) + gamma(22) filt(|x| + e_x).
            For x = a this is E_mu_a; for the products ^p = fl(^a ^b), e_p = |a| e_b + |b| e_a + e_a e_b + u (|a| + e_a)(|b| + e_b).
  sigma     ^s_ab = fl(^filt(^p) - fl(^mu_a ^mu_b)):  E_s = (E_filt(ab) + E_mumu)(1 + u) + u |s_ab|, with
            E_mumu = |mu_a| E_mu_b + |mu_b| E_mu_a + E_mu_a E_mu_b + u (|mu_a| + E_mu_a)(|mu_b| + E_mu_b).  This is the dominant part:
            E_filt and E_mumu are of the size 22 u filt(|ab|) whatever is left of s after the cancellation, and cs divides them by
            s_aa + s_bb + C2, which is as small as C2 = 0.0036 on flat patches.
  quotient  N = 2 s_ab + C2, D = s_aa + s_bb + C2 (C2 itself rounded to float32):  E_N = (2 E_s_ab + u C2)(1 + u) + u |N|,
            E_D = ((E_s_aa + E_s_bb)(1 + u) + u |s_aa + s_bb| + u C2)(1 + u) + u |D|, and
            |^N / ^D - N / D| <= (E_N + |N / D| E_D) / (D - E_D), times (1 + u) plus u |N / D| for the division itself.  D >= C2 > E_D
            is asserted.  The luminance factor is the same expression in mu_a mu_b, mu_a^2 + mu_b^2 and C1.
  ssim      E_ssim = (|cs| E_l + |l| E_cs + E_cs E_l)(1 + u) + u |ssim|.
  means     The error of a mean is at most the mean of the errors; the float64 accumulation adds 1e-15.
`value_bounds` carries the term bounds through the weighted product: t -> t^w has the derivative w t^(w-1), largest at the lower
end t - E of the interval (w < 1), and the other factors are at most max(1, t + E)^w; 1e-12 covers the float64 powers."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
C1, C2 = (0.01 * 2) ** 2, (0.03 * 2) ** 2
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WIN, SIGMA = 11, 1.5


def gamma(k):
    return k * U / (1 - k * U)


def window(dtype=torch.float64):
    """the 11 taps: float64, divided by their sum, rounded to float32 (returned as `dtype`, the values are float32 numbers)"""
    d = torch.arange(WIN, dtype=torch.float64) - WIN // 2
    g = torch.exp(-(d * d) / (2 * SIGMA * SIGMA))
    return (g / g.sum()).float().to(dtype)


def scales(h, w):
    if min(h, w) < WIN:
        raise ValueError(f"{h} x {w} is smaller than the window")
    s = 1
    while s < 5 and h % (1 << s) == 0 and w % (1 << s) == 0 and min(h, w) // (1 << s) >= WIN:
        s += 1
    return s


def weights(s):
    w = torch.tensor(WEIGHTS[:s], dtype=torch.float64)
    return w / w.sum()


def filt(x, g):
    """'valid' separable filtering of (N, C, H, W): rows, then columns"""
    c = x.shape[1]
    x = F.conv2d(x, g.to(x.dtype).reshape(1, 1, 1, WIN).repeat(c, 1, 1, 1), groups=c)
    return F.conv2d(x, g.to(x.dtype).reshape(1, 1, WIN, 1).repeat(c, 1, 1, 1), groups=c)


def maps(a, b):
    """per-pixel (cs, ssim) of one scale, in the dtype of a and b"""
    g = window(a.dtype)
    c1, c2 = (torch.tensor(v, dtype=torch.float64).to(a.dtype) for v in (C1, C2))   # rounded once to the working precision
    mua, mub = filt(a, g), filt(b, g)
    saa, sbb, sab = filt(a * a, g) - mua * mua, filt(b * b, g) - mub * mub, filt(a * b, g) - mua * mub
    cs = (2 * sab + c2) / (saa + sbb + c2)
    return cs, cs * ((2 * (mua * mub) + c1) / (mua * mua + mub * mub + c1))


def terms(a, b, dtype=torch.float64):
    """(n, S) float64: the CS means of the scales 0 .. S-2 and the SSIM mean of the last, before the clamp; the per-pixel values in
    `dtype`, the means accumulated in float64"""
    a, b = a.to(dtype), b.to(dtype)
    s = scales(a.shape[2], a.shape[3])
    out = []
    for i in range(s):
        cs, ss = maps(a, b)
        out.append((ss if i == s - 1 else cs).double().mean((1, 2, 3)))
        if i < s - 1:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    return torch.stack(out, 1)


def combine(t):
    """(n, S) terms -> (n,) MS-SSIM: clamp at 0, weighted product, float64"""
    return (t.double().clamp_min(0) ** weights(t.shape[1])[None]).prod(1)


def ms_ssim(a, b, dtype=torch.float64):
    return combine(terms(a, b, dtype))


def _quotient(num, e_num, den, e_den):
    assert bool((den - e_den > 0).all()), "the denominator's error bound reaches the denominator"
    q = num / den
    return (e_num + q.abs() * e_den) / (den - e_den) * (1 + U) + U * q.abs()


def term_bounds(a, b):
    """(n, S) float64: the bound of the module docstring for |float32 evaluation - float64 definition| of every term"""
    a, b = a.double(), b.double()
    s = scales(a.shape[2], a.shape[3])
    g = window(torch.float64)
    g22, g3 = gamma(22), gamma(3)
    ea, eb = torch.zeros_like(a), torch.zeros_like(b)
    out = []
    for i in range(s):
        ua, ub = a.abs() + ea, b.abs() + eb                       # |^a| <= ua
        mua, mub = filt(a, g), filt(b, g)
        e_mua, e_mub = filt(ea, g) + g22 * filt(ua, g), filt(eb, g) + g22 * filt(ub, g)
        ma, mb = mua.abs() + e_mua, mub.abs() + e_mub

        def e_filt_prod(x, ex, ux, y, ey, uy):
            e_p = x.abs() * ey + y.abs() * ex + ex * ey + U * ux * uy
            return filt(e_p, g) + g22 * filt(ux * uy * (1 + U), g)

        def e_mumu(mx, emx, bx, my, emy, by):
            return mx.abs() * emy + my.abs() * emx + emx * emy + U * bx * by

        saa, sbb, sab = filt(a * a, g) - mua * mua, filt(b * b, g) - mub * mub, filt(a * b, g) - mua * mub
        e_maa, e_mbb, e_mab = e_mumu(mua, e_mua, ma, mua, e_mua, ma), e_mumu(mub, e_mub, mb, mub, e_mub, mb), \
            e_mumu(mua, e_mua, ma, mub, e_mub, mb)
        e_saa = (e_filt_prod(a, ea, ua, a, ea, ua) + e_maa) * (1 + U) + U * saa.abs()
        e_sbb = (e_filt_prod(b, eb, ub, b, eb, ub) + e_mbb) * (1 + U) + U * sbb.abs()
        e_sab = (e_filt_prod(a, ea, ua, b, eb, ub) + e_mab) * (1 + U) + U * sab.abs()
        num, den = 2 * sab + C2, saa + sbb + C2
        e_num = (2 * e_sab + U * C2) * (1 + U) + U * num.abs()
        e_den = ((e_saa + e_sbb) * (1 + U) + U * (saa + sbb).abs() + U * C2) * (1 + U) + U * den.abs()
        cs, e_cs = num / den, _quotient(num, e_num, den, e_den)
        if i < s - 1:
            out.append(e_cs.mean((1, 2, 3)) + 1e-15)
            ea, eb = F.avg_pool2d(ea, 2) + g3 * F.avg_pool2d(ua, 2), F.avg_pool2d(eb, 2) + g3 * F.avg_pool2d(ub, 2)
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
            continue
        lnum, lden = 2 * mua * mub + C1, mua * mua + mub * mub + C1
        e_lnum = (2 * e_mab + U * C1) * (1 + U) + U * lnum.abs()
        e_lden = ((e_maa + e_mbb) * (1 + U) + U * (mua * mua + mub * mub) + U * C1) * (1 + U) + U * lden.abs()
        lum, e_l = lnum / lden, _quotient(lnum, e_lnum, lden, e_lden)
        e_ss = (cs.abs() * e_l + lum.abs() * e_cs + e_cs * e_l) * (1 + U) + U * (cs * lum).abs()
        out.append(e_ss.mean((1, 2, 3)) + 1e-15)
    return torch.stack(out, 1)


def value_bounds(t, e):
    """(n,) float64: the bound of |float32 MS-SSIM - float64 MS-SSIM| from the float64 terms t (n, S), all > their bounds e (n, S)"""
    assert bool((t - e > 0).all()), "a term within its bound of the clamp: the product's derivative is unbounded there"
    w = weights(t.shape[1])[None]
    others = (torch.maximum(t + e, torch.ones_like(t)) ** w).prod(1, keepdim=True)
    return (w * e * (t - e) ** (w - 1) * others).sum(1) + 1e-12


def pairs(shape, rho, gen):
    """the test inputs: a = smooth noise of correlation length 2, b = clamp(rho a + (1 - rho) smooth noise of length 1)"""
    import swd_ref
    a = swd_ref.smooth_noise(*shape, 2, gen)
    b = (rho * a + (1 - rho) * swd_ref.smooth_noise(*shape, 1, gen)).clamp(-1, 1)
    return a, b

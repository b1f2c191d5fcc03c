"""DiffAugment as DESIGN.md 4.13 defines it, restated for the tests (a helper, not a test): numpy `decode` / `fwd` / `bwd`, a float64
torch version autograd can differentiate, and the two updates of the training step with T in them, built from oracle.progan's pieces.

An image batch x is (N, C, H, W) float32, H = frequency, W = time; u is (N, 8) float32 in [0, 1), columns 6 and 7 reserved.  A policy
is a subset of {translation = 1, cutout = 2} (a bit mask, `ops`) and a probability p in [0, 1].  Per sample n, all channels alike:

  translation on iff ops & 1 and u[n,0] < p (float32 compare);  ry = floor(H/8 + 0.5), rx = floor(W/8 + 0.5);
      dy = min(floor(u[n,1] * (2 ry + 1)), 2 ry) - ry, dx likewise from u[n,2] (the product rounded once to float32);
      S x[i, j] = x[i - dy, j - dx] inside the image, +0.0 outside.
  cutout on iff ops & 2 and u[n,3] < p;  ch = floor(H/2 + 0.5), cw = floor(W/2 + 0.5);
      oy = min(floor(u[n,4] * (H + 1 - ch % 2)), H - ch % 2), ox likewise from u[n,5];
      rows [oy - ch//2, oy - ch//2 + ch) & [0, H) x the like columns become +0.0.
  T x = M . S x (translation first);  T^t g = S^t (M . g), i.e. (M . g)[i + dy, j + dx] inside the image, +0.0 outside.

Every output element is a copy of one input element or +0.0, chosen by a select, never a product."""
import numpy as np
import torch

TRANSLATION, CUTOUT = 1, 2


def _bin(u, bins):
    """min(floor(u * bins), bins - 1) with the product in float32"""
    t = (np.asarray(u, dtype=np.float32) * np.float32(bins)).astype(np.float32)
    return np.minimum(np.floor(t).astype(np.int64), bins - 1)


def decode(u, h, w, ops, p):
    """u (N, 8) -> (N, 6) int32 rows of dy, dx, y0, y1, x0, x1 (an empty box, all 0, when cutout is off)"""
    u = np.asarray(u, dtype=np.float32).reshape(-1, 8)
    p = np.float32(p)
    out = np.zeros((u.shape[0], 6), dtype=np.int32)
    ry, rx = int(np.floor(h / 8 + 0.5)), int(np.floor(w / 8 + 0.5))
    ch, cw = int(np.floor(h / 2 + 0.5)), int(np.floor(w / 2 + 0.5))
    t_on = (u[:, 0] < p) & bool(ops & TRANSLATION)
    c_on = (u[:, 3] < p) & bool(ops & CUTOUT)
    out[:, 0] = np.where(t_on, _bin(u[:, 1], 2 * ry + 1) - ry, 0)
    out[:, 1] = np.where(t_on, _bin(u[:, 2], 2 * rx + 1) - rx, 0)
    oy, ox = _bin(u[:, 4], h + 1 - ch % 2), _bin(u[:, 5], w + 1 - cw % 2)
    out[:, 2] = np.where(c_on, np.clip(oy - ch // 2, 0, h), 0)
    out[:, 3] = np.where(c_on, np.clip(oy - ch // 2 + ch, 0, h), 0)
    out[:, 4] = np.where(c_on, np.clip(ox - cw // 2, 0, w), 0)
    out[:, 5] = np.where(c_on, np.clip(ox - cw // 2 + cw, 0, w), 0)
    return out


def _gather(h, w, prm, adjoint):
    """per sample: source row / column of every output element and whether it is kept (else +0.0)"""
    dy, dx, y0, y1, x0, x1 = (int(v) for v in prm)
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if adjoint:
        si, sj = i + dy, j + dx   # gx[i, j] = (M . gy)[i + dy, j + dx]: the box is tested at the source
        bi, bj = si, sj
    else:
        si, sj = i - dy, j - dx   # y[i, j] = M[i, j] ? x[i - dy, j - dx]: the box is tested at the destination
        bi, bj = i, j
    keep = (si >= 0) & (si < h) & (sj >= 0) & (sj < w) & ~((bi >= y0) & (bi < y1) & (bj >= x0) & (bj < x1))
    return np.clip(si, 0, h - 1), np.clip(sj, 0, w - 1), keep


def _apply_np(x, u, ops, p, adjoint):
    x = np.asarray(x)
    n, c, h, w = x.shape
    prm = decode(u, h, w, ops, p)
    out = np.zeros_like(x)   # +0.0
    for k in range(n):
        si, sj, keep = _gather(h, w, prm[k], adjoint)
        out[k] = np.where(keep[None], x[k][:, si, sj], x.dtype.type(0))
    return out


def fwd(x, u, ops, p):
    return _apply_np(x, u, ops, p, False)


def bwd(gy, u, ops, p):
    return _apply_np(gy, u, ops, p, True)


def fwd_torch(x: torch.Tensor, u, ops, p) -> torch.Tensor:
    """T x on a CPU tensor of any float dtype, differentiable with respect to x: a gather and torch.where"""
    n, c, h, w = x.shape
    prm = decode(np.asarray(u), h, w, ops, p)
    outs = []
    for k in range(n):
        si, sj, keep = _gather(h, w, prm[k], False)
        picked = x[k][:, torch.from_numpy(si), torch.from_numpy(sj)]
        outs.append(torch.where(torch.from_numpy(keep)[None], picked, torch.zeros((), dtype=x.dtype)))
    return torch.stack(outs)


def d_step_aug(gs, ds, x_real, z, eps, alpha, u, ops, p, dtype=torch.float64):
    """oracle.progan.d_step(detach_fake=True) with T on both batches: u rows [0, N) for the real batch, [N, 2N) for the fake one; the
    penalty is taken on the interpolation of the two augmented batches."""
    from oracle import progan as O
    n = x_real.shape[0]
    u = np.asarray(u, dtype=np.float32)
    gp_, dp_ = O._leafs(gs, dtype), O._leafs(ds, dtype)
    x_real, z, eps = x_real.to(dtype), z.to(dtype), eps.to(dtype)
    x_fake = O.gen_forward(gp_, gs.curr_layer, gs.has_last, z, alpha).detach()
    x_real, x_fake = fwd_torch(x_real, u[:n], ops, p), fwd_torch(x_fake, u[n:], ops, p)
    out_real = O.disc_forward(dp_, ds.curr_layer, ds.has_last, x_real, alpha)
    out_fake = O.disc_forward(dp_, ds.curr_layer, ds.has_last, x_fake, alpha)
    d_loss = O.w_disc_loss(out_real, out_fake)
    gp = O.gradient_penalty(dp_, ds.curr_layer, ds.has_last, x_real, x_fake, alpha, eps)
    (d_loss + gp).backward()
    return {"x_real_aug": x_real.detach(), "x_fake_aug": x_fake.detach(), "out_real": out_real.detach(),
            "out_fake": out_fake.detach(), "disc_loss": d_loss.detach(), "grad_pen": gp.detach(),
            "d_grads": {k: dp_[k].grad.detach() for k in ds.live_keys()}}


def g_step_aug(gs, ds, z, alpha, u, ops, p, dtype=torch.float64):
    """oracle.progan.g_step with D(T(G(z))): the generator's gradient comes back through T (autograd differentiates the gather)"""
    from oracle import progan as O
    gp_, dp_ = O._leafs(gs, dtype), O._leafs(ds, dtype)
    x_fake = O.gen_forward(gp_, gs.curr_layer, gs.has_last, z.to(dtype), alpha)
    out_fake = O.disc_forward(dp_, ds.curr_layer, ds.has_last, fwd_torch(x_fake, np.asarray(u, dtype=np.float32), ops, p), alpha)
    loss = O.w_gen_loss(out_fake)
    loss.backward()
    return {"out_fake": out_fake.detach(), "gen_loss": loss.detach(), "g_grads": {k: gp_[k].grad.detach() for k in gs.live_keys()}}

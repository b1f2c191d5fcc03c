"""DiffAugment on the GPU (csrc/diffaug.hip, musicgan_amd/aug_ops.py, networks.DiffAugment, ProGANStepper(augment=...), train(augment=...))
against the definition restated in tests/diffaug_ref.py: the two kernels bit for bit, the autograd wrapper, graph capture with u
rewritten between replays, both updates of the stepper against the float64 oracle with T in it, and a resumed augmented run."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import diffaug_ref as R
from golden_util import build_oracle_states, grad_atol, load, maxabs_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUBSETS = (R.TRANSLATION, R.CUTOUT, R.TRANSLATION | R.CUTOUT)
PS = (0.0, 0.5, 1.0)
GUARD = 64           # floats on either side of a destination: 256 bytes, so the guard keeps the 16-byte alignment
SENTINEL = 0x7fc0dead  # a quiet NaN with a payload of its own


def bits(t):
    """int32 view: -0.0 != +0.0, and a NaN equals only the same NaN"""
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t).view(np.int32)
    return t.detach().contiguous().cpu().numpy().view(np.int32)


def exhaustive_u(size):
    """one row per (dy, dx) x (cutout centre row, column) of a size x size image: bin k of `bins` is hit by (k + 0.5) / bins.  The two
    on/off columns alternate 0.25 / 0.75 so that p = 0.5 switches each transform on for half of the rows (p = 1: for all)."""
    r, c = int(np.floor(size / 8 + 0.5)), int(np.floor(size / 2 + 0.5))
    tb, cb = 2 * r + 1, size + 1 - c % 2
    rows = list(itertools.product(range(tb), range(tb), range(cb), range(cb)))
    u = np.zeros((len(rows), 8), dtype=np.float32)
    for i, (a, b, cy, cx) in enumerate(rows):
        u[i] = [0.25 + 0.5 * (i & 1), (a + 0.5) / tb, (b + 0.5) / tb, 0.25 + 0.5 * ((i >> 1) & 1), (cy + 0.5) / cb, (cx + 0.5) / cb,
                0.123, 0.987]
    return u


def random_u(n, seed):
    return np.random.default_rng(seed).random((n, 8), dtype=np.float32)


def images(shape, seed):
    """normal numbers with -0.0, +0.0 and a denormal sprinkled in: a copy keeps them, a product with a 0 / 1 mask would not"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape, dtype=np.float32)
    flat = x.reshape(-1)
    idx = rng.permutation(flat.size)[:max(3, flat.size // 16)]
    flat[idx[0::3]] = np.float32(-0.0)
    flat[idx[1::3]] = np.float32(0.0)
    flat[idx[2::3]] = np.float32(1e-42)
    return x


def run_embedded(fn, x_np, u_dev, ops, p, misalign):
    """fn(x, u, ops, p, out=) with the destination inside a sentinel-filled buffer and pre-filled with another NaN; `misalign`: source
    and destination are views one float past a 16-byte boundary.  Returns the destination's bits (an int32 tensor on the device)
    after checking the guards."""
    n = x_np.size
    off = 1 if misalign else 0
    src = torch.empty(n + 4, dtype=torch.float32, device=DEV)[off:off + n].view(x_np.shape)
    src.copy_(torch.from_numpy(x_np))
    buf = torch.full((n + 2 * GUARD + 4,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    dst = buf[GUARD + off:GUARD + off + n].view(x_np.shape)
    dst.fill_(float("nan"))
    assert (src.data_ptr() % 16 == 4 * off) and (dst.data_ptr() % 16 == 4 * off)
    out = fn(src, u_dev, ops, p, out=dst)
    assert out is dst
    whole = buf.view(torch.int32)
    lo, hi = whole[:GUARD + off], whole[GUARD + off + n:]
    assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), "bytes outside the destination changed"
    return whole[GUARD + off:GUARD + off + n].reshape(x_np.shape)   # (on the device: compared there, brought back only to report)


SHAPES = {
    "exhaustive4": ((225, 2, 4, 4), lambda: exhaustive_u(4)),
    "exhaustive8": ((729, 2, 8, 8), lambda: exhaustive_u(8)),
    "tail5x7": ((5, 1, 5, 7), lambda: random_u(5, 1)),
    "tail31x33": ((4, 3, 31, 33), lambda: random_u(4, 2)),
    "row1x9": ((3, 2, 1, 9), lambda: random_u(3, 3)),
    "vec64": ((2, 2, 64, 64), lambda: random_u(2, 4)),
    "level7": ((6, 2, 512, 512), lambda: random_u(6, 5)),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_fwd_and_bwd_are_bit_exact(name):
    from musicgan_amd import aug_ops
    shape, make_u = SHAPES[name]
    u = make_u()
    assert u.shape == (shape[0], 8)
    if name.startswith("exhaustive"):  # every (dy, dx) x every box of the plane is there at p = 1
        prm = R.decode(u, shape[2], shape[3], 3, 1.0)
        assert len({tuple(r) for r in prm[:, :2]}) == 9 and len(np.unique(prm, axis=0)) == shape[0]
        assert prm[:, 2].min() == 0 and prm[:, 3].max() == shape[2] and prm[:, 4].min() == 0 and prm[:, 5].max() == shape[3]
        assert (prm[:, 3] - prm[:, 2]).min() < (shape[2] + 1) // 2 and (prm[:, 5] - prm[:, 4]).min() < (shape[3] + 1) // 2
    x, g = images(shape, 11), images(shape, 12)
    u_dev = torch.from_numpy(u).to(DEV)
    for ops, p in itertools.product(SUBSETS, PS):
        for fn, ref_fn, data in ((aug_ops.diffaug_fwd, R.fwd, x), (aug_ops.diffaug_bwd, R.bwd, g)):
            ref = bits(ref_fn(data, u, ops, p))          # computed once, shared by the aligned and the misaligned call
            if p == 0.0:
                assert np.array_equal(ref, bits(data))   # the identity, bit for bit
            ref_dev = torch.from_numpy(ref).to(DEV)
            for misalign in (False, True):
                got = run_embedded(fn, data, u_dev, ops, p, misalign)
                if not torch.equal(got, ref_dev):
                    bad = np.argwhere(got.cpu().numpy() != ref)
                    raise AssertionError((name, fn.__name__, ops, p, misalign, len(bad), bad[:4].tolist()))
    torch.cuda.synchronize()


def test_default_output_and_argument_checks():
    from musicgan_amd import aug_ops
    from musicgan_amd._lib import MusicGanHipError
    x, u = images((3, 2, 8, 8), 1), random_u(3, 6)
    xd, ud = torch.from_numpy(x).to(DEV), torch.from_numpy(u).to(DEV)
    assert np.array_equal(bits(aug_ops.diffaug_fwd(xd, ud, 3, 1.0)), bits(R.fwd(x, u, 3, 1.0)))
    assert np.array_equal(bits(aug_ops.diffaug_bwd(xd, ud, 3, 1.0)), bits(R.bwd(x, u, 3, 1.0)))
    with pytest.raises(ValueError):
        aug_ops.diffaug_fwd(xd, ud[:2], 3, 1.0)
    with pytest.raises(ValueError):
        aug_ops.diffaug_fwd(xd, ud, 4, 1.0)
    with pytest.raises(ValueError):
        aug_ops.diffaug_fwd(xd, ud, 3, 1.5)
    with pytest.raises(ValueError):
        aug_ops.diffaug_fwd(xd[0], ud[:1], 3, 1.0)
    with pytest.raises(MusicGanHipError):
        aug_ops.diffaug_fwd(xd.double(), ud, 3, 1.0)
    with pytest.raises(MusicGanHipError):
        aug_ops.diffaug_fwd(xd.transpose(2, 3), ud, 3, 1.0)
    with pytest.raises(MusicGanHipError):
        aug_ops.diffaug_fwd(xd, ud.cpu(), 3, 1.0)


@pytest.mark.parametrize("adjoint", [False, True])
def test_nan_and_inf_under_the_mask_and_past_the_border_never_reach_the_output(adjoint):
    """NaN, +inf and -inf planted on exactly the source elements the transform drops: the output is finite everywhere and +0.0 wherever
    nothing is kept"""
    from musicgan_amd import aug_ops
    shape = (81, 2, 8, 8)
    u = exhaustive_u(8)[np.arange(81) * 9 + np.arange(81) % 9].copy()
    u[:, 0] = u[:, 3] = 0.0   # both transforms on for every row
    prm = R.decode(u, 8, 8, 3, 1.0)
    x = np.random.default_rng(3).standard_normal(shape, dtype=np.float32)
    poison = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    kept_any = np.zeros(shape, dtype=bool)
    for k in range(shape[0]):
        si, sj, keep = R._gather(8, 8, prm[k], adjoint)
        used = np.zeros((8, 8), dtype=bool)
        used[si[keep], sj[keep]] = True
        kept_any[k] = keep[None]
        n_bad = int((~used).sum())
        assert n_bad > 0
        x[k][:, ~used] = np.resize(poison, n_bad)[None]
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    fn, ref_fn = (aug_ops.diffaug_bwd, R.bwd) if adjoint else (aug_ops.diffaug_fwd, R.fwd)
    ref = ref_fn(x, u, 3, 1.0)
    assert np.isfinite(ref).all()
    for misalign in (False, True):
        got = run_embedded(fn, x, torch.from_numpy(u).to(DEV), 3, 1.0, misalign).cpu().numpy()
        assert np.array_equal(got, bits(ref))
        assert np.isfinite(got.view(np.float32)).all() and (got[~kept_any] == 0).all()


def test_overlapping_source_and_destination_are_refused_before_any_launch():
    from musicgan_amd import aug_ops
    from musicgan_amd._lib import MusicGanHipError
    shape = (4, 2, 8, 8)
    n = int(np.prod(shape))
    u = torch.from_numpy(random_u(4, 7)).to(DEV)
    for fn in (aug_ops.diffaug_fwd, aug_ops.diffaug_bwd):
        for shift in (0, 1, n // 2, n - 1):
            buf = torch.arange(2 * n, dtype=torch.float32, device=DEV)
            before = buf.clone()
            with pytest.raises(MusicGanHipError, match="overlap"):
                fn(buf[:n].view(shape), u, 3, 1.0, out=buf[shift:shift + n].view(shape))
            with pytest.raises(MusicGanHipError, match="overlap"):
                fn(buf[shift:shift + n].view(shape), u, 3, 1.0, out=buf[:n].view(shape))
            torch.cuda.synchronize()
            assert torch.equal(buf, before), "something was launched"
        out = fn(buf[:n].view(shape), u, 3, 1.0, out=buf[n:].view(shape))   # adjacent, not overlapping: accepted
        assert out.data_ptr() == buf[n:].data_ptr()


def test_diffaugment_backward_is_the_adjoint_kernel_and_differentiates_once():
    from musicgan_amd import aug_ops
    from musicgan_amd.networks import DiffAugment
    aug = DiffAugment("translation,cutout", 0.5)
    shape = (16, 2, 16, 16)
    gen = torch.Generator(device=DEV).manual_seed(5)
    u = aug.draw(16, DEV, generator=gen)
    assert tuple(u.shape) == (16, 8) and u.dtype == torch.float32 and u.is_cuda and bool(((u >= 0) & (u < 1)).all())
    into = torch.empty(16, 8, device=DEV)
    assert aug.draw(16, DEV, generator=torch.Generator(device=DEV).manual_seed(5), out=into) is into and torch.equal(into, u)
    x = torch.from_numpy(images(shape, 21)).to(DEV).requires_grad_(True)
    g = torch.from_numpy(images(shape, 22)).to(DEV)
    y = aug(x, u)
    assert np.array_equal(bits(y), bits(R.fwd(x.detach().cpu().numpy(), u.cpu().numpy(), 3, 0.5)))
    y.backward(g)
    assert np.array_equal(bits(x.grad), bits(aug_ops.diffaug_bwd(g, u, 3, 0.5)))
    assert np.array_equal(bits(x.grad), bits(R.bwd(g.cpu().numpy(), u.cpu().numpy(), 3, 0.5)))
    # the adjoint identity on the device, exact on integer-valued data
    xi = torch.randint(-8, 9, shape, device=DEV, generator=gen).float()
    gi = torch.randint(-8, 9, shape, device=DEV, generator=gen).float()
    lhs = (aug_ops.diffaug_fwd(xi, u, 3, 0.5).double() * gi.double()).sum()
    rhs = (xi.double() * aug_ops.diffaug_bwd(gi, u, 3, 0.5).double()).sum()
    assert float(lhs) == float(rhs)
    # a second differentiation raises
    g2 = g.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(aug(x, u), x, g2, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_one_captured_graph_follows_u():
    """fwd and bwd captured in one graph; the static u is rewritten between replays and every replay equals the eager call with that u"""
    from musicgan_amd import aug_ops
    shape = (8, 2, 32, 32)
    xs = torch.from_numpy(images(shape, 31)).to(DEV)
    gs = torch.from_numpy(images(shape, 32)).to(DEV)
    us = torch.from_numpy(random_u(8, 40)).to(DEV)
    ys, gxs = torch.empty_like(xs), torch.empty_like(gs)
    aug_ops.diffaug_fwd(xs, us, 3, 0.5, out=ys)   # (the library is loaded and warm before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        aug_ops.diffaug_fwd(xs, us, 3, 0.5, out=ys)
        aug_ops.diffaug_bwd(gs, us, 3, 0.5, out=gxs)
    seen = set()
    for seed in (41, 42, 43):
        u = random_u(8, seed)
        us.copy_(torch.from_numpy(u))
        ys.fill_(float("nan"))
        gxs.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(ys), bits(aug_ops.diffaug_fwd(xs, us, 3, 0.5))), seed
        assert np.array_equal(bits(gxs), bits(aug_ops.diffaug_bwd(gs, us, 3, 0.5))), seed
        assert np.array_equal(bits(ys), bits(R.fwd(xs.cpu().numpy(), u, 3, 0.5)))
        assert np.array_equal(bits(gxs), bits(R.bwd(gs.cpu().numpy(), u, 3, 0.5)))
        seen.add(bits(ys).tobytes())
    assert len(seen) == 3


# ----------------------------------------------------------------------------------------------------------------- stepper
CASES = ["l2_rc16_gpnorm1", "l3_rc32_fade"]
OPS_ALL, P_ON = 3, 1.0


def build_modules(g):
    from musicgan_amd.networks import Discriminator, Generator
    torch.manual_seed(int(g["seed"]))
    gen = Generator(int(g["rand_channels"]), end_layer=int(g["g_end_layer"]))
    disc = Discriminator(start_layer=int(g["d_start_layer"]))
    for _ in range(int(g["n_grow"])):
        gen.next_layer()
        disc.next_layer()
    ws = float(g["wscale"])
    if ws != 1.0:
        with torch.no_grad():
            for net in (gen, disc):
                for k, p in net.named_parameters():
                    if k.endswith("weight"):
                        p.mul_(ws)
    return gen.to(DEV), disc.to(DEV)


def build_stepper(g, augment, fused=True, stub=True, noise=None):
    from musicgan_amd.optim import FusedAdam
    from musicgan_amd.train_step import ProGANStepper
    gen, disc = build_modules(g)
    og = FusedAdam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9))
    od = FusedAdam(disc.parameters(), lr=1e-3, betas=(0.0, 0.9))
    if stub:  # keep the gradients observable: no update
        og.step = od.step = lambda *a, **k: None
    return ProGANStepper(gen, disc, og, od, int(g["rand_channels"]), fused_d_step=fused, noise=noise, augment=augment), gen, disc


KINK_MARGIN = 4 * 2.0 ** -24   # of a layer's largest pre-activation: four float32 roundings of a number of that size


def kink_distance(fn):
    """the smallest |pre-activation| / (largest |pre-activation| of the same tensor) over every LeakyReLU that `fn()` evaluates in the
    oracle"""
    import torch.nn.functional as F
    orig, worst = F.leaky_relu, [float("inf")]

    def spy(t, *a, **k):
        d = t.detach().abs()
        worst[0] = min(worst[0], float(d.min() / d.max().clamp_min(1e-300)))
        return orig(t, *a, **k)
    F.leaky_relu = spy
    try:
        fn()
    finally:
        F.leaky_relu = orig
    return worst[0]


@functools.lru_cache(maxsize=None)
def well_posed_u(case):
    """The random numbers of a case: (3N, 8) from numpy's generator at the first seed from 1234 on at which the comparison with a
    float64 oracle is well posed.  LeakyReLU has a kink at 0: where the oracle's pre-activation is closer to 0 than float32 can
    resolve at the size of the numbers it is summed from, a float32 evaluation lands on either side depending on its order of
    summation, both are right, and the gradients of the two differ by 0.8 of that element's whole contribution -- no float32 code,
    the plain-PyTorch evaluation included, can be held to the float64 gradient there.  So such inputs are not used: every
    pre-activation of both float64 oracle updates (critic: real, fake and interpolated batch; generator update: both networks) must
    keep KINK_MARGIN of its tensor's largest value from 0.  The rule reads the float64 oracle alone, never the code under test.
    (Seed 1234 fails it for l2_rc16_gpnorm1: one pre-activation of block 6 on the augmented fake batch is 4.8e-7 at a scale of
    10.9, 4.4e-8 of it.)"""
    g = load(f"progan_{case}.npz")
    gs, ds = build_oracle_states(g)
    n, alpha = g["x_real"].shape[0], float(g["alpha"])
    x_real, z, z2, eps = (torch.from_numpy(g[k]) for k in ("x_real", "z", "z2", "eps"))
    for seed in range(1234, 1234 + 64):
        u = np.random.default_rng(seed).random((3 * n, 8), dtype=np.float32)

        def both():
            R.d_step_aug(gs, ds, x_real, z, eps, alpha, u[:2 * n], OPS_ALL, P_ON, dtype=torch.float64)
            R.g_step_aug(gs, ds, z2, alpha, u[2 * n:], OPS_ALL, P_ON, dtype=torch.float64)
        if kink_distance(both) >= KINK_MARGIN:
            return seed, u
    raise AssertionError(f"{case}: no seed in 1234 .. 1297 keeps the oracle's pre-activations off the LeakyReLU kink")


def case_inputs(g, case):
    n = g["x_real"].shape[0]
    _, u = well_posed_u(case)
    return dict(alpha=float(g["alpha"]), n=n, x_real=torch.from_numpy(g["x_real"]), z=torch.from_numpy(g["z"]),
                z2=torch.from_numpy(g["z2"]), eps=torch.from_numpy(g["eps"]), u_d=u[:2 * n], u_g=u[2 * n:])


def grads_of(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def both_updates(st, gen, disc, c, with_u):
    """one critic and one generator update with everything injected -> (losses, critic gradients, generator gradients)"""
    dev = lambda t: (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)
    kw_d = {"u": dev(c["u_d"])} if with_u else {}
    kw_g = {"u": dev(c["u_g"])} if with_u else {}
    m = st.d_step(dev(c["x_real"]), c["alpha"], z=dev(c["z"]), eps=dev(c["eps"]), **kw_d)
    d_grads = grads_of(disc)
    assert all(p.grad is None for p in gen.parameters())
    mg = st.g_step(c["n"], c["alpha"], DEV, z=dev(c["z2"]), **kw_g)
    g_grads = grads_of(gen)
    losses = {"disc_loss": m["disc_loss"], "grad_pen": m["grad_pen"], "out_real_mean": m["out_real_mean"],
              "out_fake_mean": m["out_fake_mean"], "gen_loss": mg["gen_loss"], "g_out_fake_mean": mg["out_fake_mean"]}
    return {k: v.detach().clone() for k, v in losses.items()}, d_grads, g_grads


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_p_zero_is_bitwise_no_augmentation(case, fused):
    from musicgan_amd.networks import DiffAugment
    g = load(f"progan_{case}.npz")
    c = case_inputs(g, case)
    runs = []
    for aug in (None, DiffAugment("translation,cutout", 0.0)):
        st, gen, disc = build_stepper(g, aug, fused=fused)
        runs.append(both_updates(st, gen, disc, c, with_u=aug is not None))
    (la, da, ga), (lb, db, gb) = runs
    for a, b in ((la, lb), (da, db), (ga, gb)):
        assert a.keys() == b.keys() and len(a) > 0
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("case", CASES)
def test_fused_critic_update_is_disc_step_fused_on_the_augmented_batches(case):
    from musicgan_amd import aug_ops, ops
    from musicgan_amd.networks import DiffAugment, engine
    g = load(f"progan_{case}.npz")
    c = case_inputs(g, case)
    n, alpha = c["n"], c["alpha"]
    aug = DiffAugment("translation,cutout", P_ON)
    st, gen, disc = build_stepper(g, aug)
    u = torch.from_numpy(c["u_d"]).to(DEV)
    x_real, z, eps = c["x_real"].to(DEV), c["z"].to(DEV), c["eps"].to(DEV)
    m = st.d_step(x_real, alpha, z=z, eps=eps, u=u)
    got = grads_of(disc)
    # the same update by hand, on a second copy of the networks
    _, gen2, disc2 = build_stepper(g, None)
    with torch.no_grad():
        gen2._pack_cache.refresh(False)
        x_fake, _ = engine.gen_forward(gen2._weights(), z.contiguous(), alpha, gen2._pack_cache, save=False)
        xr, xf = aug_ops.diffaug_fwd(x_real, u[:n], *aug.spec), aug_ops.diffaug_fwd(x_fake.contiguous(), u[n:], *aug.spec)
        assert not torch.equal(xr, x_real) and not torch.equal(xf, x_fake)
        disc2._pack_cache.refresh(False)
        W, sink = disc2._weights(), engine.GradSink()
        disc_loss, grad_pen, out, stats = engine.disc_step_fused(W, xr, xf, eps, alpha, disc2._pack_cache, sink, defer=ops.WgradDefer())
    assert np.array_equal(bits(m["disc_loss"]), bits(disc_loss)) and np.array_equal(bits(m["grad_pen"]), bits(grad_pen))
    assert np.array_equal(bits(m["out_real_mean"]), bits(stats[0])) and np.array_equal(bits(m["out_fake_mean"]), bits(stats[1]))
    names = {id(p): k for k, p in disc2.named_parameters()}
    ref = {names[id(p)]: sink.get(p) for p in W.tensors()}
    assert sorted(ref) == sorted(got)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(ref[k])), k


@functools.lru_cache(maxsize=None)
def oracle_steps(case):
    """both updates of the float64 oracle with T in them, the float32 run of the same (the second term of grad_atol), the un-cancelled
    real term of the critic's gradient on the augmented real batch, and the un-augmented float64 updates (for the non-vacuity check)"""
    from oracle import progan as O
    g = load(f"progan_{case}.npz")
    c = case_inputs(g, case)
    gs, ds = build_oracle_states(g)
    d_args = (c["x_real"], c["z"], c["eps"], c["alpha"], c["u_d"], OPS_ALL, P_ON)
    g_args = (c["z2"], c["alpha"], c["u_g"], OPS_ALL, P_ON)
    d64, d32 = R.d_step_aug(gs, ds, *d_args, dtype=torch.float64), R.d_step_aug(gs, ds, *d_args, dtype=torch.float32)
    g64, g32 = R.g_step_aug(gs, ds, *g_args, dtype=torch.float64), R.g_step_aug(gs, ds, *g_args, dtype=torch.float32)
    terms = O.real_term_grads(ds, d64["x_real_aug"], c["alpha"])
    plain_d = O.d_step(gs, ds, c["x_real"], c["z"], c["eps"], c["alpha"], dtype=torch.float64, detach_fake=True)
    plain_g = O.g_step(gs, ds, c["z2"], c["alpha"], dtype=torch.float64)
    return dict(d64=d64, d32=d32, g64=g64, g32=g32, terms=terms, plain_d=plain_d, plain_g=plain_g)


@pytest.mark.parametrize("case", CASES)
def test_both_updates_meet_the_fp64_oracle_with_the_transform_in_it(case):
    """Every gradient of both updates within golden_util.grad_atol of the float64 oracle restatement (tests/diffaug_ref.py), losses and
    penalty within the tolerances of test_networks_gpu.py::test_fused_d_step_equals_module_path, the module path within twice the
    fused path's budget.  Not vacuous: the oracle's augmented and un-augmented gradients differ by more than 100x the budget on at
    least half of the tensors of each update, so an implementation that augments only one update, or forgets T^t, fails.

    The random numbers come from `well_posed_u`: inputs at which an oracle pre-activation sits on LeakyReLU's kink to within float32
    resolution are not a case any float32 evaluation can be held to (measured with seed 1234 on l2_rc16_gpnorm1: the small-map and
    the direct conv route computed -1.6e-7 and +6.4e-7 for an oracle value of +4.8e-7 at a scale of 10.9, took slopes 0.2 and 1 there,
    and the module path's critic gradients ended up to 10.5 budgets from the oracle while the fused path sat at 0.001)."""
    from musicgan_amd.networks import DiffAugment
    g = load(f"progan_{case}.npz")
    c = case_inputs(g, case)
    o = oracle_steps(case)
    d64, d32, g64, g32, terms = o["d64"], o["d32"], o["g64"], o["g32"], o["terms"]
    atol_d = {k: grad_atol(k, d64["d_grads"], d32["d_grads"], terms) for k in d64["d_grads"]}
    atol_g = {k: grad_atol(k, g64["g_grads"], g32["g_grads"]) for k in g64["g_grads"]}
    for which, atol, aug_g, plain in (("critic", atol_d, d64["d_grads"], o["plain_d"]["d_grads"]),
                                      ("generator", atol_g, g64["g_grads"], o["plain_g"]["g_grads"])):
        moved = [k for k in aug_g if maxabs_err(aug_g[k], plain[k]) > 100 * atol[k]]
        print(f"{case} {which}: augmentation moves {len(moved)} of {len(aug_g)} tensors by more than 100x their budget")
        assert 2 * len(moved) >= len(aug_g), (which, len(moved), len(aug_g))
    grads = {}
    for fused in (True, False):
        st, gen, disc = build_stepper(g, DiffAugment("translation,cutout", P_ON), fused=fused)
        losses, dg, gg = both_updates(st, gen, disc, c, with_u=True)
        out_scale = float(d64["out_real"].abs().max())
        print(f"{case} fused={fused}: disc_loss {float(losses['disc_loss']):.7f} vs {float(d64['disc_loss']):.7f}, grad_pen "
              f"{float(losses['grad_pen']):.6f} vs {float(d64['grad_pen']):.6f}, gen_loss {float(losses['gen_loss']):.7f} vs "
              f"{float(g64['gen_loss']):.7f}")
        assert abs(float(losses["disc_loss"]) - float(d64["disc_loss"])) <= 1e-6 + 2e-5 * out_scale
        assert abs(float(losses["grad_pen"]) - float(d64["grad_pen"])) <= 1e-5 * max(1.0, float(d64["grad_pen"]) / 10.0)
        assert abs(float(losses["gen_loss"]) - float(g64["gen_loss"])) <= 1e-6 + 2e-5 * float(g64["out_fake"].abs().max())
        grads[fused] = (dg, gg)
    for i, (ref, atol, name) in enumerate(((d64["d_grads"], atol_d, "critic"), (g64["g_grads"], atol_g, "generator"))):
        fused_g, module_g = grads[True][i], grads[False][i]
        assert sorted(fused_g) == sorted(module_g) == sorted(ref)
        for k, r in ref.items():
            e_f, e_m = maxabs_err(fused_g[k], r), maxabs_err(fused_g[k], module_g[k])
            print(f"{case} {name} {k}: fused vs fp64 {e_f:.3e}, fused vs module {e_m:.3e}, budget {atol[k]:.3e}")
            if float(r.abs().max()) < 1e-12:   # the classifier's bias in the critic update: -1 + 1, exactly 0 in the oracle
                assert float(fused_g[k].abs().max()) <= 1e-6 and float(module_g[k].abs().max()) <= 1e-6
                continue
            assert e_f <= atol[k], f"{name} {k}: fused path {e_f:.3e} > {atol[k]:.3e}"
            assert e_m <= 2 * atol[k], f"{name} {k}: fused vs module path {e_m:.3e} > {2 * atol[k]:.3e}"


@pytest.mark.parametrize("inject", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_graph_replay_equals_eager_updates_bit_for_bit(case, inject, monkeypatch):
    """four consecutive critic + generator updates (two eager, the capture, a replay), each with fresh z, eps and u -- injected, or drawn
    from the stepper's noise generator straight into the graph's static inputs -- against the MG_GRAPHS=0 stepper.  The optimizer
    steps are real here (a capture needs their state); the gradients are read from p.grad after every call."""
    from musicgan_amd.networks import DiffAugment
    g = load(f"progan_{case}.npz")
    c = case_inputs(g, case)
    n = c["n"]

    def run(graphs):
        monkeypatch.setenv("MG_GRAPHS", "1" if graphs else "0")
        noise = torch.Generator(device=DEV).manual_seed(77)
        st, gen, disc = build_stepper(g, DiffAugment("translation,cutout", 0.8), stub=False, noise=noise)
        assert st.use_graphs == graphs
        rng = torch.Generator(device=DEV).manual_seed(9)
        trace = []
        for it in range(4):
            alpha = min(1.0, c["alpha"] * (1 + it) / 4)
            x = torch.rand(n, 2, *g["x_real"].shape[2:], device=DEV, generator=rng) * 2 - 1
            kd, kg = {}, {}
            if inject:
                zs = tuple(g["z"].shape)
                kd = dict(z=torch.randn(zs, device=DEV, generator=rng), eps=torch.rand(n, 1, 1, 1, device=DEV, generator=rng),
                          u=torch.rand(2 * n, 8, device=DEV, generator=rng))
                kg = dict(z=torch.randn(zs, device=DEV, generator=rng), u=torch.rand(n, 8, device=DEV, generator=rng))
            m = st.d_step(x, alpha, **kd)
            trace += [m[k].clone() for k in sorted(m)] + [v for _, v in sorted(grads_of(disc).items())]
            m = st.g_step(n, alpha, DEV, **kg)
            trace += [m[k].clone() for k in sorted(m)] + [v for _, v in sorted(grads_of(gen).items())]
        st.finish()
        if graphs:
            assert sum("graph" in e for e in st._graphs.values()) == 2
        trace += [p.detach().clone() for net in (gen, disc) for p in net.parameters()]
        trace.append(noise.get_state().float())
        return trace

    on, off = run(True), run(False)
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(bits(a), bits(b)), i


# ----------------------------------------------------------------------------------------------------------------- train()

def _train():
    """`train` through the package's lazy re-export: importing the sub-module first would leave `musicgan_amd.train` bound to the module
    for the rest of the process, which other tests read as the function"""
    import musicgan_amd
    t = musicgan_amd.train
    return t if callable(t) else t.train


def _tiny_dataset(tmp_path, n=6):
    data = tmp_path / "data"
    data.mkdir()
    rng = torch.Generator().manual_seed(17)
    for i in range(n):
        x = (torch.rand(2, 512, 512, generator=rng) * 2 - 1).double()
        torch.save(x, str(data / f"magn_phase_{i}.pt"))
    return data


def test_augmented_training_resumes_bit_for_bit(tmp_path):
    """12 iterations straight == 6 iterations + a resume for 6 more, in weights and optimiser state; train_state carries the flags, and
    a run without them writes no new key.

    The networks grow once, from level 0 to level 1, before the interruption, and every parameter an optimiser holds stays part of
    its network to the end.  (A second growth drops the oldest stem from the critic; its last gradient stays on the dropped parameter
    and the uninterrupted run's Adam keeps stepping it, while a resumed run has no such gradient: the
    states of a parameter no network uses then differ, with or without augmentation.)"""
    train = _train()
    data = _tiny_dataset(tmp_path)
    kw = dict(nb_epoch=10, batch_size=2, num_workers=0, save_every=2, rand_channels=8,
              fadein_lengths=[1, 6, 6, 6, 6, 6, 6, 6], train_lengths=[5, 1000, 1000, 1000, 1000, 1000, 1000])
    aug = dict(augment="translation,cutout")
    torch.manual_seed(123)
    a = tmp_path / "straight"
    train("a", str(data), str(a), max_iters=12, **aug, **kw)
    torch.manual_seed(123)
    b = tmp_path / "interrupted"
    train("b", str(data), str(b), max_iters=6, **aug, **kw)
    assert os.path.exists(str(b / "train_state_2.pt")) and not os.path.exists(str(b / "train_state_3.pt"))
    torch.manual_seed(999)
    with pytest.raises(ValueError, match="would not continue it"):
        train("b", str(data), str(b), max_iters=12, resume_from=str(b), **kw)
    with pytest.raises(ValueError, match="would not continue it"):
        train("b", str(data), str(b), max_iters=12, resume_from=str(b), augment="cutout", **kw)
    train("b", str(data), str(b), max_iters=12, resume_from=str(b), **aug, **kw)
    sa, sb = torch.load(str(a / "train_state_5.pt")), torch.load(str(b / "train_state_5.pt"))
    assert sa["augment"] == sb["augment"] == "translation,cutout" and sa["augment_p"] == sb["augment_p"] == 1.0
    assert sa["level"] == sb["level"] == 1 and sa["iter_idx"] == sb["iter_idx"] == 12   # grew once
    assert sa["grower"] == sb["grower"]
    assert all(torch.equal(x, y) for x, y in zip(sa["noise_rng"], sb["noise_rng"]))
    for net in ("gen", "disc"):
        wa, wb = torch.load(str(a / f"{net}_5.pt")), torch.load(str(b / f"{net}_5.pt"))
        assert list(wa.keys()) == list(wb.keys())
        for k in wa:
            assert torch.equal(wa[k], wb[k]), f"{net} {k} differs after resume"
        oa, ob = torch.load(str(a / f"optim_{net}_5.pt")), torch.load(str(b / f"optim_{net}_5.pt"))
        assert oa["state"].keys() == ob["state"].keys()
        for i in oa["state"]:
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(oa["state"][i][key].cpu(), ob["state"][i][key].cpu()), f"optim_{net} state {i} {key}"
    # the augmentation changed the run (it is not a no-op that resumes trivially), and the plain run records nothing new
    torch.manual_seed(123)
    plain = tmp_path / "plain"
    train("p", str(data), str(plain), max_iters=6, **kw)
    sp = torch.load(str(plain / "train_state_2.pt"))
    assert "augment" not in sp and "augment_p" not in sp
    assert set(sp.keys()) == set(sb.keys()) - {"augment", "augment_p"}
    wp, wb6 = torch.load(str(plain / "disc_2.pt")), torch.load(str(b / "disc_2.pt"))
    assert any(not torch.equal(wp[k], wb6[k]) for k in wp)

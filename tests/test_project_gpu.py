"""GPU: the multi-scale L2 loss kernels (csrc/pyrloss.hip through musicgan_amd/proj_ops.py) against tests/pyrloss_ref.py,
networks.PyramidL2, the data-only backward pass of the generator, the projector on a tiny generator against the same algorithm in
float64 on the CPU, and generate's latents / morph_to / seed."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison  # noqa: E402
import pyrloss_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INPLACE = {"pyramid_l2": ("out",)}   # "`out` (optional) receives all of the gradient"


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.numpy().view(np.uint64 if t.dtype == torch.float64 else np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def case(shape):
    """inputs and reference of one kernel shape, computed once and only read afterwards"""
    *dims, levels = shape
    x, t = R.inputs(tuple(dims), 100 + levels + dims[-1])
    lam = R.default_weights(levels)
    d = R.pyramid(x, t, levels)
    g64, mag = R.grad64(d, lam)
    return x, t, lam, R.loss(d, lam), g64, mag


def run(x, t, lam=None, **kw):
    from musicgan_amd import proj_ops
    return proj_ops.pyramid_l2(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), lam, **kw)


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_loss_and_gradient_against_the_reference(shape):
    """loss: |l - l_ref| <= T 2^-53 l_ref (a float64 sum of T non-negative terms, in any order).  gradient: |g - g64| <=
    gamma_{L+2} k sum_s lambda_s |d_s| -- L roundings in the chain, one in k, one in the last product."""
    x, t, lam, l_ref, g64, mag = case(shape)
    levels = shape[-1]
    loss, g = run(x, t, lam)
    assert loss.dtype == torch.float64 and loss.shape == (shape[0],) and g.dtype == torch.float32 and g.shape == x.shape
    err_l = np.abs(loss.cpu().numpy() - l_ref)
    bound_l = R.terms(x.shape, levels) * 2.0 ** -53 * l_ref
    print("loss error / bound:", (err_l / bound_l).max())
    assert (err_l <= bound_l).all()
    err_g = np.abs(g.cpu().numpy().astype(np.float64) - g64)
    bound_g = R.gamma(levels + 2) * mag
    print("gradient error / bound:", (err_g / np.maximum(bound_g, 1e-300)).max())
    assert (err_g <= bound_g).all()
    # the default weights are 1 / L over the deepest pyramid the sides take
    if levels == min(7, 1 + min(int(np.log2(shape[2] & -shape[2])), int(np.log2(shape[3] & -shape[3])))):
        loss_d, g_d = run(x, t)
        assert same_bits(loss_d, loss) and same_bits(g_d, g)
    # again: the same bits
    loss2, g2 = run(x, t, lam)
    assert same_bits(loss2, loss) and same_bits(g2, g)


@pytest.mark.parametrize("shape", [(5, 1, 2, 6), (2, 2, 8, 8), (1, 2, 96, 32), (2, 2, 128, 192)], ids=str)
def test_plain_mse_and_zero_weights(shape):
    """levels = 1: g has the bits of (x - t) * k in torch float32.  weights (1, 0, .., 0): the same bits as levels = 1."""
    x, t = R.inputs(shape, 7)
    loss1, g1 = run(x, t, (1.0,))
    k = np.float32(2.0 / (shape[1] * shape[2] * shape[3]))
    want = (torch.from_numpy(x).to(DEV) - torch.from_numpy(t).to(DEV)) * float(k)
    assert float(torch.tensor(float(k), dtype=torch.float32)) == float(k)
    assert same_bits(g1, want)
    mse = ((x.astype(np.float64) - t.astype(np.float64)) ** 2).mean(axis=(1, 2, 3))
    np.testing.assert_allclose(loss1.cpu().numpy(), mse, rtol=1e-6)   # (d_0 is rounded to float32 first)
    levels = min(4, 1 + int(np.log2(shape[2] & -shape[2])), 1 + int(np.log2(shape[3] & -shape[3])))
    loss0, g0 = run(x, t, (1.0,) + (0.0,) * (levels - 1))
    assert same_bits(g0, g1) and same_bits(loss0, loss1)


def test_zero_weights_at_four_levels():
    x, t = R.inputs((2, 2, 8, 8), 8)
    assert same_bits(run(x, t, (1.0, 0.0, 0.0, 0.0))[1], run(x, t, (1.0,))[1])


@pytest.mark.parametrize("shape", [(5, 1, 2, 6, 2), (3, 2, 64, 64, 7), (2, 2, 128, 192, 7)], ids=str)
def test_identical_inputs_give_exact_zeros(shape):
    from musicgan_amd import proj_ops
    *dims, levels = shape
    x = torch.from_numpy(R.inputs(tuple(dims), 9)[0]).to(DEV)
    for t in (x, x.clone()):
        loss, g = proj_ops.pyramid_l2(x, t, R.default_weights(levels))
        assert not bits(loss).any() and not bits(g).any()   # 0.0 and +0.0: all bits clear


def test_samples_are_independent():
    """a batch of 3 equals three batches of 1 bit for bit; NaN planted in sample 1 leaves samples 0 and 2 alone"""
    shape, levels = (3, 2, 128, 192), 7
    x, t = R.inputs(shape, 10)
    lam = R.default_weights(levels)
    loss, g = run(x, t, lam)
    for i in range(3):
        li, gi = run(x[i:i + 1], t[i:i + 1], lam)
        assert same_bits(li, loss[i:i + 1]) and same_bits(gi, g[i:i + 1])
    xn = x.copy()
    xn[1, 0, 70, 130] = np.nan
    loss_n, g_n = run(xn, t, lam)
    for i in (0, 2):
        assert same_bits(loss_n[i:i + 1], loss[i:i + 1]) and same_bits(g_n[i:i + 1], g[i:i + 1])
    assert bool(torch.isnan(loss_n[1])) and bool(torch.isnan(g_n[1]).any())


@pytest.mark.parametrize("shape", [(5, 1, 2, 6, 2), (2, 2, 128, 192, 7)], ids=str)
def test_loss_alone_leaves_the_gradient_buffer_untouched(shape):
    from musicgan_amd import proj_ops
    x, t, lam, *_ = case(shape)
    loss, _ = run(x, t, lam)
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    with poison.poisoned(0xFF, module=proj_ops, inplace=INPLACE):
        loss_only, none = proj_ops.pyramid_l2(xd, td, lam, need_grad=False)
    assert none is None and same_bits(loss_only, loss)
    buf = torch.full(x.shape, float("nan"), device=DEV)
    before = bits(buf).copy()
    proj_ops.pyramid_l2(xd, td, lam, out=buf)
    assert same_bits(buf, run(x, t, lam)[1]) and not np.array_equal(bits(buf), before)
    with pytest.raises(ValueError):
        proj_ops.pyramid_l2(xd, td, lam, need_grad=False, out=buf)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (5, 1, 2, 6, 2), (1, 2, 96, 32, 6), (2, 2, 128, 192, 7)], ids=str)
def test_on_poisoned_memory_between_guard_bands(shape):
    """the call under poison.rule: outputs and workspace between guard bands that stay intact, no input changed, the same bits
    whatever the memory held before (so every output element is written), nothing non-finite; and every float64 of the workspace
    that the plan asks for is written (under fill 0xFF an unwritten one reads as NaN)"""
    from musicgan_amd import ops, proj_ops
    x, t, lam, *_ = case(shape)
    loss, g = run(x, t, lam)
    nbytes = proj_ops.pyramid_l2_ws_bytes(*shape)
    assert nbytes == R.plan(*shape)["ws_bytes"]

    def body(p):
        p.out = proj_ops.pyramid_l2(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), lam)
        torch.cuda.synchronize()
        (ws,) = [b for b in ops._ws_cache.values()]
        p.partials = ws[:nbytes].view(torch.float64).clone()

    r0, r1 = poison.rule(body, module=proj_ops, inplace=INPLACE)
    for r in (r0, r1):
        assert same_bits(r.out[0], loss) and same_bits(r.out[1], g)
        assert bool(torch.isfinite(r.partials).all()) and bool((r.partials >= 0).all())
    assert same_bits(r0.partials, r1.partials)
    assert "pyramid_l2" in {name for name, _, _ in r1.calls}


def test_one_captured_graph_follows_x():
    from musicgan_amd import proj_ops
    shape, levels = (2, 2, 128, 192), 7
    lam = R.default_weights(levels)
    xs = torch.from_numpy(R.inputs(shape, 20)[0]).to(DEV)
    ts = torch.from_numpy(R.inputs(shape, 21)[0]).to(DEV)
    gs = torch.empty_like(xs)
    proj_ops.pyramid_l2(xs, ts, lam, out=gs)   # (the library is loaded and warm before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ls, _ = proj_ops.pyramid_l2(xs, ts, lam, out=gs)
    for seed in (22, 23):
        xs.copy_(torch.from_numpy(R.inputs(shape, seed)[0]))
        gs.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want_l, want_g = proj_ops.pyramid_l2(xs.clone(), ts, lam)
        assert same_bits(ls, want_l) and same_bits(gs, want_g), seed


def test_bad_arguments_raise():
    from musicgan_amd import _lib, proj_ops
    x = torch.zeros(1, 2, 8, 8, device=DEV)
    for bad in (dict(weights=(1.0,) * 5), dict(weights=(-1.0,)), dict(weights=())):
        with pytest.raises(ValueError):
            proj_ops.pyramid_l2(x, x, **bad)
    with pytest.raises(ValueError):
        proj_ops.pyramid_l2(x, torch.zeros(1, 1, 8, 8, device=DEV))
    with pytest.raises(ValueError):
        proj_ops.pyramid_l2(x[0], x[0])
    with pytest.raises(_lib.MusicGanHipError):
        proj_ops.pyramid_l2(x, x.double())
    with pytest.raises(_lib.MusicGanHipError):
        proj_ops.pyramid_l2(x, x, out=x)   # the gradient over an input: the library refuses


# ------------------------------------------------------------------ networks.PyramidL2
def _loss64(img, tgt, lam):
    """the definition in float64 torch (checked against the reference on the CPU, tests/test_project_cpu.py): (N,) losses"""
    cur, total = img - tgt, 0.0
    for s, l in enumerate(lam):
        if s:
            cur = torch.nn.functional.avg_pool2d(cur, 2)
        total = total + float(np.float32(l)) * (cur * cur).mean(dim=(1, 2, 3))
    return total


@pytest.mark.parametrize("shape", [(3, 2, 64, 64, 7), (5, 1, 2, 6, 2)], ids=str)
def test_module_backward_with_a_non_uniform_upstream(shape):
    from musicgan_amd import networks
    x, t, lam, l_ref, g64, mag = case(shape)
    levels = shape[-1]
    up = torch.linspace(-1.5, 2.0, shape[0], dtype=torch.float64)
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    td = torch.from_numpy(t).to(DEV).requires_grad_(True)
    loss = networks.PyramidL2(levels=levels)(xd, td)
    assert loss.dtype == torch.float64 and np.array_equal(bits(loss), bits(run(x, t, lam)[0]))
    (loss * up.to(DEV)).sum().backward()
    assert td.grad is None
    # against the reference's g64 times the upstream value: the kernel's L + 2 roundings and the one of the product with the upstream
    # value, which is a float32 number here (multiples of 1/8), so that its conversion rounds nothing
    assert torch.equal(up.float().double(), up)
    upb = up.reshape(-1, 1, 1, 1)
    err = (xd.grad.double().cpu() - torch.from_numpy(g64) * upb).abs()
    bound = R.gamma(levels + 3) * torch.from_numpy(mag) * upb.abs()
    print("module gradient error / bound:", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    # and against float64 autograd through the definition, whose pyramid is not rounded to float32 level by level.  A level adds two
    # roundings of sums of |d| <= max |d_0| (the product with 0.25 is exact), so |d_s - exact| <= 2 s u max |d_0|, and with
    # sum lambda_s = 1 the gradient moves by at most 2 L u k max |d_0|: added, since |d_s| does not cover it where d_s cancels
    x64 = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    (_loss64(x64, torch.from_numpy(t.astype(np.float64)), lam) * up).sum().backward()
    k = 2.0 / (shape[1] * shape[2] * shape[3])
    slack = bound + 2 * levels * 2.0 ** -24 * k * float(np.abs(x.astype(np.float64) - t).max()) * upb.abs()
    assert bool(((xd.grad.double().cpu() - x64.grad).abs() <= slack).all())
    assert networks.PyramidL2(weights=lam)(xd.detach(), td.detach()).requires_grad is False


# ------------------------------------------------------------------ the data-only backward pass
@pytest.mark.parametrize("level,alpha", [(0, 1.0), (1, 1.0), (2, 1.0), (2, 0.5), (3, 1.0)])
def test_frozen_parameters_take_the_data_only_pass(level, alpha):
    from musicgan_amd.networks import Generator
    from oracle import progan as O
    torch.manual_seed(30 + level)
    gs = O.GenState(32, end_layer=level)
    gen = Generator(32, end_layer=level)
    gen.load_state_dict(gs.params)
    gen = gen.to(DEV)
    rng = torch.Generator().manual_seed(5)
    z0 = torch.randn(2, 32, 2, 2, generator=rng)
    side = 4 << level
    g_out = torch.randn(2, 2, side, side, generator=rng)

    def backward():
        z = z0.to(DEV).requires_grad_(True)
        gen.zero_grad()
        gen(z, alpha).backward(g_out.to(DEV))
        return z.grad

    gz_train = backward()
    assert len([k for k, p in gen.named_parameters() if p.grad is not None]) == 4 * (level + 1) + (4 if level else 2)
    for p in gen.parameters():
        p.requires_grad_(False)
    gz = backward()
    assert same_bits(gz, gz_train)
    assert all(p.grad is None for p in gen.parameters())
    errs = {}
    for dtype in (torch.float64, torch.float32):
        p = {k: v.to(dtype) for k, v in gs.params.items()}
        z = z0.to(dtype).requires_grad_(True)
        (O.gen_forward(p, level, gs.has_last, z, alpha) * g_out.to(dtype)).sum().backward()
        errs[dtype] = z.grad
    tol = max(1e-3, 2.0 * maxrel(errs[torch.float32], errs[torch.float64]))
    assert maxrel(gz, errs[torch.float64]) <= tol


def test_data_only_sink_launches_no_weight_gradient():
    """the routing census of one frozen backward pass at level 3: no conv3x3_wgrad / conv1x1_wgrad launch, and the same data-path
    launches as the trainable pass"""
    from routing_census import census
    from musicgan_amd import ops
    from musicgan_amd.networks import Generator
    torch.manual_seed(3)
    gen = Generator(16, end_layer=3).to(DEV)
    z0 = torch.randn(2, 16, 2, 2, device=DEV)

    def names():
        z = z0.clone().requires_grad_(True)
        out = gen(z, 1.0)
        with census(ops) as c:
            out.backward(torch.ones_like(out))
        return [r[0] for r in c.calls]

    full = names()
    for p in gen.parameters():
        p.requires_grad_(False)
    frozen = names()
    assert any("wgrad" in n for n in full) and not any("wgrad" in n for n in frozen)
    rest = iter(full)
    assert all(n in rest for n in frozen)   # the frozen pass's launches, in order, are launches of the trainable pass
    print("only in the trainable pass:", sorted(set(full) - set(frozen)))
    assert len(frozen) < len(full)


# ------------------------------------------------------------------ the projector, tiny
def _cpu_projection(gs, targets, cands, lam, steps, lr, dtype):
    """the projector's algorithm on the CPU: oracle forward, the definition of the loss, autograd down to z, oracle Adam"""
    from oracle import progan as O
    p = {k: v.to(dtype) for k, v in gs.params.items()}
    tg = targets.to(dtype)
    fwd = lambda z: O.gen_forward(p, gs.curr_layer, gs.has_last, z, 1.0)
    z = []
    for wi, zc in enumerate(cands):
        with torch.no_grad():
            lc = _loss64(fwd(zc.to(dtype)), tg[wi:wi + 1], lam)
        z.append(zc[int(torch.argmin(lc))].to(dtype))
    z = torch.stack(z)
    m, v, hist = torch.zeros_like(z), torch.zeros_like(z), []
    for k in range(steps):
        zk = z.clone().requires_grad_(True)
        loss = _loss64(fwd(zk), tg, lam)
        loss.sum().backward()
        hist.append(loss.detach())
        z, m, v = O.adam_update(z, zk.grad, m, v, k + 1, lr=lr, beta1=0.9, beta2=0.999)
    with torch.no_grad():
        return z, torch.stack(hist), _loss64(fwd(z), tg, lam)


def test_projection_matches_the_float64_algorithm():
    from musicgan_amd import project, proj_ops
    from musicgan_amd.networks import Generator
    from oracle import progan as O
    level, rc, n, cands_n, steps, lr, seed = 2, 8, 3, 4, 10, 0.05, 0
    torch.manual_seed(40)
    gs = O.GenState(rc, end_layer=level)
    gen = Generator(rc, end_layer=level)
    gen.load_state_dict(gs.params)
    gen = gen.to(DEV).eval()
    z_star = torch.randn(n, rc, 2, 2, generator=torch.Generator().manual_seed(41))
    with torch.no_grad():
        p64 = {k: v.double() for k, v in gs.params.items()}
        targets = O.gen_forward(p64, level, gs.has_last, z_star.double(), 1.0).float()
    assert targets.shape == (n, 2, 16, 16)
    lam = proj_ops.check_weights(16, 16)
    cands = [project.draw_candidates(seed, wi, cands_n, rc, torch.device(DEV)).cpu() for wi in range(n)]
    z64, hist64, end64 = _cpu_projection(gs, targets, cands, lam, steps, lr, torch.float64)
    z32, _, _ = _cpu_projection(gs, targets, cands, lam, steps, lr, torch.float32)
    print("float64 losses:", hist64[0].tolist(), "->", end64.tolist())
    assert bool((end64 < hist64[0]).all()), "the float64 algorithm itself does not descend at this seed / lr: change them"

    kw = dict(steps=steps, lr=lr, candidates=cands_n, batch_size=2, seed=seed, schedule=False)
    res = project.project_images(gen, targets.to(DEV), **kw)
    assert all(p.requires_grad for p in gen.parameters())   # put back as they were
    assert res["latents"].shape == (n, rc, 2, 2) and res["latents"].dtype == torch.float32
    assert res["history"].shape == (steps, n) and res["loss"].dtype == torch.float64
    tol = max(1e-3, 2.0 * maxrel(z32, z64))
    print("z after the steps, against float64:", maxrel(res["latents"], z64), "allowed", tol)
    assert maxrel(res["latents"], z64) <= tol
    assert bool((res["loss"] < res["loss_start"]).all())
    assert torch.equal(res["loss_start"], res["history"][0])
    np.testing.assert_allclose(res["loss_start"].numpy(), hist64[0].numpy(), rtol=1e-3)
    # rms: the square root of the plain MSE of the final images
    with torch.no_grad():
        img = gen(res["latents"].to(DEV), 1.0)
    mse = ((img.double() - targets.to(DEV).double()) ** 2).mean(dim=(1, 2, 3)).sqrt().cpu()
    np.testing.assert_allclose(res["rms"].numpy(), mse.numpy(), rtol=1e-5)
    again = project.project_images(gen, targets.to(DEV), **kw)
    assert same_bits(again["latents"], res["latents"]) and same_bits(again["loss"], res["loss"])


def test_project_writes_the_same_bytes_twice(tmp_path):
    """project() end to end at level 2 on a short synthetic recording: latents.pt has the same bytes in two runs, the dict has the
    documented entries, projection.json one record per window, and no audio below level 7; a file shorter than one window raises"""
    import json
    from musicgan_amd import audio, project
    from musicgan_amd.networks import Generator
    torch.manual_seed(50)
    ckpt = str(tmp_path / "gen.pt")
    torch.save(Generator(8, end_layer=2).state_dict(), ckpt)
    frames = audio.STFT_STRIDE * (2 * audio.N_VEC + 8)
    tone = 0.3 * torch.sin(torch.arange(frames) * 0.05) + 0.05 * torch.randn(frames, generator=torch.Generator().manual_seed(51))
    clip = str(tmp_path / "clip.wav")
    audio.wavio.save(clip, tone[None, :], audio.SAMPLE_RATE)
    blobs = []
    for name in ("a", "b"):
        out = str(tmp_path / name)
        d = project.project(ckpt, 8, clip, out, level=2, steps=3, candidates=2, batch_size=2, seed=4)
        blobs.append(open(os.path.join(out, "latents.pt"), "rb").read())
        assert sorted(os.listdir(out)) == ["latents.pt", "projection.json"]
    assert blobs[0] == blobs[1]
    d = torch.load(os.path.join(out, "latents.pt"))
    n = d["latents"].shape[0]
    assert n == 2 and d["latents"].shape == (n, 8, 2, 2) and d["latents"].dtype == torch.float32 and not d["latents"].is_cuda
    assert d["loss"].dtype == d["loss_start"].dtype == torch.float64 and d["loss"].shape == d["loss_start"].shape == (n,)
    assert (d["rand_channels"], d["level"], d["steps"], d["seed"], d["source"]) == (8, 2, 3, 4, "clip.wav")
    rec = json.load(open(os.path.join(out, "projection.json")))
    assert len(rec["windows"]) == n and set(rec["windows"][0]) == {"loss_start", "loss", "rms"}
    assert torch.equal(project.load_latents(os.path.join(out, "latents.pt"), 8, 2), d["latents"])
    short = str(tmp_path / "short.wav")
    audio.wavio.save(short, tone[None, :audio.STFT_STRIDE * 100], audio.SAMPLE_RATE)
    with pytest.raises(ValueError):
        project.project(ckpt, 8, short, str(tmp_path / "c"), level=2, steps=1, candidates=1)


# ------------------------------------------------------------------ generate
@pytest.fixture(scope="module")
def full_generator(tmp_path_factory):
    """a level-7 checkpoint with few latent channels, and two latents files of two windows"""
    from musicgan_amd.networks import Generator
    d = tmp_path_factory.mktemp("generate_latents")
    torch.manual_seed(60)
    rc = 4
    ckpt = str(d / "gen.pt")
    torch.save(Generator(rc, end_layer=7).state_dict(), ckpt)
    files = []
    for i in range(2):
        z = torch.randn(2, rc, 2, 2, generator=torch.Generator().manual_seed(61 + i))
        files.append(str(d / f"latents_{i}.pt"))
        torch.save({"latents": z, "loss": torch.zeros(2, dtype=torch.float64), "loss_start": torch.zeros(2, dtype=torch.float64),
                    "rand_channels": rc, "level": 7, "steps": 0, "seed": 0, "source": "none"}, files[-1])
    return d, ckpt, rc, files


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_generate_from_latents_and_morph(full_generator):
    from musicgan_amd import audio, project
    from musicgan_amd.generate import _load_generator, generate
    d, ckpt, rc, (fa, fb) = full_generator
    generate(str(d / "a"), rc, ckpt, 7, 9, latents=fa)
    generate(str(d / "b"), rc, ckpt, 7, 9, latents=fb)
    assert os.listdir(d / "a") == ["sound_0.wav"]
    gen = _load_generator(rc, ckpt, torch.device(DEV))
    wide = project.wide_latent(project.load_latents(fa, rc)).to(DEV)
    assert wide.shape == (1, rc, 2, 4)
    with torch.no_grad():
        audio.magn_phase_to_wav(gen(wide, 1.0), str(d / "direct.wav"), audio.SAMPLE_RATE)
    assert _read(d / "a" / "sound_0.wav") == _read(d / "direct.wav")
    generate(str(d / "m"), rc, ckpt, 7, 2, latents=fa, morph_to=fb)
    assert sorted(os.listdir(d / "m")) == ["sound_0.wav", "sound_1.wav"]
    assert _read(d / "m" / "sound_0.wav") == _read(d / "a" / "sound_0.wav")
    assert _read(d / "m" / "sound_1.wav") == _read(d / "b" / "sound_0.wav")
    assert _read(d / "a" / "sound_0.wav") != _read(d / "b" / "sound_0.wav")


def test_generate_seed(full_generator):
    from musicgan_amd import audio
    from musicgan_amd.generate import _load_generator, generate
    d, ckpt, rc, _ = full_generator
    generate(str(d / "s1"), rc, ckpt, 1, 1, seed=5)
    generate(str(d / "s2"), rc, ckpt, 1, 1, seed=5)
    generate(str(d / "s3"), rc, ckpt, 1, 1, seed=6)
    assert _read(d / "s1" / "sound_0.wav") == _read(d / "s2" / "sound_0.wav") != _read(d / "s3" / "sound_0.wav")
    # seed=None: the global generator's next draw, as before
    torch.manual_seed(1)
    generate(str(d / "g"), rc, ckpt, 1, 1)
    torch.manual_seed(1)
    z = torch.randn(1, rc, 2, 2, device=torch.device("cuda", torch.cuda.current_device()))
    gen = _load_generator(rc, ckpt, torch.device(DEV))
    with torch.no_grad():
        audio.magn_phase_to_wav(gen(z.contiguous(), 1.0), str(d / "parent.wav"), audio.SAMPLE_RATE)
    assert _read(d / "g" / "sound_0.wav") == _read(d / "parent.wav")

"""GPU: the exponential running average of the generator's weights kept inside the fused Adam launch (mg_adam_step_dev_ema,
csrc/elementwise.hip) -- the kernel against mg_adam_step_dev and the float64 recurrence, FusedAdam(ema_decay=...), the stepper,
growth, and `train --ema-decay` end to end.  Every bound is derived where it is used; none is fitted to what the kernel gives."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24   # unit round-off of float32, round to nearest: |fl(x) - x| <= U |x|
HYPER = dict(lr=1e-3, beta1=0.0, beta2=0.9, eps=1e-8)


# ------------------------------------------------------------------ tensor sets
def _sets():
    """name -> the sizes of one call; 'flat': slices of one flat buffer that start at multiples of 4 bytes, not of 16"""
    return {
        "one element": [1],
        "not a multiple of four": [1023, 7, 5],
        "flat slices at 4-byte offsets": "flat",
        "more tensors than a chunk": [4 * (i % 9) + (i % 3) + 1 for i in range(131)],   # 48 records per launch: three chunks
        "multi-MB": [3 * 1024 * 1024 + 4, 513],
    }


def _make(sizes, seed, zero_moments=False, zero_grads=False):
    """equal seeded states: lists p, g, m, v (float32), s (int32 step counts, all 0) and, for 'flat', cut out of flat buffers"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if sizes == "flat":
        cuts = [(1, 37), (38, 64), (103, 4), (107, 1021), (1131, 256), (1388, 12)]   # (offset, length) in floats; only the last is 16-byte aligned
        total = 1400
        flats = [torch.randn(total, device=DEV, generator=g) for _ in range(4)]
        flats[3].abs_()
        p, gr, m, v = ([f[o:o + n] for o, n in cuts] for f in flats)
        assert any(t.data_ptr() % 16 for t in p) and any(t.data_ptr() % 16 == 0 and t.numel() % 4 == 0 for t in p)
    else:
        p = [torch.randn(n, device=DEV, generator=g) for n in sizes]
        gr = [torch.randn(n, device=DEV, generator=g) for n in sizes]
        m = [torch.randn(n, device=DEV, generator=g) * 0.1 for n in sizes]
        v = [torch.rand(n, device=DEV, generator=g) * 0.1 for n in sizes]
    if zero_moments:
        for t in m + v:
            t.zero_()
    if zero_grads:
        for t in gr:
            t.zero_()
    s = [torch.zeros((), dtype=torch.int32, device=DEV) for _ in p]
    return p, gr, m, v, s


def _plain_step(p, g, m, v, s, grad_scale=1.0):
    """the existing entry point, called as FusedAdam calls it"""
    from musicgan_amd import _lib
    recs = (_lib.AdamTensorDev * len(p))(*[_lib.AdamTensorDev(a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), a.numel(),
                                                                 e.data_ptr()) for a, b, c, d, e in zip(p, g, m, v, s)])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().mg_adam_step_dev(ctypes.cast(recs, ctypes.c_void_p), len(p), HYPER["lr"], HYPER["beta1"], HYPER["beta2"],
                                            HYPER["eps"], grad_scale, stream), "mg_adam_step_dev")


def _new_grads(g, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    for t in g:
        t.copy_(torch.randn(t.shape, device=DEV, generator=gen))


# ------------------------------------------------------------------ 1. Adam is untouched
@pytest.mark.parametrize("name", list(_sets()))
def test_adam_arithmetic_is_bitwise_the_plain_step(name):
    from musicgan_amd import avg_ops
    sizes = _sets()[name]
    a, b = _make(sizes, 11), _make(sizes, 11)
    ema = [t.clone() for t in a[0]]
    for k in range(7):
        _new_grads(a[1], 100 + k)
        _new_grads(b[1], 100 + k)
        avg_ops.adam_step_ema(*a, ema, **HYPER, grad_scale=0.5, decay=0.999)
        _plain_step(*b, grad_scale=0.5)
    torch.cuda.synchronize()
    for what, xs, ys in zip(("param", "grad", "exp_avg", "exp_avg_sq", "steps"), a, b):
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert torch.equal(x, y), f"{name}: {what}[{i}] differs from mg_adam_step_dev"
    assert all(int(s) == 7 for s in a[4])
    assert all(bool(torch.isfinite(e).all()) for e in ema) and any(not torch.equal(e, p) for e, p in zip(ema, a[0]))


# ------------------------------------------------------------------ 2. the average is right
@pytest.mark.parametrize("decay", [0.5, 0.999])
@pytest.mark.parametrize("name", list(_sets()))
def test_average_within_the_rounding_bound_of_the_float64_recurrence(name, decay):
    """The kernel evaluates e' = fl(e + fl(fl(p - e) w)), w = fl(1 - d): three roundings.  With M the larger of |p| and |e| (per
    element, over the run): |p - e| <= 2 M, so the first rounding errs by <= U 2M and reaches e' scaled by w; the second by
    <= U 2M w; the third by <= U M.  Together U M (1 + 4 w) per step, which is <= 3 U M for w <= 1/2 -- both decays here -- i.e.
    three roundings of at most U M each.  An error present in e is carried on scaled by (1 - w), so after n steps the local errors
    have added up to at most 3 U M (1 + (1 - w) + ...) <= 3 U M min(n, 1 / w).  The float64 recurrence runs on the kernel's own
    float32 p_k and the kernel's own w; its rounding (2^-53) is far below."""
    from musicgan_amd import avg_ops
    n = 7
    sizes = _sets()[name]
    p, g, m, v, s = _make(sizes, 23)
    ema = [t.clone() + 0.25 for t in p]                     # away from the fixed point from the first step on
    w = avg_ops.ema_weight(decay)
    assert w <= 0.5
    e64 = [e.double() for e in ema]
    big = [torch.maximum(e.abs(), q.abs()).double() for e, q in zip(ema, p)]
    for k in range(n):
        _new_grads(g, 200 + k)
        avg_ops.adam_step_ema(p, g, m, v, s, ema, **HYPER, decay=decay)
        for i in range(len(p)):
            e64[i] += (p[i].double() - e64[i]) * w
            big[i] = torch.maximum(big[i], torch.maximum(p[i].abs(), ema[i].abs()).double())
    torch.cuda.synchronize()
    worst = 0.0
    for i in range(len(p)):
        bound = 3 * U * big[i] * min(n, 1.0 / w)
        err = (ema[i].double() - e64[i]).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), f"{name}, decay {decay}: tensor {i}: error {float(err.max()):.3e}, {worst:.3f} of the bound"
    print(f"EMA {name} decay {decay}: worst error {worst:.3f} of the a-priori bound")
    assert all(not torch.equal(e, q) for e, q in zip(ema, p))    # the average is not simply the weights


# ------------------------------------------------------------------ 3. fixed point
@pytest.mark.parametrize("name", list(_sets()))
def test_average_equal_to_the_weights_is_an_exact_fixed_point(name):
    from musicgan_amd import avg_ops
    p, g, m, v, s = _make(_sets()[name], 31, zero_moments=True, zero_grads=True)
    p0 = [t.clone() for t in p]
    ema = [t.clone() for t in p]
    for _ in range(7):
        avg_ops.adam_step_ema(p, g, m, v, s, ema, **HYPER, decay=0.999)
    torch.cuda.synchronize()
    for i in range(len(p)):
        assert torch.equal(p[i], p0[i]) and torch.equal(ema[i], p0[i]), f"{name}: tensor {i} moved"
    assert all(int(x) == 7 for x in s)


def test_bad_arguments_are_refused_by_the_library():
    from musicgan_amd import _lib, avg_ops
    p, g, m, v, s = _make([8], 1)
    lib = _lib.load()
    rec = (_lib.AdamTensorDevEma * 1)(_lib.AdamTensorDevEma(p[0].data_ptr(), g[0].data_ptr(), m[0].data_ptr(), v[0].data_ptr(), 8,
                                                            s[0].data_ptr(), None))
    args = (ctypes.cast(rec, ctypes.c_void_p), 1, 1e-3, 0.0, 0.9, 1e-8, 1.0)
    assert lib.mg_adam_step_dev_ema(*args, 0.5, None) != 0 and b"null pointer" in lib.mg_last_error()
    rec[0].ema = p[0].data_ptr()
    for w in (0.0, -0.5, 1.5, float("nan")):
        assert lib.mg_adam_step_dev_ema(*args, w, None) != 0 and b"ema_weight" in lib.mg_last_error()
    with pytest.raises(_lib.MusicGanHipError):
        avg_ops.adam_step_ema(p, g, m, v, [s[0].float()], [p[0].clone()], **HYPER, decay=0.9)   # steps must be int32
    torch.cuda.synchronize()
    assert int(s[0]) == 0


# ------------------------------------------------------------------ 4. FusedAdam(ema_decay=d)
@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_fused_adam_with_average_against_torch_adam(decay):
    """Parameters against torch.optim.Adam on the same gradients; the moments do not depend on the parameters, so the two
    implementations drift apart by rounding alone: per step one rounding of p (U |p|) in each, plus the update term lr * m^ /
    (sqrt(v^) + eps), at most lr / sqrt(1 - beta2) in size (v >= (1 - beta2) g^2 with beta1 = 0) and formed in under ten float32
    operations in each: n (2 U P + 20 U lr / sqrt(1 - beta2)).  The averages against the float64 recurrence as in test 2."""
    from musicgan_amd import avg_ops
    from musicgan_amd.optim import FusedAdam
    n, lr, betas = 7, 1e-3, (0.0, 0.9)
    gen = torch.Generator(device=DEV).manual_seed(5)
    shapes = [(64, 48, 3, 3), (48,), (7, 3), (2, 48, 1, 1), (5,)]
    ours = [torch.nn.Parameter(torch.randn(s, device=DEV, generator=gen)) for s in shapes]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    start = [p.detach().clone() for p in ours]
    opt = FusedAdam(ours, lr=lr, betas=betas, ema_decay=decay)
    ref = torch.optim.Adam(theirs, lr=lr, betas=betas)
    w = avg_ops.ema_weight(decay)
    e64, big, frozen = {}, {}, None
    for k in range(n):
        for i, (p, q) in enumerate(zip(ours, theirs)):
            # the last parameter never has a gradient, the one before it loses its gradient after three steps
            if i == len(ours) - 1 or (i == len(ours) - 2 and k >= 3):
                p.grad = q.grad = None
                continue
            p.grad = torch.randn(p.shape, device=DEV, generator=gen)
            q.grad = p.grad.clone()
            if p not in e64:
                e64[p], big[p] = p.detach().double(), p.detach().abs().double()   # "Gs starts as a copy of G"
        if k == 3:
            frozen = opt.state[ours[-2]]["ema"].clone()
        opt.step()
        ref.step()
        for p in ours:
            if p.grad is not None:
                e64[p] += (p.detach().double() - e64[p]) * w
                big[p] = torch.maximum(big[p], torch.maximum(p.detach().abs(), opt.state[p]["ema"].abs()).double())
    torch.cuda.synchronize()
    tol = n * (2 * U * max(float(p.detach().abs().max()) for p in ours) + 20 * U * lr / (1 - betas[1]) ** 0.5)
    for i, (p, q) in enumerate(zip(ours, theirs)):
        assert float((p.detach() - q.detach()).abs().max()) <= tol, f"parameter {i} against torch.optim.Adam"
    for i, p in enumerate(ours[:-1]):
        steps = n if i < len(ours) - 2 else 3
        assert float(opt.state[p]["step"]) == steps and int(opt.state[p]["step_dev"]) == steps
        assert float(ref.state[theirs[i]]["step"]) == steps
        err = (opt.state[p]["ema"].double() - e64[p]).abs()
        assert bool((err <= 3 * U * big[p] * min(steps, 1.0 / w)).all()), f"average {i}: {float(err.max()):.3e}"
        assert opt.averaged(p) is opt.state[p]["ema"] and not torch.equal(opt.state[p]["ema"], p.detach())
    # skipped parameters: no state and no average for the one that never had a gradient; an average at rest for the other
    assert ours[-1] not in opt.state and opt.averaged(ours[-1]) is ours[-1] and torch.equal(ours[-1].detach(), start[-1])
    assert torch.equal(opt.state[ours[-2]]["ema"], frozen)
    # the state dict travels to torch.optim.Adam and back with the averages
    sd = opt.state_dict()
    torch.optim.Adam(theirs, lr=lr, betas=betas).load_state_dict(sd)
    again = FusedAdam(ours, lr=lr, betas=betas, ema_decay=decay)
    again.load_state_dict(sd)
    for p in ours[:-1]:
        assert torch.equal(again.state[p]["ema"], opt.state[p]["ema"]) and again.state[p]["ema"].is_cuda


# ------------------------------------------------------------------ 5. training is not perturbed
def _run_stepper(level, batch, decay, graphs, monkeypatch, iters=12):
    import bench
    from musicgan_amd.optim import FusedAdam
    from musicgan_amd.train_step import ProGANStepper
    monkeypatch.setenv("MG_GRAPHS", "1" if graphs else "0")
    gen, disc = bench.build_nets(level, 8, DEV)
    og = FusedAdam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9), ema_decay=decay)
    od = FusedAdam(disc.parameters(), lr=1e-3, betas=(0.0, 0.9))
    st = ProGANStepper(gen, disc, og, od, 8)
    assert st.use_graphs == graphs
    side = bench.LEVEL_SIDE[level]
    rng = torch.Generator(device=DEV).manual_seed(77)
    for i in range(iters):
        x = torch.rand(batch, 2, side, side, device=DEV, generator=rng) * 2 - 1
        z = torch.randn(batch, 8, 2, 2, device=DEV, generator=rng)
        eps = torch.rand(batch, 1, 1, 1, device=DEV, generator=rng)
        zg = torch.randn(batch, 8, 2, 2, device=DEV, generator=rng)
        st.d_step(x, 0.5, z=z, eps=eps)
        if i % 5 == 0:
            st.g_step(batch, 0.5, DEV, z=zg)
    st.finish()
    torch.cuda.synchronize()
    out = {}
    for tag, net, opt in (("gen", gen, og), ("disc", disc, od)):
        for k, p in net.named_parameters():
            out[f"{tag}.{k}"] = p.detach().clone()
            for key in ("exp_avg", "exp_avg_sq", "step", "step_dev", "ema"):
                if key in opt.state.get(p, {}):
                    out[f"{tag}.{k}.{key}"] = opt.state[p][key].detach().clone()
    return out


@pytest.mark.parametrize("level, batch", [(3, 8), (4, 4)])
def test_training_is_bitwise_the_same_with_and_without_the_average(level, batch, monkeypatch):
    off = _run_stepper(level, batch, 0.0, True, monkeypatch)
    on = _run_stepper(level, batch, 0.999, True, monkeypatch)
    eager = _run_stepper(level, batch, 0.999, False, monkeypatch)
    assert not any(k.endswith(".ema") for k in off)
    emas = [k for k in on if k.endswith(".ema")]
    assert emas and all(k.startswith("gen.") for k in emas)           # the critic has no average
    for k, t in off.items():
        assert torch.equal(t.cpu(), on[k].cpu()), f"{k} differs once the generator's weights are averaged"
    assert set(on) - set(off) == set(emas)
    for k in emas:
        assert torch.equal(on[k], eager[k]), f"{k}: graph replay and MG_GRAPHS=0 disagree"
        assert float(on[k[:-4] + ".step"]) == 3.0                     # iterations 0, 5, 10: the third update is a replay
        assert not torch.equal(on[k], on[k[:-4]])


# ------------------------------------------------------------------ 6. growth
def test_new_parameter_groups_start_their_averages_at_their_own_first_step():
    """elementwise float32 torch expressions round as the kernel does (nothing is contracted into an FMA on either side), so the
    expected averages are formed bit for bit"""
    from musicgan_amd import avg_ops
    from musicgan_amd.networks import Generator
    from musicgan_amd.optim import FusedAdam
    decay = 0.9
    w = avg_ops.ema_weight(decay)
    torch.manual_seed(0)
    gen = Generator(8).to(DEV)
    opt = FusedAdam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9), ema_decay=decay)
    rng = torch.Generator(device=DEV).manual_seed(9)

    def step(params):
        for p in gen.parameters():
            p.grad = None
        for p in params:
            p.grad = torch.randn(p.shape, device=DEV, generator=rng)
        opt.step()

    old = list(gen.parameters())
    first = [p.detach().clone() for p in old]
    step(old)
    for p, p0 in zip(old, first):
        assert torch.equal(opt.state[p]["ema"], p0 + (p.detach() - p0) * w)   # started at p0, then one update
    step(old)
    gen.next_layer()
    new = [p for p in gen.end_block_params() if all(p is not q for q in old)]
    assert new and all(p not in opt.state for p in new)
    opt.add_param_group({"params": gen.end_block_params(), "lr": 1e-3, "betas": (0.0, 0.9)})
    live = [p for p in gen.parameters()]
    before = {p: p.detach().clone() for p in live}
    carried = {p: opt.state[p]["ema"].clone() for p in old}
    step(live)
    torch.cuda.synchronize()
    for p in new:
        assert float(opt.state[p]["step"]) == 1.0
        assert torch.equal(opt.state[p]["ema"], before[p] + (p.detach() - before[p]) * w), "a new average must start at the weights"
    for p in old:
        if p in before:     # still a parameter of the grown network
            assert float(opt.state[p]["step"]) == 3.0
            assert torch.equal(opt.state[p]["ema"], carried[p] + (p.detach() - carried[p]) * w), "an old average must carry on"
    sd = opt.averaged_state_dict(gen)
    assert list(sd.keys()) == list(gen.state_dict().keys())
    fresh = Generator(8)
    fresh.next_layer()
    fresh.load_state_dict(sd, strict=True)


# ------------------------------------------------------------------ 7. no host sync
def test_steps_with_the_average_do_not_synchronise_the_host():
    from musicgan_amd.networks import Generator
    from musicgan_amd.optim import FusedAdam
    torch.manual_seed(0)
    gen = Generator(8).to(DEV)
    gen.next_layer()
    opt = FusedAdam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9), ema_decay=0.999)
    grads = {p: torch.randn_like(p) for p in gen.parameters()}
    late = torch.nn.Parameter(torch.randn(33, device=DEV))
    grads[late] = torch.randn_like(late)

    def step():
        for p, g in grads.items():
            p.grad = g
        opt.step()

    step()   # warm-up: library load, first allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            step()
        opt.add_param_group({"params": [late], "lr": 1e-3, "betas": (0.0, 0.9)})   # a group added at growth: its state, its average
        step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert float(opt.state[late]["step"]) == 1.0 and int(opt.state[late]["step_dev"]) == 1
    assert all(int(opt.state[p]["step_dev"]) == 5 for p in gen.parameters())


# ------------------------------------------------------------------ 8. poisoned memory
INPLACE = {"adam_step_ema": ("params", "exp_avg", "exp_avg_sq", "steps", "ema")}   # "Writes all of params[i], exp_avg[i], ..."


@pytest.mark.parametrize("name", ["not a multiple of four", "flat slices at 4-byte offsets", "more tensors than a chunk"])
def test_adam_step_ema_on_poisoned_memory(name):
    """poison.rule over avg_ops.  The wrapper takes lists, which the harness does not re-home, so the case cuts every tensor out of
    a guarded allocation of the harness itself ([guard | payload | guard], guards filled with 0x00 in one run and 0xFF in the
    other): the guards of all of them are checked when the run ends, and the digests of the five written arguments and of the
    gradients (which must come back unchanged) are compared between the fills -- a read or a write outside a tensor shows up in
    one or the other."""
    from musicgan_amd import avg_ops
    sizes = _sets()[name]
    digests = []

    def case(p):
        src = _make(sizes, 41)
        if sizes == "flat":
            # one guarded buffer per array; the slices keep their 4-byte offsets inside it
            lists = []
            for xs in src[:4]:
                base = xs[0].data_ptr() - 4
                flat = p.allocate((1400,), torch.float32, torch.device(DEV), 0)
                views = [flat[(x.data_ptr() - base) // 4:(x.data_ptr() - base) // 4 + x.numel()] for x in xs]
                for dst, x in zip(views, xs):
                    dst.copy_(x)
                lists.append(views)
            pp, g, m, v = lists
        else:
            pp, g, m, v = ([p.allocate(tuple(x.shape), torch.float32, torch.device(DEV), None).copy_(x) for x in xs] for xs in src[:4])
        s = [p.allocate((), torch.int32, torch.device(DEV), 0) for _ in pp]
        ema = [p.allocate(tuple(x.shape), torch.float32, torch.device(DEV), None).copy_(x * 0.5) for x in pp]
        g0 = [x.clone() for x in g]
        for _ in range(3):
            avg_ops.adam_step_ema(pp, g, m, v, s, ema, **HYPER, decay=0.999)
        torch.cuda.synchronize()
        p.check_all("adam_step_ema", name)
        assert all(torch.equal(a, b) for a, b in zip(g, g0)), "the gradients are not declared as written"
        for xs in (pp, m, v, ema):
            assert all(bool(torch.isfinite(x).all()) for x in xs)
        digests.append([poison.hash_bits(x) for xs in (pp, g, m, v, s, ema) for x in xs])

    r0, r1 = poison.rule(case, module=avg_ops, inplace=INPLACE, classes=())
    assert digests[0] == digests[1], "the step depends on memory outside its tensors"
    assert r1.census.ops() >= {"adam_step_ema"} and [n for n, _, _ in r1.calls] == ["adam_step_ema"] * 3


# ------------------------------------------------------------------ 9. end to end
def test_train_with_ema_decay_end_to_end(tmp_path, capsys):
    import musicgan_amd
    from musicgan_amd.networks import Generator
    from musicgan_amd.train import train
    from test_audio_gpu import _tiny_dataset
    data = _tiny_dataset(tmp_path)
    kw = dict(nb_epoch=10, batch_size=2, num_workers=0, save_every=2, rand_channels=8, ema_decay=0.99,
              fadein_lengths=[1, 6, 6, 6, 6, 6, 6, 6], train_lengths=[5, 4, 100, 100, 100, 100, 100])
    torch.manual_seed(123)
    a = tmp_path / "straight"
    train("a", str(data), str(a), max_iters=6, **kw)               # grows after iterations 3 and 5
    files = sorted(f for f in os.listdir(a) if f.endswith(".pt"))
    assert files == sorted(f"{s}_{k}.pt" for s in ("disc", "gen", "gen_ema", "optim_disc", "optim_gen", "train_state") for k in range(3))
    raw, avg = torch.load(str(a / "gen_2.pt")), torch.load(str(a / "gen_ema_2.pt"))
    assert list(raw.keys()) == list(avg.keys())
    gen = Generator(8)
    gen.next_layer()
    gen.next_layer()
    gen.load_state_dict(avg, strict=True)
    moved = [k for k in raw if not torch.equal(raw[k], avg[k])]
    assert moved and all(bool(torch.isfinite(avg[k]).all()) for k in avg)
    osd = torch.load(str(a / "optim_gen_2.pt"))
    assert all("ema" in s for s in osd["state"].values())
    assert all("ema" not in s for s in torch.load(str(a / "optim_disc_2.pt"))["state"].values())
    # interrupted after 4 iterations and resumed: the averages continue bit for bit
    torch.manual_seed(123)
    b = tmp_path / "interrupted"
    train("b", str(data), str(b), max_iters=4, **kw)
    torch.manual_seed(999)
    train("b", str(data), str(b), max_iters=6, resume_from=str(b), **kw)
    for f in ("gen_ema_2.pt", "gen_2.pt"):
        x, y = torch.load(str(a / f)), torch.load(str(b / f))
        assert list(x.keys()) == list(y.keys())
        for k in x:
            assert torch.equal(x[k], y[k]), f"{f} {k} differs after resume"
    oa, ob = osd, torch.load(str(b / "optim_gen_2.pt"))
    assert all(torch.equal(oa["state"][i]["ema"].cpu(), ob["state"][i]["ema"].cpu()) for i in oa["state"])
    # a run that had no averages, resumed with them: they start at the resumed weights
    torch.manual_seed(123)
    c = tmp_path / "late"
    train("c", str(data), str(c), max_iters=4, **{**kw, "ema_decay": 0.0})
    assert not [f for f in os.listdir(c) if f.startswith("gen_ema")]
    train("c", str(data), str(c), max_iters=5, resume_from=str(c), **{**kw, "save_every": 1})   # iteration 4: no generator update
    x, y = torch.load(str(c / "gen_2.pt")), torch.load(str(c / "gen_ema_2.pt"))
    assert all(torch.equal(x[k], y[k]) for k in x)
    # evaluate takes the averaged checkpoint as it takes the raw one
    capsys.readouterr()
    res = musicgan_amd.evaluate(str(a / "gen_ema_2.pt"), 8, str(data), level=2, nb_images=6, batch_size=3, seed=1)
    res_raw = musicgan_amd.evaluate(str(a / "gen_2.pt"), 8, str(data), level=2, nb_images=6, batch_size=3, seed=1)
    assert list(res) == list(res_raw) and all(v == v for v in res.values())
    # generate needs a fully grown network: one level per iteration up to level 7, generator updates at iterations 0, 5, 10
    torch.manual_seed(5)
    d = tmp_path / "grown"
    train("d", str(data), str(d), max_iters=11, **{**kw, "save_every": 11, "fadein_lengths": [1] + [4] * 7, "train_lengths": [2] * 7})
    assert torch.load(str(d / "train_state_0.pt"))["level"] == 7
    musicgan_amd.generate(str(tmp_path / "sound"), 8, str(d / "gen_ema_0.pt"), 1, 1)
    from musicgan_amd.audio import wavio
    wav, sr = wavio.load(str(tmp_path / "sound" / "sound_0.wav"))
    assert sr == 44100 and bool(torch.isfinite(wav).all())

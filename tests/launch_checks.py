"""Per-launch checks of a training step, independent of the configuration: the routing census of one critic + one generator update
at (level, batch), and for every kind of launch a float64 host restatement of the same operation (F.conv2d / F.conv_transpose2d /
F.avg_pool2d / F.interpolate / autograd) that the launch is compared with element by element, at exactly the recorded shape and
flags, on inputs seeded by the crc32 of the record's line.  test_headline_shapes_gpu.py (level 5, batch 64) commits the records
of its step and runs these checks; nothing here depends on that configuration, so a file for another (level, batch) needs only its
own committed lists.  The bounds are those of each kernel's per-op test and are stated where they are applied.

`check_launch(line, hook)` / `check_sweep(lines, key, hook)`: `hook(what, got, delta)` (optional) is called with every tensor a
check is about to compare -- `what` names the comparison; `delta` is 4 x its bound x max|reference| (for an exact comparison of
floats: 4 float32 epsilons of max|reference|), for a tile mask compared with float64 signs a uint8 tensor of got's shape holding
per byte the bit of the tile's pixel that is farthest from zero, for a mask compared bit for bit None -- and what it returns is
compared in place of `got`: a test may change a VALUE the kernel produced (never a shape or an address; the kernel runs as
always) to see that the comparison notices."""
import contextlib
import math
import zlib

import torch
import torch.nn.functional as F

from routing_census import census, parse, spec
from test_ops_gpu import report
from test_wino_strip_gpu import _tile_mask

DEV = "cuda:0"
SLOPE = 0.2
CHUNK = 16  # images per slice of the float64 reference ...
SLICE = 16 * 64 * 128 * 128  # ... and at most this many elements (16 images of the headline's largest map; 2 of 32 x 512 x 512)

# not kernel launches of the step (host queries, the weight packing -- test_pack_multi_equals_single_tensor_packs) or launches covered
# as a whole sweep (the weight gradients and their one-launch reduction: test_weight_gradient_sweep)
NOT_PER_LAUNCH = {"packed_floats", "wino_wgrad_form", "wgrad_group_chunks", "fuse_ends", "workspace", "pack_multi", "WgradDefer.flush",
                  "conv3x3_wgrad"}


def _ops():
    from musicgan_amd import ops
    return ops


def _launch(name: str) -> bool:
    return not name.endswith("_supported") and name not in NOT_PER_LAUNCH


def step_census(monkeypatch, level, batch, fused_d_step=True):
    """The routing census of one critic + one generator update at (level, batch), alpha 0.5 (eager: MG_GRAPHS=0);
    `fused_d_step=False`: through the modules and autograd instead of the two fused steps."""
    import bench
    from musicgan_amd.optim import FusedAdam
    from musicgan_amd.train_step import ProGANStepper
    monkeypatch.setenv("MG_GRAPHS", "0")
    gen, disc = bench.build_nets(level, 32, DEV)
    og = FusedAdam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9))
    od = FusedAdam(disc.parameters(), lr=1e-3, betas=(0.0, 0.9))
    st = ProGANStepper(gen, disc, og, od, 32, fused_d_step=fused_d_step)
    side = 4 << level  # bench.LEVEL_SIDE where that has the level (test_launch_checks_cpu.py); levels 0-2 are below its table
    rng = torch.Generator(device=DEV).manual_seed(1234)
    x_real = torch.rand(batch, 2, side, side, device=DEV, generator=rng) * 2 - 1
    z = torch.randn(batch, 32, 2, 2, device=DEV, generator=rng)
    eps = torch.rand(batch, 1, 1, 1, device=DEV, generator=rng)
    with census() as c:
        st.d_step(x_real, 0.5, z=z, eps=eps)
        st.g_step(batch, 0.5, DEV, z=z)
        torch.cuda.synchronize()
    return c


def sweeps_of(calls):
    """The deferred weight-gradient layers of each `WgradDefer.flush`, in call order."""
    out, cur = [], []
    for rec in calls:
        if rec[0] == "conv3x3_wgrad":
            cur.append(spec(rec))
        elif rec[0] == "WgradDefer.flush":
            out.append(cur)
            cur = []
    assert not cur, "weight gradients left outside a flushed sweep"
    return out


# ------------------------------------------------------------------ float64 references
def _gen(line: str) -> torch.Generator:
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(line.encode()))


def _host(t, i0=None, i1=None):
    return (t if i0 is None else t[i0:i1]).detach().double().cpu()


def _slope(act):
    return torch.where(act > 0, 1.0, SLOPE).double()


def _slope_of_bits(m):
    """uint8 tile mask (N,C,H/2,W/2), bit 2i+j <-> pixel (2Y+i, 2X+j) -> the LeakyReLU derivative (N,C,H,W) it stands for."""
    n, c, h, w = m.shape
    b = torch.stack([(m.long() >> k) & 1 for k in range(4)], dim=-1).reshape(n, c, h, w, 2, 2)
    return torch.where(b.permute(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * h, 2 * w) > 0, 1.0, SLOPE).double()


def _up2(t):
    return F.interpolate(t, scale_factor=2, mode="nearest")


def _pn(act):
    rn = 1.0 / torch.sqrt((act * act).mean(dim=1, keepdim=True) + 1e-8)
    return act * rn, rn


# the hook of the check in progress: a module global because the comparisons sit at the bottom of every check function; set only
# inside `_hooked`, which check_launch / check_sweep enter (check_sweep after its kernels have run: only comparisons see it)
_hook = None


@contextlib.contextmanager
def _hooked(hook):
    global _hook
    before, _hook = _hook, hook
    try:
        yield
    finally:
        _hook = before


def _slices(n, per_image):
    step = max(1, min(CHUNK, SLICE // max(per_image, 1)))
    return [(i0, min(n, i0 + step)) for i0 in range(0, n, step)]


def _report(what, got, ref, tol):
    """test_ops_gpu.report (max-norm relative error of the whole tensor), behind the hook."""
    if _hook is not None:
        got = _hook(what, got, 4 * tol * float(ref.detach().abs().max()))
    return report(what, got, ref, tol)


def _check(what, got, ref_fn, tol):
    """Max-norm relative error of the GPU tensor `got` (images along dim 0) against ref_fn(i0, i1), the float64 host reference of
    images i0:i1, computed slice by slice over EVERY image; the failure names the worst image."""
    n = got.shape[0]
    refs = {}
    if _hook is not None:  # the scale of the whole reference first; its slices are kept, not computed again
        refs = {i0: ref_fn(i0, i1) for i0, i1 in _slices(n, got[0].numel())}
        got = _hook(what, got, 4 * tol * max(float(r.abs().max()) for r in refs.values()))
    err, scale, worst = 0.0, 0.0, -1
    for i0, i1 in _slices(n, got[0].numel()):
        r = refs.pop(i0) if refs else ref_fn(i0, i1)
        e = (_host(got, i0, i1) - r).abs().reshape(i1 - i0, -1).max(dim=1).values
        k = int(e.argmax())
        if float(e[k]) > err:
            err, worst = float(e[k]), i0 + k
        scale = max(scale, float(r.abs().max()))
    assert err <= tol * scale, f"{what}: max-norm rel err {err / max(scale, 1e-30):.3e} > {tol:.1e} (worst image {worst} of {n})"


def _farthest_bit(act):
    """Per 2x2 tile of the activation (N,C,H,W): the tile-mask bit (1 << 2i+j, uint8 (N,C,H/2,W/2)) of its pixel farthest from zero."""
    n, c, h, w = act.shape
    t = act.abs().reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    return (1 << t.argmax(dim=-1)).to(torch.uint8)


def _equal(what, got, want):
    """An exact comparison, behind the hook: bit for bit for a tile mask, value for value for floats."""
    if _hook is not None:
        got = _hook(what, got, None if got.dtype == torch.uint8 else 4 * torch.finfo(torch.float32).eps * float(want.abs().max()))
    assert torch.equal(got, want), f"{what}: differs from the reference in {int((got != want).sum())} of {got.numel()} places"


def _check_tile_mask(what, m, act_fn):
    """Tile-mask bits against the sign of the float64 activation, wherever that is not within round-off (1e-5 of its scale) of 0."""
    n = m.shape[0]
    acts = {}
    if _hook is not None:
        acts = {i0: act_fn(i0, i1) for i0, i1 in _slices(n, 4 * m[0].numel())}
        m = _hook(what, m, torch.cat([_farthest_bit(a) for a in acts.values()]))
    for i0, i1 in _slices(n, 4 * m[0].numel()):
        a = acts.pop(i0) if acts else act_fn(i0, i1)
        s = 1e-5 * float(a.abs().max())
        ok = (m[i0:i1].cpu() == _tile_mask(a)) | (_tile_mask(a + s) != _tile_mask(a - s))
        assert bool(ok.all()), f"{what}: tile-mask bits differ from the float64 sign in images {i0}..{i1 - 1}"


def _weight(g, co, ci):
    return torch.randn(co, ci, 3, 3, device=DEV, generator=g) / math.sqrt(9 * ci)


def _inputs(g, a, skip=()):
    """Seeded tensors for the recorded shapes: N(0,1) fp32, uniform tile-mask bytes for u8 shapes."""
    out = {}
    for k, v in a.items():
        if k in skip:
            continue
        if isinstance(v, tuple) and v and v[0] == "u8":
            out[k] = torch.randint(0, 16, v[1:], device=DEV, generator=g, dtype=torch.uint8)
        elif isinstance(v, tuple):
            out[k] = torch.randn(v, device=DEV, generator=g)
        else:
            out[k] = v
    return out


# ------------------------------------------------------------------ 3x3 convolutions: direct, Winograd (strip / staged), small-map
def _check_conv(name, a, g):
    ops = _ops()
    n, cin = a["x"][0], a["x"][1]
    cout = a["cout"]
    pk = "wpk" if name == "conv3x3_small" else ("wino" if a.get("wino") is not None else "wp")
    ups = a.get("ups", False)
    pooled = a.get("pool", False) or a.get("pool_out") is not None
    # the engine's data-gradient convs: no bias, no activation, no pool, a fresh output (a tangent conv writes over its mask)
    dgrad = a.get("bias") is None and not a.get("lrelu", False) and not pooled and a.get("out") is None
    w = _weight(g, cin, cout) if dgrad else _weight(g, cout, cin)
    pack = {"wino": ops.pack_wino3x3, "wp": ops.pack_conv3x3, "wpk": ops.pack_smallnet}[pk](w, dgrad)
    assert pack.numel() == a[pk][0]
    kw = _inputs(g, a, skip=(pk, "out", "pool_out"))
    kw[pk] = pack
    mask = kw.get("mask_aux")
    mask0 = mask.clone() if mask is not None else None
    if a.get("out") is not None:
        kw["out"] = mask if mask is not None and mask.dtype == torch.float32 and tuple(mask.shape) == a["out"] else \
            torch.empty(a["out"], device=DEV)
    if a.get("pool_out") is not None:
        kw["pool_out"] = torch.full(a["pool_out"], float("nan"), device=DEV)
    res = getattr(ops, name)(**kw)
    w64, b64 = _host(w), (_host(kw["bias"]) if kw.get("bias") is not None else None)
    xs = kw["x"]

    def pre(i0, i1):
        xi = _host(xs, i0, i1)
        if ups:
            xi = _up2(xi)
        return F.conv_transpose2d(xi, w64, padding=1) if dgrad else F.conv2d(xi, w64, b64, padding=1)

    act = (lambda i0, i1: F.leaky_relu(pre(i0, i1), SLOPE)) if a.get("lrelu") else pre
    small = name == "conv3x3_small"
    t_main = 3e-6 if small and (mask is not None or dgrad) else 2e-6
    t_pool = 3e-6 if pk == "wp" else 2e-6
    if a.get("unpool_mask") is not None:
        um = kw["unpool_mask"]
        _check(f"{name} un-pooled", res, lambda i0, i1: 0.25 * _up2(pre(i0, i1)) * _slope_of_bits(um[i0:i1].cpu()), 2e-6)
    elif a.get("unpool_aux") is not None:
        ua = kw["unpool_aux"]
        _check(f"{name} un-pooled", res, lambda i0, i1: 0.25 * _up2(pre(i0, i1)) * _slope(_host(ua, i0, i1)), 3e-6)
    elif a.get("upsum"):
        _check(f"{name} block sums", res[1], lambda i0, i1: 4.0 * F.avg_pool2d(pre(i0, i1), 2), 3e-6)
    elif a.get("mask_out"):
        m, p = res
        _check(f"{name} pooled", p, lambda i0, i1: F.avg_pool2d(act(i0, i1), 2), t_pool)
        _check_tile_mask(f"{name} tile mask", m, act)
    elif mask is not None:
        sl = (lambda i0, i1: _slope_of_bits(mask0[i0:i1].cpu())) if mask.dtype == torch.uint8 else \
            (lambda i0, i1: _slope(_host(mask0, i0, i1)))
        y_ref = lambda i0, i1: pre(i0, i1) * sl(i0, i1)
        y, p = res if pooled else (res, None)
        if y is not None:
            if kw.get("out") is not None:
                assert y is kw["out"]
            _check(f"{name} masked", y, y_ref, t_main)
        if p is not None:
            assert a.get("pool_out") is None or p is kw["pool_out"]
            _check(f"{name} masked pooled", p, lambda i0, i1: F.avg_pool2d(y_ref(i0, i1), 2), 3e-6 if small else t_pool)
    elif a.get("pixnorm"):
        y, p, rn = res
        if y is not None:
            _check(f"{name} y", y, act, 2e-6)
        _check(f"{name} p", p, lambda i0, i1: _pn(act(i0, i1))[0], 3e-6)
        _check(f"{name} rn", rn, lambda i0, i1: _pn(act(i0, i1))[1], 3e-6)
    elif pooled:
        y, p = res
        _check(f"{name} y", y, act, 2e-6)
        _check(f"{name} pooled", p, lambda i0, i1: F.avg_pool2d(act(i0, i1), 2), t_pool)
    else:
        _check(name, res, act, t_main)


def _check_conv_fade(a, g):
    from musicgan_amd import _lib
    ops = _ops()
    n, cin = a["x"][0], a["x"][1]
    cout, mode = a["cout"], a["mode"]
    bwd = mode == _lib.MG_FADE_BWD
    w = _weight(g, cin, cout) if bwd else _weight(g, cout, cin)
    kw = _inputs(g, a, skip=("wino", "coef", "out"))
    kw["wino"] = ops.pack_wino3x3(w, bwd)
    assert kw["wino"].numel() == a["wino"][0]
    kw["coef"] = torch.tensor([0.37, 0.63], device=DEV)
    if a.get("out") is not None:
        kw["out"] = torch.empty(a["out"], device=DEV)
    res = ops.conv3x3_fade(**kw)
    w64, b64 = _host(w), (_host(kw["bias"]) if kw.get("bias") is not None else None)
    x, other, m_in = kw["x"], kw["other"], kw.get("mask_in")
    pre = (lambda i0, i1: F.conv_transpose2d(_host(x, i0, i1), w64, padding=1)) if bwd else \
        (lambda i0, i1: F.conv2d(_host(x, i0, i1), w64, b64, padding=1))
    if mode == _lib.MG_FADE_FWD:
        act = lambda i0, i1: F.leaky_relu(pre(i0, i1), SLOPE)
        _check("fade blend", res[0], lambda i0, i1: 0.37 * act(i0, i1) + 0.63 * _host(other, i0, i1), 2e-6)
        _check_tile_mask("fade tile mask", res[1], act)
    elif mode == _lib.MG_FADE_TANGENT:
        assert res is kw["out"]
        _check("fade tangent", res, lambda i0, i1: 0.37 * pre(i0, i1) * _slope_of_bits(m_in[i0:i1].cpu()) + 0.63 * _host(other, i0, i1), 2e-6)
    else:
        _check("fade bwd new", res[0], lambda i0, i1: 0.37 * pre(i0, i1) * _slope_of_bits(m_in[i0:i1].cpu()), 2e-6)
        _check("fade bwd old", res[1], lambda i0, i1: 0.63 * pre(i0, i1) * _slope(_host(other, i0, i1)), 2e-6)


# ------------------------------------------------------------------ Upsample(x2) -> Conv3x3: 9-component Winograd, sub-pixel
def _check_upconv(name, a, g):
    ops = _ops()
    ci, co = a["x"][1], a["cout"]
    w = _weight(g, co, ci)
    pk = "up" if name.startswith("winoups") else "wp"
    kw = _inputs(g, a, skip=(pk, "hw", "hb", "mp_out"))
    kw[pk] = ops.pack_winoups3x3(w, False) if pk == "up" else ops.pack_upconv3x3(w)
    assert kw[pk].numel() == a[pk][0]
    x, w64, b64 = kw["x"], _host(w), _host(kw["bias"])
    act = lambda i0, i1: F.leaky_relu(F.conv2d(_up2(_host(x, i0, i1)), w64, b64, padding=1), SLOPE)
    if name == "winoups3x3_head":
        hw = torch.randn(2, co, 1, 1, device=DEV, generator=g) / math.sqrt(co)
        hb = torch.randn(2, device=DEV, generator=g) * 0.1
        kw["hw"], kw["hb"] = hw, hb
        y, p, rn, mp = ops.winoups3x3_head(**kw)
        _check("winoups3x3_head p", p, lambda i0, i1: _pn(act(i0, i1))[0], 3e-6)
        _check("winoups3x3_head rn", rn, lambda i0, i1: _pn(act(i0, i1))[1], 3e-6)
        # the head on the kernel's own p, absolute (tanh in [-1, 1]): test_forward_with_the_head_in_the_epilogue
        head = lambda i0, i1: torch.tanh(F.conv2d(_host(p, i0, i1), _host(hw), _host(hb)))
        sl = _slices(mp.shape[0], p[0].numel())
        if _hook is not None:
            mp = _hook("winoups3x3_head mp", mp, 4 * 2e-6 * max(float(head(i0, i1).abs().max()) for i0, i1 in sl))
        err = max(float((_host(mp, i0, i1) - head(i0, i1)).abs().max()) for i0, i1 in sl)
        assert err <= 2e-6, f"winoups3x3_head mp: {err:.3e}"
        return
    y, p, rn = getattr(ops, name)(**kw)
    t_y, t_p = (2e-6, 3e-6) if pk == "up" else (3e-6, 4e-6)
    if y is not None:
        _check(f"{name} y", y, act, t_y)
    _check(f"{name} p", p, lambda i0, i1: _pn(act(i0, i1))[0], t_p)
    _check(f"{name} rn", rn, lambda i0, i1: _pn(act(i0, i1))[1], t_p)


def _check_winoups_dgrad(name, a, g):
    ops = _ops()
    co, ci = a["gy"][1], a["cin"]
    w = _weight(g, co, ci)
    kw = _inputs(g, a, skip=("up", "p", "rn"))
    kw["up"] = ops.pack_winoups3x3(w, True)
    assert kw["up"].numel() == a["up"][0]
    gy, w64 = kw["gy"], _host(w)
    gx = lambda i0, i1: 4.0 * F.avg_pool2d(F.conv_transpose2d(_host(gy, i0, i1), w64, padding=1), 2)  # autograd of up2 -> conv
    if name == "winoups3x3_dgrad":
        _check(name, ops.winoups3x3_dgrad(**kw), gx, 3e-6)
        return
    p = torch.randn(a["p"], device=DEV, generator=g)
    rn = torch.rand(a["rn"], device=DEV, generator=g) + 0.5
    kw["p"], kw["rn"] = p, rn
    got = ops.winoups3x3_dgrad_pn(**kw)

    def ref(i0, i1):  # PixelNorm + LeakyReLU backward from the normalised output (test_pixelnorm_bwd_small_maps, from_p)
        g64, p64, rn64 = gx(i0, i1), _host(p, i0, i1), _host(rn, i0, i1)
        return _slope(p64) * rn64 * (g64 - p64 * (g64 * p64).mean(dim=1, keepdim=True))
    _check(name, got, ref, 3e-6)
    # and the bound of test_data_gradient_matches_autograd: against the two launches it replaces
    _report(f"{name} vs dgrad + pixelnorm_lrelu_bwd", got, ops.pixelnorm_lrelu_bwd(ops.winoups3x3_dgrad(gy, kw["up"], ci), p, rn, from_p=True), 2e-6)


def _check_small_pn(a, g):
    ops = _ops()
    c, co = a["x_raw"][1], a["cout"]
    w = _weight(g, co, c)
    kw = _inputs(g, a, skip=("wpk",))
    kw["wpk"] = ops.pack_smallnet(w, False)
    assert kw["wpk"].numel() == a["wpk"][0]
    y, p, rn = ops.conv3x3_small_pn(**kw)
    x, w64, b64 = kw["x_raw"], _host(w), _host(kw["bias"])
    pn = lambda i0, i1: _pn(_host(x, i0, i1))
    src = (lambda i0, i1: _up2(pn(i0, i1)[0])) if a.get("ups") else (lambda i0, i1: pn(i0, i1)[0])
    _check("conv3x3_small_pn y", y, lambda i0, i1: F.leaky_relu(F.conv2d(src(i0, i1), w64, b64, padding=1), SLOPE), 3e-6)
    if a.get("save", True):
        _check("conv3x3_small_pn p", p, lambda i0, i1: pn(i0, i1)[0], 2e-6)
        _check("conv3x3_small_pn rn", rn, lambda i0, i1: pn(i0, i1)[1], 2e-6)
    else:
        assert p is None and rn is None


# ------------------------------------------------------------------ the fade-in ends and the generator head (fade_ends.hip)
def _check_ends(name, a, g):
    ops = _ops()
    kw = _inputs(g, a)
    h = _host
    c1x1 = lambda x, w, b=None: F.conv2d(x, h(w), None if b is None else h(b))
    if name == "stem_pair" and a.get("masked"):
        h0_act, o_act = kw["h0"].clone(), kw["o"].clone()
        ops.stem_pair(**kw)
        u = h(kw["x"])
        _report("stem_pair tangent h0", kw["h0"], c1x1(u, kw["ws"]) * _slope(h(h0_act)), 2e-6)
        _report("stem_pair tangent xp", kw["xp"], F.avg_pool2d(u, 2), 2e-6)
        _report("stem_pair tangent o", kw["o"], c1x1(F.avg_pool2d(u, 2), kw["wo"]) * _slope(h(o_act)), 2e-6)
    elif name == "stem_pair":
        h0, xp, o, *hm = ops.stem_pair(**kw)  # (the tile mask only with want_mask)
        x = kw["x"]
        ref_h0 = lambda i0, i1: F.leaky_relu(c1x1(h(x, i0, i1), kw["ws"], kw["bs"]), SLOPE)
        _check("stem_pair h0", h0, ref_h0, 2e-6)
        _check("stem_pair xp", xp, lambda i0, i1: F.avg_pool2d(h(x, i0, i1), 2), 2e-6)
        _check("stem_pair o", o, lambda i0, i1: F.leaky_relu(c1x1(F.avg_pool2d(h(x, i0, i1), 2), kw["wo"], kw["bo"]), SLOPE), 2e-6)
        assert len(hm) == int(a.get("want_mask", False))
        if hm:
            _equal("stem_pair mask", hm[0], _tile_mask(h0))  # the bits of its own h0 (test_stem_pair_forward_and_tangent)
    elif name == "stem_pair_gx":
        gs, go = kw["gs"], kw["go"]
        _check("stem_pair_gx", ops.stem_pair_gx(**kw), lambda i0, i1: F.conv_transpose2d(h(gs, i0, i1), h(kw["ws"])) +
               0.25 * _up2(F.conv_transpose2d(h(go, i0, i1), h(kw["wo"]))), 3e-6)
    elif name == "head_pair":
        # the separate-heads form of the fade-in output (the last conv did not take the head in its epilogue): bounds of
        # test_head_pair_and_blend_backward
        kw["wh"], kw["wo"] = kw["wh"] / math.sqrt(a["wh"][1]), kw["wo"] / math.sqrt(a["wo"][1])
        if a.get("out") is not None:
            kw["out"] = torch.full(a["out"], float("nan"), device=DEV)
        out, mp, old = ops.head_pair(**kw)
        assert a.get("out") is None or out is kw["out"]
        mp_ref = lambda i0, i1: torch.tanh(c1x1(h(kw["x"], i0, i1), kw["wh"], kw["bh"]))
        old_ref = lambda i0, i1: torch.tanh(c1x1(h(kw["xl"], i0, i1), kw["wo"], kw["bo"]))
        if a.get("save", True):
            _check("head_pair mp", mp, mp_ref, 3e-6)
            _check("head_pair old", old, old_ref, 3e-6)
        else:
            assert mp is None and old is None
        _check("head_pair out", out, lambda i0, i1: a["a"] * mp_ref(i0, i1) + a["b"] * _up2(old_ref(i0, i1)), 3e-6)
    elif name == "head_pair_from_mp":
        kw["mp"] = torch.tanh(kw["mp"])
        kw["wo"] = kw["wo"] / math.sqrt(a["wo"][1])
        if a.get("out") is not None:
            kw["out"] = torch.empty(a["out"], device=DEV)
        out, old = ops.head_pair_from_mp(**kw)
        old_ref = lambda i0, i1: torch.tanh(c1x1(h(kw["xl"], i0, i1), kw["wo"], kw["bo"]))
        if old is not None:
            _check("head_pair_from_mp old", old, old_ref, 3e-6)
        _check("head_pair_from_mp out", out, lambda i0, i1: a["a"] * h(kw["mp"], i0, i1) + a["b"] * _up2(old_ref(i0, i1)), 3e-6)
    elif name == "gen_head_bwd":
        # consistent inputs as test_gen_head_bwd_matches_the_three_launches_and_autograd: p, rn, mp of one y, float64 autograd
        n, c = a["p"][0], a["p"][1]
        y = torch.randn(a["p"], device=DEV, generator=g).double().cpu().requires_grad_(True)
        wt = (torch.randn(a["w"], device=DEV, generator=g).double().cpu() / math.sqrt(c)).requires_grad_(True)
        bt = torch.randn(2, device=DEV, generator=g).double().cpu().requires_grad_(True)
        g_mp = torch.randn(a["g_mp"], device=DEV, generator=g)
        g_in = torch.randn(a["g_in"], device=DEV, generator=g) if a.get("g_in") is not None else None
        p, rn = _pn(F.leaky_relu(y, SLOPE))
        mp = torch.tanh(F.conv2d(p, wt, bt))
        loss = (mp * g_mp.double().cpu()).sum() + ((p * g_in.double().cpu()).sum() if g_in is not None else 0.0)
        loss.backward()
        gw, gb = torch.full(a["gw"], float("nan"), device=DEV), torch.full(a["gb"], float("nan"), device=DEV)
        f = lambda t: t.detach().float().to(DEV)
        gpre = ops.gen_head_bwd(g_mp, f(mp), f(wt), f(p), f(rn), gw, gb, accumulate=a.get("accumulate", False), g_in=g_in)
        _report("gen_head_bwd gpre", gpre, y.grad, 5e-6)
        _report("gen_head_bwd gw", gw, wt.grad, 5e-6)
        _report("gen_head_bwd gb", gb, bt.grad, 5e-6)
    elif name == "blend_up_bwd":
        gx, gy = ops.blend_up_bwd(**kw)
        _report("blend_up_bwd a g", gx, a["a"] * h(kw["g"]), 1e-6)
        _report("blend_up_bwd b sums", gy, a["b"] * 4.0 * F.avg_pool2d(h(kw["g"]), 2), 2e-6)


# ------------------------------------------------------------------ the lone 1x1 convs of level 0, where neither end has a partner to
# fuse with: the critic's stem (2 -> C, LeakyReLU), its tangent form (bias-free, times the LeakyReLU derivative of the saved
# activation, written over it), its data gradient (C -> 2 with w^T) and the generator's head (C -> 2, tanh)
def _check_conv1x1(name, a, g):
    ops = _ops()
    known = {"x", "w", "bias", "cout", "lrelu", "tanh", "mask_aux", "transposed", "out"}
    assert set(a) <= known and sum(bool(a.get(k)) for k in ("lrelu", "tanh", "transposed")) + (a.get("mask_aux") is not None) == 1, \
        f"no headline-shape check for conv1x1 with {sorted(set(a) - {'x', 'w', 'bias', 'cout'})}"
    kw = _inputs(g, a, skip=("out",))
    kw["w"] = kw["w"] / math.sqrt(a["x"][1])  # pre-activations of order 1: tanh neither saturated nor linear
    mask = kw.get("mask_aux")
    mask0 = mask.clone() if mask is not None else None
    if a.get("out") is not None:
        # the tangent pass writes over the activation it reads its mask from (disc_step_fused); any other `out` is written in full
        kw["out"] = mask if mask is not None and tuple(mask.shape) == a["out"] else torch.full(a["out"], float("nan"), device=DEV)
    got = ops.conv1x1(**kw)
    assert a.get("out") is None or got is kw["out"]
    assert tuple(got.shape) == (a["x"][0], a["cout"]) + tuple(a["x"][2:])
    x, w64 = kw["x"], _host(kw["w"])
    b64 = _host(kw["bias"]) if kw.get("bias") is not None else None
    # bounds of test_conv1x1_all_modes: "stem" and "stem tangent" 2e-6, "head" and "stem dgrad" 3e-6
    if a.get("transposed"):
        assert b64 is None
        _check("conv1x1 transposed", got, lambda i0, i1: F.conv_transpose2d(_host(x, i0, i1), w64), 3e-6)
    elif a.get("tanh"):
        _check("conv1x1 tanh", got, lambda i0, i1: torch.tanh(F.conv2d(_host(x, i0, i1), w64, b64)), 3e-6)
    elif a.get("lrelu"):
        _check("conv1x1 lrelu", got, lambda i0, i1: F.leaky_relu(F.conv2d(_host(x, i0, i1), w64, b64), SLOPE), 2e-6)
    else:
        _check("conv1x1 masked", got, lambda i0, i1: F.conv2d(_host(x, i0, i1), w64, b64) * _slope(_host(mask0, i0, i1)), 2e-6)


# ------------------------------------------------------------------ the kernels without an off switch (on both sides of
# test_full_size_step_is_algorithm_independent): PixelNorm, up-sampling / pooling, LeakyReLU, classifier, penalty, 1x1 weight gradient
def _check_elementwise(name, a, g):
    ops = _ops()
    kw = _inputs(g, a, skip=("out",))
    h = _host
    if a.get("out") is not None:
        kw["out"] = torch.empty(a["out"], device=DEV)
    if name == "pixelnorm_fwd":
        p, rn = ops.pixelnorm_fwd(**kw)
        _report("pixelnorm p", p, _pn(h(kw["y"]))[0], 3e-6)
        _report("pixelnorm rn", rn, _pn(h(kw["y"]))[1], 3e-6)
    elif name == "pixelnorm_lrelu_bwd":
        assert a.get("from_p")
        kw["rn"] = torch.rand(a["rn"], device=DEV, generator=g) + 0.5
        gp, p64, rn64 = h(kw["gp"]), h(kw["y"]), h(kw["rn"])
        _report("pixelnorm_lrelu_bwd", ops.pixelnorm_lrelu_bwd(**kw), _slope(p64) * rn64 * (gp - p64 * (gp * p64).mean(dim=1, keepdim=True)), 2e-6)
    elif name == "upsample2x_fwd":
        _equal("upsample2x_fwd", ops.upsample2x_fwd(**kw).cpu(), _up2(kw["x"].cpu()))
    elif name == "upsample2x_bwd":
        _report("upsample2x_bwd", ops.upsample2x_bwd(**kw), 4.0 * F.avg_pool2d(h(kw["gy"]), 2), 1e-6)
    elif name == "avgpool2_bwd":
        act = kw["act"]
        sl = _slope_of_bits(act.cpu()) if act.dtype == torch.uint8 else _slope(h(act))
        _report("avgpool2_bwd", ops.avgpool2_bwd(**kw), 0.25 * _up2(h(kw["gy"])) * sl, 1e-6)
    elif name == "lrelu_bwd":
        _report("lrelu_bwd", ops.lrelu_bwd(**kw), h(kw["g"]) * _slope(h(kw["act"])), 1e-7)
    elif name == "linear1_fwd":
        _report("linear1_fwd", ops.linear1_fwd(**kw), F.linear(h(kw["x"]), h(kw["w"]), h(kw["b"])), 2e-6)
    elif name == "linear1_bwd":
        gx = ops.linear1_bwd(**kw)
        gy = h(kw["gy"])
        if a.get("need_gx", True):
            _report("linear1_bwd gx", gx, gy @ h(kw["w"]), 1e-6)
        if kw.get("gw") is not None:
            _report("linear1_bwd gw", kw["gw"], gy.t() @ h(kw["x"]), 2e-6)
        if kw.get("gb") is not None:
            _report("linear1_bwd gb", kw["gb"], gy[:a.get("bias_n", 0) or gy.shape[0]].sum().reshape(1), 2e-6)
    elif name == "axpby":
        assert a.get("coef") is None
        if a.get("out") is not None:
            kw["out"].fill_(float("nan"))
        got = ops.axpby(**kw)
        assert a.get("out") is None or got is kw["out"]
        _report("axpby", got, a["a"] * h(kw["x"]) + (a["b"] * h(kw["y"]) if kw.get("y") is not None else 0.0), 1e-6)
    elif name == "blend_lrelu_bwd":
        # bit for bit lrelu_bwd(axpby(c, g), act) (test_blend_lrelu_bwd_equals_the_four_kernels_it_replaces): axpby's bound, the
        # factor 1 or 0.2 behind it adds one rounding
        assert a.get("coef") is None
        ga, go = ops.blend_lrelu_bwd(**kw)
        _report("blend_lrelu_bwd new", ga, a["ca"] * h(kw["g"]) * _slope(h(kw["act_a"])), 1e-6)
        _report("blend_lrelu_bwd old", go, a["co"] * h(kw["g"]) * _slope(h(kw["act_o"])), 1e-6)
    elif name == "gp_interp":
        kw["eps"] = torch.rand(a["eps"], device=DEV, generator=g)
        e = h(kw["eps"])
        _report("gp_interp", ops.gp_interp(**kw), e * h(kw["x_real"]) + (1 - e) * h(kw["x_fake"]), 1e-6)
    elif name == "sumsq_per_sample":
        _report("sumsq_per_sample", ops.sumsq_per_sample(**kw), h(kw["g"]).pow(2).sum(dim=(1, 2, 3)), 2e-6)
    elif name == "gp_apply":
        n = a["g"][0]
        kw["g"] = kw["g"] * 0.01  # per-sample norms around 1: (||g|| - 1) of both signs
        kw["sumsq"] = h(kw["g"]).pow(2).sum(dim=(1, 2, 3)).float().to(DEV)
        pen, out = ops.gp_apply(**kw)
        nrm = h(kw["sumsq"]).sqrt()
        f, up = a["factor"], a.get("upstream", 1.0)
        _report("gp_apply penalty", pen, f * ((nrm - 1) ** 2).mean(), 2e-6)
        _report("gp_apply out", out, h(kw["g"]) * (up * f * 2 * (nrm - 1) / (n * nrm)).reshape(n, 1, 1, 1), 3e-6)
    elif name == "group_means":
        kw["scores"] = kw["scores"] * 7
        out = h(ops.group_means(**kw))
        gr = a["groups"]
        m = h(kw["scores"]).reshape(gr, -1).mean(dim=1)
        want = float(m[1] - m[0]) if gr >= 2 else float(-m[0])
        means, diff = out[:gr], out[gr:gr + 1]
        if _hook is not None:
            means = _hook("group_means means", means, 4 * 1e-6 * float(m.abs().max() + 1))
            diff = _hook("group_means difference", diff, 4 * 2e-6 * (abs(want) + 1))
        assert float((means - m).abs().max()) <= 1e-6 * float(m.abs().max() + 1), "group_means means"
        assert abs(float(diff[0]) - want) <= 2e-6 * (abs(want) + 1), "group_means difference"
    elif name == "conv1x1_wgrad":
        kw["gw"], kw["gb"] = torch.full(a["gw"], float("nan"), device=DEV), torch.full(a["gb"], float("nan"), device=DEV)
        ops.conv1x1_wgrad(**kw)
        bn = a.get("bias_n", 0) or a["x"][0]
        ref_w = torch.einsum("nohw,nchw->oc", h(kw["gy"]), h(kw["x"]))
        ref_b = h(kw["gy"], 0, bn).sum(dim=(0, 2, 3))
        # reduction over N H W = 3.1 M pixels: twice plain fp32's own deviation from float64 where that exceeds the bound
        w32 = torch.nn.grad.conv2d_weight(kw["x"].cpu(), a["gw"], kw["gy"].cpu()).reshape(ref_w.shape)
        d_w = float((w32.double() - ref_w).abs().max())
        d_b = float((kw["gy"][:bn].cpu().sum(dim=(0, 2, 3)).double() - ref_b).abs().max())
        tw, tb = max(3e-6, 2 * d_w / float(ref_w.abs().max())), max(3e-6, 2 * d_b / float(ref_b.abs().max()))
        ew = _report("conv1x1_wgrad w", kw["gw"].reshape(ref_w.shape), ref_w, tw)
        eb = _report("conv1x1_wgrad b", kw["gb"], ref_b, tb)
        print(f"conv1x1_wgrad {a['x']}: error w {ew:.2e} b {eb:.2e}, fp32 term w {2 * d_w / float(ref_w.abs().max()):.2e} "
              f"b {2 * d_b / float(ref_b.abs().max()):.2e}")
    else:
        raise AssertionError(f"no headline-shape check for {name}")


CHECKS = {"conv3x3": _check_conv, "conv3x3_small": _check_conv, "winoups3x3": _check_upconv, "winoups3x3_head": _check_upconv,
          "upconv3x3": _check_upconv, "winoups3x3_dgrad": _check_winoups_dgrad, "winoups3x3_dgrad_pn": _check_winoups_dgrad,
          "stem_pair": _check_ends, "stem_pair_gx": _check_ends, "head_pair_from_mp": _check_ends, "gen_head_bwd": _check_ends,
          "blend_up_bwd": _check_ends, "head_pair": _check_ends, "conv1x1": _check_conv1x1}


def check_launch(line, hook=None):
    """One committed census line: the launch on its own at that shape and those flags, against its float64 restatement."""
    name, args = parse(line)
    a = dict(args)
    g = _gen(line)
    with _hooked(hook):
        if name == "conv3x3_fade":
            _check_conv_fade(a, g)
        elif name == "conv3x3_small_pn":
            _check_small_pn(a, g)
        elif name in CHECKS:
            CHECKS[name](name, a, g)
        else:
            _check_elementwise(name, a, g)
    torch.cuda.synchronize()


def check_sweep(lines, key, hook=None):
    """One replay of a deferred weight-gradient sweep: the layers of `lines`, in that order, into one WgradDefer, one flush (the
    grouped matrix launches and the one-launch slab reduction), gw and gb pre-filled with NaN; every weight and bias gradient in
    full against float64 autograd of F.conv2d (through F.interpolate for the up-sampled inputs).  Bound: the larger of 3e-6 and
    twice plain fp32 PyTorch's own deviation from the float64 reference at the same shape (the reduction runs over N H W: 3.1 M
    terms for 192 images at 128 x 128, where fp32 itself is 5.7e-6 of the largest element off), printed per layer.  Returns the
    fp32 terms [(weights, bias), ...]."""
    ops = _ops()
    g = _gen(key)
    d = ops.WgradDefer()
    layers = []
    for line in lines:
        a = dict(parse(line)[1])
        x, gy = torch.randn(a["x"], device=DEV, generator=g), torch.randn(a["gy"], device=DEV, generator=g)
        gw, gb = torch.full(a["gw"], float("nan"), device=DEV), torch.full(a["gb"], float("nan"), device=DEV)
        ops.conv3x3_wgrad(x, gy, gw, gb, ups=a.get("ups", False), accumulate=False, bias_n=a.get("bias_n", 0), defer=d)
        layers.append((a, x, gy, gw, gb))
    d.flush()
    torch.cuda.synchronize()
    terms = []
    with _hooked(hook):
        for a, x, gy, gw, gb in layers:
            n = a["x"][0]
            bn = a.get("bias_n", 0) or n
            ups = a.get("ups", False)
            src = (lambda t: _up2(t)) if ups else (lambda t: t)
            w64 = torch.zeros(a["gw"], dtype=torch.float64)
            for i0, i1 in _slices(n, gy[0].numel()):
                w64 += torch.nn.grad.conv2d_weight(src(_host(x, i0, i1)), a["gw"], _host(gy, i0, i1), padding=1)
            b64 = _host(gy, 0, bn).sum(dim=(0, 2, 3))
            w32 = torch.nn.grad.conv2d_weight(src(x.cpu()), a["gw"], gy.cpu(), padding=1)
            b32 = gy[:bn].cpu().sum(dim=(0, 2, 3))
            fw = 2 * float((w32.double() - w64).abs().max()) / float(w64.abs().max())
            fb = 2 * float((b32.double() - b64).abs().max()) / float(b64.abs().max())
            print(f"wgrad {a['x']} -> {a['gy']}{' ups' if ups else ''}: fp32 term w {fw:.2e} b {fb:.2e} (bound 3e-6 or that)")
            terms.append((fw, fb))
            _report(f"wgrad w {a['x']} -> {a['gy']}", gw, w64, max(3e-6, fw))
            _report(f"wgrad b {a['x']} -> {a['gy']}", gb, b64, max(3e-6, fb))
    return terms


# ------------------------------------------------------------------ would a check notice?  (tests/test_launch_checks_cpu.py)
def listen(seen):
    """Hook that changes nothing and appends the name of every comparison to `seen`."""
    def hook(what, got, delta):
        seen.append(what)
        return got
    return hook


def perturb(target, last, fired):
    """Hook: the first tensor compared under the name `target` with ONE value changed -- the element in the middle of every
    dimension, or (`last`) the very last one (last image, last row); + delta, or one flipped bit of a tile mask (the bit `delta`
    names for that byte, bit 0 where the comparison is bit for bit)."""
    def hook(what, got, delta):
        if what != target or fired:
            return got
        fired.append(what)
        t = got.detach().clone(memory_format=torch.contiguous_format)
        k = t.numel() - 1 if last else sum((s // 2) * st for s, st in zip(t.shape, t.stride()))
        if delta is None:
            t.view(-1)[k] ^= 1
        elif isinstance(delta, torch.Tensor):
            t.view(-1)[k] ^= delta.reshape(-1)[k].to(t.device)
        else:
            t.view(-1)[k] += delta
        return t
    return hook


def must_notice(run, whats):
    """run(hook) performs a check; with one element of any one of the comparisons `whats` changed it must fail, and fail there."""
    import re
    import pytest
    assert whats
    for what in dict.fromkeys(whats):
        for last in (False, True):
            fired = []
            with pytest.raises(AssertionError, match=re.escape(what)):
                run(perturb(what, last, fired))
            assert fired == [what]

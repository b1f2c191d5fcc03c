"""The launch prologue of the wave-per-tile-block Winograd kernels (csrc/wino_strip.hip, csrc/wino_ups.hip): the filter bank reaches LDS
by LDS-DMA, every piece requested before the first wait (wino_bank_fill, csrc/wino_common.h), with the first block's rows in flight
behind it.  Checked at the ENDS of the bank size rather than at the workload's: the smallest bank (2 chunks, one tile), an odd
out-tile count (the LDS image carries a padding tile), five out-tiles, and the one-tile kernel whose bank is the whole 160 KB; for
wino_ups the chunks that end in half a copy instruction (odd tile counts) and the two-launch tile-group data gradient, whose launches
copy a strided part of the bank.  Strip kernel: bit for bit the staged kernel's results (MG_WINO_STRIP=0) and fp64 `F.conv2d` /
`F.conv_transpose2d` at tests/test_wino_strip_gpu.py's tolerance; wino_ups: fp64 `F.interpolate -> F.conv2d` and autograd at
tests/test_winoups_gpu.py's.  Every case first asks the planner / the *_supported query that the shape takes the kernel in question."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE = 0.2


def _ops():
    from musicgan_amd import ops
    return ops


def _tile_mask(act):
    n, c, h, w = act.shape
    b = (act > 0).reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4).to(torch.uint8)
    return (b[..., 0] + 2 * b[..., 1] + 4 * b[..., 2] + 8 * b[..., 3]).contiguous()


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------------------------ the strip kernel
# (N, Cin, Cout, H, W) of the layer and what the plan of its forward call must say: tiles per wave, workgroup rows, a padding row, chunks
STRIP_SHAPES = {
    "smallest bank": ((64, 16, 16, 64, 64), dict(niw=1, rows=1, pad=False, s_nchunk=2, lds=2 * 8192)),
    "odd tile count": ((64, 48, 48, 64, 64), dict(niw=2, rows=2, pad=True, s_nchunk=6, lds=6 * 2 * 8192)),
    "five tiles": ((64, 64, 80, 64, 64), dict(niw=2, rows=3, pad=True, s_nchunk=8, lds=8 * 2 * 8192)),
    "largest bank": ((128, 160, 160, 32, 32), dict(niw=1, rows=10, pad=False, s_nchunk=20, lds=160 * 1024)),
}
KINDS = ["plain", "lrelu+pool+mask_out", "dgrad mask bytes", "unpool_mask"]


@functools.lru_cache(maxsize=1)  # (one shape's tensors at a time: the cases of a shape run one after the other)
def _strip_case(name):
    """Inputs (host and device) and the fp64 references of one layer, shared by its four kinds and left unchanged."""
    (n, ci, co, h, w), _ = STRIP_SHAPES[name]
    g = torch.Generator().manual_seed(57)
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, 3, 3, generator=g) / math.sqrt(9 * ci)
    b = torch.randn(co, generator=g)
    gy = torch.randn(n, co, h, w, generator=g)
    act_up = torch.randn(n, ci, 2 * h, 2 * w, generator=g)
    c = dict(x=x, wt=wt, b=b, gy=gy, act_up=act_up)
    c["pre"] = F.conv2d(x.double(), wt.double(), None, padding=1)            # without the bias
    c["refd"] = F.conv_transpose2d(gy.double(), wt.double(), padding=1)       # data gradient
    for k in ("x", "wt", "b", "gy"):
        c[k + "_d"] = c[k].to(DEV)
    c["m_x"] = _tile_mask(c["x_d"])
    c["m_up"] = _tile_mask(act_up.to(DEV))
    return c


def _strip_call(ops, c, kind, strip):
    """One call of `kind`; `strip` False: the staged kernel's form of it (the fp32 mask where it has no byte form)."""
    ci, co = c["wt"].shape[1], c["wt"].shape[0]
    if kind == "plain":
        return (ops.conv3x3(c["x_d"], None, None, co, wino=ops.pack_wino3x3(c["wt_d"], dgrad=False)),)
    if kind == "lrelu+pool+mask_out":
        return ops.conv3x3(c["x_d"], None, c["b_d"], co, lrelu=True, pool=True, wino=ops.pack_wino3x3(c["wt_d"], dgrad=False), mask_out=True)
    upd = ops.pack_wino3x3(c["wt_d"], dgrad=True)
    if kind == "dgrad mask bytes":
        return (ops.conv3x3(c["gy_d"], None, None, ci, mask_aux=c["m_x"] if strip else c["x_d"], wino=upd),)
    return (ops.conv3x3(c["gy_d"], None, None, ci, wino=upd, unpool_mask=c["m_up"]),)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(STRIP_SHAPES))
def test_strip_kernel_at_the_ends_of_the_bank_size(name, kind, monkeypatch, tmp_path_factory):
    import wino_plan_shim as shim
    ops = _ops()
    (n, ci, co, h, w), want = STRIP_SHAPES[name]
    for v in ("MG_WINO_STRIP", "MG_WINO_STRIP_NIW", "MG_WINO_STRIP_WGS", "MG_WINO_STRIP_MIN_BLOCKS", "MG_WINO_STRIP_ABLATE"):
        monkeypatch.delenv(v, raising=False)
    # the planner, as the library was built with it: the default route of this call is the strip kernel, in the form the case is about
    lib = shim.load(tmp_path_factory.mktemp("wino_plan"))
    Fl = shim.FLAGS
    layer = {"plain": (n, ci, co, h, w, 0, 0, 1),
             "lrelu+pool+mask_out": (n, ci, co, h, w, Fl["LRELU"] | Fl["POOL_OUT"] | Fl["MASK_OUT"], 1, 1),
             "dgrad mask bytes": (n, co, ci, h, w, Fl["MASK_AUX"] | Fl["MASK_BYTES"], 0, 1),
             "unpool_mask": (n, co, ci, h, w, Fl["UNPOOL"], 0, 1)}[kind]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    p = shim.plan(lib, np.array([layer]), n_cu, 1, shim.switches(lib))
    assert p.strip[0] == 1, f"{name} / {kind}: the planner leaves {layer} to the staged kernel"
    if kind in ("plain", "lrelu+pool+mask_out"):
        got = dict(niw=int(p.niw[0]), rows=int(p.rows[0]), pad=bool(p.g_pad[0] > 0), s_nchunk=int(p.s_nchunk[0]), lds=int(p.lds[0]))
        assert got == want, (name, got)
    if kind == "dgrad mask bytes":
        assert ops.wino3x3_mask_bytes_y_supported(n, co, ci, h, w)

    c = _strip_case(name)
    res_strip = _strip_call(ops, c, kind, True)
    monkeypatch.setenv("MG_WINO_STRIP", "0")
    res_staged = _strip_call(ops, c, kind, False)
    monkeypatch.delenv("MG_WINO_STRIP")
    again = _strip_call(ops, c, kind, True)
    torch.cuda.synchronize()
    for i, (s, q, r) in enumerate(zip(res_staged, res_strip, again)):
        assert torch.equal(s, q), f"{name} / {kind}[{i}]: {int((s != q).sum())} of {s.numel()} elements differ from the staged kernel"
        assert torch.equal(q, r), f"{name} / {kind}[{i}]: two runs differ"

    # fp64, at tests/test_wino_strip_gpu.py's tolerance
    if kind == "plain":
        ref = c["pre"]
        assert float((res_strip[0].double().cpu() - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
    elif kind == "lrelu+pool+mask_out":
        ref = F.leaky_relu(c["pre"] + c["b"].double().view(1, -1, 1, 1), SLOPE)
        scale = float(ref.abs().max())
        m, q = res_strip
        assert float((q.double().cpu() - F.avg_pool2d(ref, 2)).abs().max()) <= 2e-6 * scale
        near = _tile_mask(ref + 1e-5 * scale) != _tile_mask(ref - 1e-5 * scale)  # (within round-off of zero: either bit)
        assert bool(((m.cpu() == _tile_mask(ref)) | near).all())
    elif kind == "dgrad mask bytes":
        ref = c["refd"] * torch.where(c["x"] > 0, 1.0, SLOPE).double()
        assert float((res_strip[0].double().cpu() - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
    else:
        ref = 0.25 * F.interpolate(c["refd"], scale_factor=2, mode="nearest") * torch.where(c["act_up"] > 0, 1.0, SLOPE).double()
        assert float((res_strip[0].double().cpu() - ref).abs().max()) <= 2e-6 * float(ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------------- wino_ups
UPS = (16, 64, 48, 32, 32)  # (N, Cin, Cout, Hin, Win): three out tiles forward (chunks of 13.5 copy instructions), four in the data gradient


def _ups_inputs(seed, n, ci, co, h, w):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, 3, 3, generator=g) / math.sqrt(9 * ci)
    b = torch.randn(co, generator=g)
    gy = torch.randn(n, co, 2 * h, 2 * w, generator=g)
    return x, wt, b, gy


def test_winoups_forward_and_head():
    ops = _ops()
    n, ci, co, h, w = UPS
    assert ops.winoups3x3_supported(n, ci, co, h, w) and ops.winoups3x3_head_supported(n, ci, co, h, w)
    x, wt, b, _ = _ups_inputs(71, *UPS)
    g = torch.Generator().manual_seed(72)
    hw = torch.randn(2, co, 1, 1, generator=g) / math.sqrt(co)
    hb = torch.randn(2, generator=g) * 0.1
    pre = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), wt.double(), b.double(), padding=1)
    act = F.leaky_relu(pre, SLOPE)
    rn_ref = 1.0 / torch.sqrt((act * act).mean(dim=1, keepdim=True) + 1e-8)
    xd, bd, hwd, hbd = x.to(DEV), b.to(DEV), hw.to(DEV), hb.to(DEV)
    up = ops.pack_winoups3x3(wt.to(DEV), False)
    y = ops.winoups3x3(xd, up, bd, co, lrelu=True)
    assert _rel(y, act) <= 2e-6
    assert _rel(ops.winoups3x3(xd, up, None, co), pre - b.double().view(1, -1, 1, 1)) <= 2e-6
    yy, p, rn = ops.winoups3x3(xd, up, bd, co, lrelu=True, pixnorm=True)
    assert torch.equal(yy, y)
    assert _rel(p, act * rn_ref) <= 3e-6 and _rel(rn, rn_ref) <= 3e-6
    # the head form: the same p and rn, mp = tanh(conv1x1(p)) against fp64 on that p
    y1, p1, rn1, mp = ops.winoups3x3_head(xd, up, bd, co, hwd, hbd, want_y=True)
    assert torch.equal(p1, p) and torch.equal(rn1, rn) and torch.equal(y1, y)
    ref = torch.tanh(F.conv2d(p.double().cpu(), hw.double(), hb.double()))
    assert float((mp.double().cpu() - ref).abs().max()) <= 2e-6


def test_winoups_data_gradient_plain_and_with_pixelnorm_backward():
    ops = _ops()
    n, ci, co, h, w = UPS
    assert ops.winoups3x3_supported(n, ci, co, h, w, dgrad=True) and ops.winoups3x3_dgrad_pn_supported(n, ci, co, h, w)
    _, wt, _, gy = _ups_inputs(73, *UPS)
    g = torch.Generator().manual_seed(74)
    x = torch.randn(n, ci, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    (F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt.double(), None, padding=1) * gy.double()).sum().backward()
    upd = ops.pack_winoups3x3(wt.to(DEV), True)
    gx = ops.winoups3x3_dgrad(gy.to(DEV), upd, ci)
    assert _rel(gx, x.grad) <= 3e-6
    assert torch.equal(gx, ops.winoups3x3_dgrad(gy.to(DEV), upd, ci))
    pl = torch.randn(n, ci, h, w, generator=g).to(DEV)
    rnl = (torch.rand(n, 1, h, w, generator=g) + 0.5).to(DEV)
    gpre = ops.winoups3x3_dgrad_pn(gy.to(DEV), upd, pl, rnl, ci)
    assert _rel(gpre, ops.pixelnorm_lrelu_bwd(gx, pl, rnl, from_p=True)) <= 2e-6


def test_winoups_tile_group_data_gradient_twice_with_different_weights():
    """80 <- 64 from 32x32 x 64 images: two launches, tiles 0-2 (chunks that end in half a copy instruction) and tiles 3-4, each copying
    its part of every chunk of the bank.  Run twice in one process with different weights, each result against its own reference: a
    zero-filled or stale piece that lands outside a launch's image -- on the other chunk, or left over from the first run -- makes the
    second result wrong.  The second weight set is the first with its input channels reversed: every tile of the bank changes (tile t
    holds what tile 4 - t held, mirrored), and its reference is the first one's with the channels reversed (the sums over the 64
    out-channels are the same sums) -- one fp64 pass instead of two."""
    ops = _ops()
    n, ci, co, h, w = 64, 80, 64, 32, 32
    assert ops.winoups3x3_supported(n, ci, co, h, w, dgrad=True) and not ops.winoups3x3_dgrad_pn_supported(n, ci, co, h, w)
    _, wt, _, gy = _ups_inputs(75, n, ci, co, h, w)
    # gradient w.r.t. the low-res input = 2x2 block sums of the hi-res data gradient
    ref = 4.0 * F.avg_pool2d(F.conv_transpose2d(gy.double(), wt.double(), padding=1), 2)
    gyd = gy.to(DEV)
    wt2 = wt.flip(1).contiguous()
    up1, up2 = ops.pack_winoups3x3(wt.to(DEV), True), ops.pack_winoups3x3(wt2.to(DEV), True)
    gx1 = ops.winoups3x3_dgrad(gyd, up1, ci)
    gx2 = ops.winoups3x3_dgrad(gyd, up2, ci)
    gx1b = ops.winoups3x3_dgrad(gyd, up1, ci)
    assert _rel(gx1, ref) <= 3e-6
    assert _rel(gx2, ref.flip(1)) <= 3e-6
    assert torch.equal(gx1, gx1b)

"""DiffAugment without a device: the parameter decode the kernels run (csrc/diffaug_plan.h, compiled by g++ into a ctypes shim, and the
library's host entry mg_diffaug_decode) against the definition restated in tests/diffaug_ref.py; the reference's own adjoint
identity; the CLI flags, the argument checks and the resume refusal of `train`, all before anything touches a device."""
import ctypes
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import diffaug_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "musicgan_amd", "csrc")
SIZES = (1, 2, 3, 4, 5, 7, 8, 16, 31, 64, 512)
OPS = (0, 1, 2, 3)
PS = (0.0, 0.5, 1.0)

SHIM = r'''
#include "diffaug_plan.h"
extern "C" void shim_decode(const float* u, int n, int h, int w, int ops, float p, int* out) {
  for (int i = 0; i < n; ++i) {
    const DaParams q = da_decode(u + (long long)i * DA_U, h, w, ops, p);
    int* o = out + (long long)i * 6;
    o[0] = q.dy; o[1] = q.dx; o[2] = q.y0; o[3] = q.y1; o[4] = q.x0; o[5] = q.x1;
  }
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """the header compiled by plain g++: no HIP header in reach"""
    d = tmp_path_factory.mktemp("diffaug_shim")
    src, so = str(d / "diffaug_shim.cpp"), str(d / "diffaug_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, src, "-o", so],
                   check=True)
    return ctypes.CDLL(so)


def shim_decode(lib, u, h, w, ops, p):
    u = np.ascontiguousarray(u, dtype=np.float32)
    out = np.full((u.shape[0], 6), -12345, dtype=np.int32)
    lib.shim_decode(u.ctypes.data_as(ctypes.c_void_p), u.shape[0], h, w, ops, ctypes.c_float(p), out.ctypes.data_as(ctypes.c_void_p))
    return out


def edge_values(size, p):
    """0, the largest float32 below 1, every bin edge k / bins of the two decodes of a side of `size` one ulp below, at and one ulp
    above, and the same around p -- everything inside [0, 1)"""
    r, c = int(np.floor(size / 8 + 0.5)), int(np.floor(size / 2 + 0.5))
    vals = [np.float32(0), np.nextafter(np.float32(1), np.float32(0))]
    edges = [np.float32(p)]
    for bins in (2 * r + 1, size + 1 - c % 2):
        edges += [np.float32(k / bins) for k in range(bins + 1)]
    for e in edges:
        vals += [np.nextafter(e, np.float32(-1)), e, np.nextafter(e, np.float32(2))]
    v = np.unique(np.array(vals, dtype=np.float32))
    return v[(v >= 0) & (v < 1)]


def crafted_u(h, w, p):
    """rows whose columns run through the edge values of their own decode"""
    vh, vw = edge_values(h, p), edge_values(w, p)
    n = max(len(vh), len(vw))
    u = np.zeros((n, 8), dtype=np.float32)
    rng = np.random.default_rng(1000 * h + w)
    for col, v in enumerate((vh, vh, vw, vw, vh, vw, vh, vw)):
        u[:, col] = np.resize(rng.permutation(v), n)   # every value at least once, each column in an order of its own
    # the on/off columns also against every value of the others: a second block with columns 0 and 3 reversed
    u2 = u.copy()
    u2[:, 0], u2[:, 3] = u[::-1, 0], u[::-1, 3]
    return np.concatenate([u, u2])


def test_plan_header_equals_the_definition(shim):
    checked = 0
    for h, w in itertools.product(SIZES, SIZES):
        ry, rx = int(np.floor(h / 8 + 0.5)), int(np.floor(w / 8 + 0.5))
        for p in PS:
            u = crafted_u(h, w, p)
            for ops in OPS:
                got, ref = shim_decode(shim, u, h, w, ops, p), R.decode(u, h, w, ops, p)
                bad = np.nonzero((got != ref).any(axis=1))[0]
                assert bad.size == 0, (h, w, ops, p, u[bad[0]], got[bad[0]], ref[bad[0]])
                dy, dx, y0, y1, x0, x1 = got.T
                assert (np.abs(dy) <= ry).all() and (np.abs(dx) <= rx).all()
                assert (0 <= y0).all() and (y0 <= y1).all() and (y1 <= h).all() and (0 <= x0).all() and (x0 <= x1).all() and (x1 <= w).all()
                if p == 0.0 or ops == 0:
                    assert not got.any(), "p = 0 or no op must decode to the identity"
                if not ops & R.TRANSLATION:
                    assert not dy.any() and not dx.any()
                if not ops & R.CUTOUT:
                    assert not got[:, 2:].any()
                checked += got.shape[0]
    assert checked > 100000


def test_every_shift_and_every_box_is_reached(shim):
    """the decode is onto: at p = 1 the crafted rows produce every dy in [-ry, ry] and every box position, clipped ones included"""
    for size in (4, 8, 31, 512):
        r, c = int(np.floor(size / 8 + 0.5)), int(np.floor(size / 2 + 0.5))
        got = shim_decode(shim, crafted_u(size, size, 1.0), size, size, 3, 1.0)
        assert set(got[:, 0]) == set(range(-r, r + 1)) and set(got[:, 1]) == set(range(-r, r + 1))
        tops = {max(oy - c // 2, 0) for oy in range(size + 1 - c % 2)}
        assert set(got[:, 2]) == tops and set(got[:, 4]) == tops
        assert got[:, 3].max() == size and (got[:, 3] - got[:, 2]).min() < c   # a box clipped at the far edge, and one cut short


def test_out_of_range_u_cannot_leave_the_image(shim):
    """u is promised in [0, 1); a value outside it (an uninitialised buffer) still decodes to a shift and a box inside the image"""
    u = np.array([[0, v, v, 0, v, v, 0, 0] for v in (-1.0, 1.0, 2.0, 1e30, -1e30, np.inf, -np.inf, np.nan)], dtype=np.float32)
    for h, w in ((1, 1), (5, 7), (64, 512)):
        got = shim_decode(shim, u, h, w, 3, 1.0)
        assert (np.abs(got[:, 0]) <= (h + 4) // 8).all() and (np.abs(got[:, 1]) <= (w + 4) // 8).all()
        assert (got[:, 2] >= 0).all() and (got[:, 3] <= h).all() and (got[:, 4] >= 0).all() and (got[:, 5] <= w).all()


def test_library_host_decode_equals_the_definition():
    from musicgan_amd import aug_ops
    for (h, w), ops, p in itertools.product(((4, 4), (8, 8), (5, 7), (31, 33), (512, 512)), OPS, PS):
        u = crafted_u(h, w, p)
        assert np.array_equal(aug_ops.diffaug_decode(u, h, w, ops, p), R.decode(u, h, w, ops, p)), (h, w, ops, p)
        assert np.array_equal(aug_ops.diffaug_decode(torch.from_numpy(u), h, w, ops, p), R.decode(u, h, w, ops, p))
    with pytest.raises(ValueError):
        aug_ops.diffaug_decode(np.zeros((2, 7), np.float32), 4, 4, 3, 1.0)
    with pytest.raises(ValueError):
        aug_ops.diffaug_decode(np.zeros((2, 8), np.float32), 4, 4, 3, 1.5)


def test_reference_adjoint_identity_is_exact():
    """<T x, g> == <x, T^t g> on integer-valued data (every product and sum exact in float64)"""
    rng = np.random.default_rng(5)
    for (n, c, h, w), ops, p in itertools.product(((40, 2, 4, 4), (30, 1, 5, 7), (12, 3, 8, 8), (6, 2, 31, 33)), OPS, PS):
        x = rng.integers(-8, 9, (n, c, h, w)).astype(np.float32)
        g = rng.integers(-8, 9, (n, c, h, w)).astype(np.float32)
        u = rng.random((n, 8), dtype=np.float32)
        lhs = float((R.fwd(x, u, ops, p).astype(np.float64) * g).sum())
        rhs = float((x.astype(np.float64) * R.bwd(g, u, ops, p)).sum())
        assert lhs == rhs, (n, c, h, w, ops, p)
        if p == 0.0 or ops == 0:
            assert np.array_equal(R.fwd(x, u, ops, p), x) and np.array_equal(R.bwd(g, u, ops, p), g)
        # the differentiable restatement is the same map, and autograd's gradient of it is bwd
        xt = torch.from_numpy(x).double().requires_grad_(True)
        y = R.fwd_torch(xt, u, ops, p)
        assert np.array_equal(y.detach().numpy(), R.fwd(x, u, ops, p).astype(np.float64))
        (gx,) = torch.autograd.grad(y, xt, torch.from_numpy(g).double())
        assert np.array_equal(gx.numpy(), R.bwd(g, u, ops, p).astype(np.float64))


def test_reference_drops_nan_under_the_mask_and_writes_positive_zero():
    x = np.full((1, 1, 8, 8), np.nan, dtype=np.float32)
    u = np.array([[0, 0.99, 0.99, 0, 0.5, 0.5, 0, 0]], dtype=np.float32)   # dy = dx = +1, box rows / columns [2, 6)
    (dy, dx, y0, y1, x0, x1), = R.decode(u, 8, 8, 3, 1.0)
    assert (dy, dx, y0, y1, x0, x1) == (1, 1, 2, 6, 2, 6)
    y = R.fwd(x, u, 3, 1.0)
    dropped = np.zeros((8, 8), bool)
    dropped[0, :] = dropped[:, 0] = dropped[2:6, 2:6] = True
    assert np.isnan(y[0, 0][~dropped]).all()
    assert (y[0, 0][dropped].view(np.int32) == 0).all()   # +0.0, not -0.0, not NaN


# ------------------------------------------------------------------------------------------------ CLI, arguments, resume

def _train():
    """`train` through the package's lazy re-export: importing the sub-module first would leave `musicgan_amd.train` bound to the module
    for the rest of the process, which other tests read as the function"""
    import musicgan_amd
    t = musicgan_amd.train
    return t if callable(t) else t.train


def test_cli_flags_reach_train_as_keywords(monkeypatch):
    from musicgan_amd import __main__ as cli
    calls = []
    _train()
    train_mod = importlib.import_module("musicgan_amd.train")
    monkeypatch.setattr(train_mod, "train", lambda *a, **k: calls.append((a, k)))
    base = ["train", "R", "-i", "D", "-o", "O"]
    cli.main(base)
    cli.main(base + ["--augment", "translation,cutout"])
    cli.main(base + ["--augment", "cutout", "--augment-p", "0.8"])
    cli.main(base + ["--resident", "--augment", "translation"])
    assert calls == [(("R", "D", "O"), {}), (("R", "D", "O"), {"augment": "translation,cutout"}),
                     (("R", "D", "O"), {"augment": "cutout", "augment_p": 0.8}),
                     (("R", "D", "O"), {"resident": True, "augment": "translation"})]
    for bad in (["--augment", "rotation"], ["--augment", "cutout,cutout"], ["--augment", "translation,"], ["--augment", ""],
                ["--augment", "cutout", "--augment-p", "1.5"], ["--augment", "cutout", "--augment-p", "-0.1"],
                ["--augment", "cutout", "--augment-p", "nan"], ["--augment", "cutout", "--augment-p", "often"]):
        with pytest.raises(SystemExit):
            cli.main(base + bad)
    assert len(calls) == 4


def test_train_signature_defaults_off():
    import inspect
    train = _train()
    p = inspect.signature(train).parameters
    assert p["augment"].default == "" and p["augment_p"].default == 1.0
    assert p["augment"].kind == p["augment_p"].kind == inspect.Parameter.KEYWORD_ONLY


def _no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(torch.cuda, "set_device", touched)


def test_train_refuses_bad_flags_before_it_touches_the_device(tmp_path, monkeypatch):
    train = _train()
    _no_device(monkeypatch)
    data = tmp_path / "data"
    data.mkdir()
    for kw in (dict(augment="rotation"), dict(augment="cutout,cutout"), dict(augment="cutout", augment_p=1.5),
               dict(augment="cutout", augment_p=-0.5), dict(augment="cutout", augment_p=float("nan")), dict(augment_p=0.5)):
        with pytest.raises(ValueError):
            train("t", str(data), str(tmp_path / "out"), **kw)
    assert not (tmp_path / "out").exists()


def test_resume_with_other_augmentation_flags_is_refused(tmp_path, monkeypatch):
    train = _train()
    _no_device(monkeypatch)
    data = tmp_path / "data"
    data.mkdir()
    cases = (({"augment": "translation", "augment_p": 1.0}, dict(augment="translation,cutout")),
             ({"augment": "translation,cutout", "augment_p": 1.0}, dict(augment="translation,cutout", augment_p=0.5)),
             ({"augment": "translation,cutout", "augment_p": 1.0}, dict()),
             ({}, dict(augment="cutout")))
    for i, (saved, flags) in enumerate(cases):
        run = tmp_path / f"run{i}"
        run.mkdir()
        torch.save({"iter_idx": 3, **saved}, str(run / "train_state_0.pt"))
        with pytest.raises(ValueError, match="would not continue it"):
            train("t", str(data), str(tmp_path / "out"), resume_from=str(run), **flags)
    assert not (tmp_path / "out").exists()


def test_diffaugment_validates_without_a_device_and_refuses_cpu_tensors():
    from musicgan_amd import aug_ops
    from musicgan_amd._lib import MusicGanHipError
    from musicgan_amd.networks import DiffAugment
    a = DiffAugment()
    assert a.spec == (3, 1.0) and hash(a.spec) == hash((3, 1.0)) and a.policy == "translation,cutout"
    assert DiffAugment("cutout", 0.25).spec == (2, 0.25) and DiffAugment(" cutout , translation ").spec == (3, 1.0)
    for bad in (dict(policy=""), dict(policy="colour"), dict(policy="cutout,cutout"), dict(policy=3), dict(p=1.01), dict(p=-1e-9),
                dict(p=float("nan")), dict(p="often")):
        with pytest.raises(ValueError):
            DiffAugment(**bad)
    u = a.draw(5, "cpu", generator=torch.Generator().manual_seed(1))
    assert tuple(u.shape) == (5, 8) and u.dtype == torch.float32 and bool(((u >= 0) & (u < 1)).all())
    x = torch.zeros(5, 2, 4, 4, requires_grad=True)
    with pytest.raises(MusicGanHipError, match="no CPU fallback"):
        a(x, u)
    for fn in (aug_ops.diffaug_fwd, aug_ops.diffaug_bwd):
        with pytest.raises(MusicGanHipError, match="no CPU fallback"):
            fn(x.detach(), u, 3, 1.0)
        with pytest.raises(MusicGanHipError):
            fn(x.detach().numpy(), u, 3, 1.0)


def test_stepper_refuses_u_without_augmentation():
    from musicgan_amd.train_step import ProGANStepper
    st = ProGANStepper(None, None, None, None, 8)
    assert st.augment is None
    with pytest.raises(ValueError, match="without augmentation"):
        st.d_step(torch.zeros(2, 2, 4, 4), 1.0, u=torch.zeros(4, 8))
    with pytest.raises(ValueError, match="without augmentation"):
        st.g_step(2, 1.0, "cpu", u=torch.zeros(2, 8))


def test_kernels_use_no_scratch_memory_and_no_lds():
    from musicgan_amd import _build
    _build.build()
    usage = {k: v for k, v in _build.resource_usage().items() if "diffaug_k" in k}
    assert len(usage) == 4, sorted(usage)   # forward / backward x vector / scalar
    for name, u in usage.items():
        assert u.get("ScratchSize [bytes/lane]", 0) == 0 and u.get("LDS Size [bytes/block]", 0) == 0 and u.get("VGPRs", 0) > 0, (name, u)

"""CPU: the definition of the multi-scale L2 loss (tests/pyrloss_ref.py against autograd), its launch planner
(musicgan_amd/csrc/pyrloss_plan.h through a g++ shim), project.slerp, the `project` sub-command and the new flags of `generate`, and
the refusals of generate(latents=...) that come before any device is touched."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyrloss_ref as R  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "musicgan_amd", "csrc")
FIELDS = "ok tile_h tile_w tiles_y tiles_x tiles_per_sample grid elems lds_bytes ws_bytes".split()
SHIM = r'''
#include "pyrloss_plan.h"
static_assert(sizeof(((PyrPlan*)0)->elems) == 8 && sizeof(((PyrPlan*)0)->grid) == 8 && sizeof(((PyrPlan*)0)->tiles_per_sample) == 8 &&
              sizeof(((PyrPlan*)0)->ws_bytes) == 8, "element, tile and byte counts are held in 64 bits");
extern "C" void shim_plan(int n, int c, int h, int w, int l, long long* out) {
  const PyrPlan p = pyr_plan(n, c, h, w, l);
  const long long row[] = {p.ok, p.tile_h, p.tile_w, p.tiles_y, p.tiles_x, p.tiles_per_sample, p.grid, p.elems,
                           (long long)p.lds_bytes, (long long)p.ws_bytes};
  for (int k = 0; k < 10; ++k) out[k] = row[k];
}
extern "C" int shim_extent(int size, int t) { return pl_tile_extent(size, t); }
extern "C" int shim_const(int i) {
  const int v[] = {PL_MAX_LEVELS, PL_TILE, PL_THREADS, PL_RED, (int)PL_LDS_LIMIT};
  return v[i];
}
extern "C" int shim_level(int s, int what) { return what ? pl_level_stride(s) : pl_level_off(s); }
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("pyrloss_plan")
    src, so = os.path.join(str(d), "shim.cpp"), os.path.join(str(d), "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, src, "-o", so], check=True)
    return ctypes.CDLL(so)


def _plan(shim, n, c, h, w, l):
    out = (ctypes.c_longlong * len(FIELDS))()
    shim.shim_plan(n, c, h, w, l, out)
    return dict(zip(FIELDS, list(out)))


# ------------------------------------------------------------------ the definition
@pytest.mark.parametrize("shape", [(2, 2, 8, 8, 4), (1, 2, 96, 32, 6), (3, 1, 64, 64, 7)], ids=str)
def test_reference_gradient_is_the_derivative_of_the_definition(shape):
    """g64 of the reference against torch.autograd through avg_pool2d in float64, to 1e-12 relative.  The inputs are multiples of
    1/8 in [-1, 1]: d_0 has 5 significant bits and every level adds 2, so the float32 pyramid is exact and both sides see the same d_s."""
    *dims, levels = shape
    rng = np.random.default_rng(1)
    x, t = (rng.integers(-8, 9, size=dims).astype(np.float32) / 8 for _ in range(2))
    lam = tuple(float(v) for v in rng.integers(0, 5, size=levels) / 4.0)
    d = R.pyramid(x, t, levels)
    g64, _ = R.grad64(d, lam)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    cur, total = xt - torch.from_numpy(t.astype(np.float64)), 0.0
    for s in range(levels):
        if s:
            cur = torch.nn.functional.avg_pool2d(cur, 2)
        assert np.array_equal(cur.detach().numpy(), d[s].astype(np.float64))
        total = total + lam[s] * (cur * cur).mean(dim=(1, 2, 3))
    np.testing.assert_allclose(total.detach().numpy(), R.loss(d, lam), rtol=1e-12)
    total.sum().backward()
    scale = np.abs(g64).max()
    assert scale > 0 and np.abs(xt.grad.numpy() - g64).max() <= 1e-12 * scale


# ------------------------------------------------------------------ the planner
def test_plan_constants_are_the_reference_s(shim):
    assert [shim.shim_const(i) for i in range(5)] == [R.MAX_LEVELS, R.TILE, R.THREADS, R.RED, R.LDS_LIMIT]
    off = 0
    for s in range(1, R.MAX_LEVELS):   # the levels kept in LDS lie one behind the other
        assert shim.shim_level(s, 0) == off and shim.shim_level(s, 1) == R.TILE >> s
        off += (R.TILE >> s) ** 2


@pytest.mark.parametrize("shape", R.SHAPES + [(6, 2, 512, 512, 7), (1, 2, 512, 5120, 7), (4096, 2, 512, 5120, 1)], ids=str)
def test_plan_covers_every_plane_once(shim, shape):
    from musicgan_amd import _build, _lib
    _build.build()
    n, c, h, w, levels = shape
    p, g = _plan(shim, *shape), 1 << (levels - 1)
    assert p["ok"] == 1
    want = R.plan(*shape)
    assert {k: p[k] for k in want} == want
    assert p["tile_h"] % g == 0 and p["tile_w"] % g == 0
    for size, tiles in ((h, p["tiles_y"]), (w, p["tiles_x"])):
        ext = [shim.shim_extent(size, t) for t in range(tiles)]
        assert all(0 < e <= R.TILE and e % g == 0 for e in ext) and sum(ext) == size   # consecutive, so: each pixel in one tile
    assert p["lds_bytes"] <= R.LDS_LIMIT
    assert p["elems"] == n * c * h * w and p["grid"] == n * c * p["tiles_y"] * p["tiles_x"] < 1 << 31
    assert p["ws_bytes"] == p["grid"] * levels * 8 == _lib.load().mg_pyramid_l2_ws_bytes(*shape)


@pytest.mark.parametrize("shape", [(1, 1, 2, 6, 3), (1, 1, 6, 2, 3), (1, 2, 96, 32, 7), (1, 1, 64, 64, 0), (1, 1, 64, 64, 8),
                                   (0, 1, 8, 8, 1), (1 << 21, 2, 512, 5120, 1)], ids=str)
def test_plan_refuses(shim, shape):
    from musicgan_amd import _build, _lib
    _build.build()
    assert _plan(shim, *shape) == dict.fromkeys(FIELDS, 0) and R.plan(*shape) is None
    assert _lib.load().mg_pyramid_l2_ws_bytes(*shape) == 0


def test_weights_are_checked_on_the_host():
    from musicgan_amd import proj_ops
    assert proj_ops.default_levels(512, 512) == 7 and proj_ops.default_levels(96, 32) == 6 and proj_ops.default_levels(2, 6) == 2
    assert proj_ops.default_levels(1, 1) == 1 and proj_ops.default_levels(16, 16) == 5
    assert proj_ops.check_weights(16, 16) == (0.2,) * 5 and proj_ops.check_weights(16, 16, levels=2) == (0.5, 0.5)
    assert proj_ops.check_weights(8, 8, (1, 0, 0.5)) == (1.0, 0.0, 0.5)
    for bad in (dict(weights=()), dict(weights=(1.0,) * 8), dict(weights=(1.0, -0.5)), dict(weights=(float("nan"),)),
                dict(weights=(float("inf"),)), dict(levels=0), dict(levels=8), dict(levels=5), dict(weights=(1, 1), levels=3),
                dict(weights="ab")):
        with pytest.raises(ValueError):
            proj_ops.check_weights(8, 8, **bad)


def test_pyramid_l2_refuses_cpu_tensors_loudly():
    from musicgan_amd import _lib, networks, proj_ops
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(_lib.MusicGanHipError):
        proj_ops.pyramid_l2(x, x)
    with pytest.raises(_lib.MusicGanHipError):
        networks.PyramidL2()(x, x)
    with pytest.raises(ValueError):
        networks.PyramidL2(weights=(1.0, -1.0))
    with pytest.raises(ValueError):
        networks.PyramidL2(levels=9)


# ------------------------------------------------------------------ slerp and the schedule
def test_slerp():
    from musicgan_amd.project import slerp
    rng = torch.Generator().manual_seed(2)
    a, b = torch.randn(8, 2, 2, generator=rng), torch.randn(8, 2, 2, generator=rng)
    assert torch.equal(slerp(a, b, 0.0), a) and torch.equal(slerp(a, b, 1.0), b)      # the end points, exactly
    b = b * (a.norm() / b.norm())
    for t in (0.1, 0.25, 0.5, 0.9):
        m = slerp(a, b, t)
        assert m.dtype == torch.float32 and m.shape == a.shape
        assert abs(float(m.double().norm() / a.double().norm()) - 1.0) <= 1e-6       # equal norms: the norm is kept
    # halfway on the arc between two orthogonal unit vectors
    e0, e1 = torch.tensor([1.0, 0.0]), torch.tensor([0.0, 1.0])
    assert torch.allclose(slerp(e0, e1, 0.5), torch.full((2,), 0.5 ** 0.5), atol=1e-7)
    # equal inputs: the angle is below 1e-6, the straight line takes over
    for t in (0.0, 0.3, 1.0):
        assert torch.allclose(slerp(a, a.clone(), t), a, rtol=1e-6, atol=0)
    assert torch.equal(slerp(torch.zeros(4), torch.ones(4), 0.5), torch.full((4,), 0.5))   # a zero vector has no direction: line
    # antipodal inputs raise: every great circle through them is a shortest arc
    with pytest.raises(ValueError):
        slerp(a, -a, 0.5)
    with pytest.raises(ValueError):
        slerp(a, b[:4], 0.5)


def test_lr_schedule_is_the_stylegan2_projector_s():
    from musicgan_amd.project import lr_at
    steps, lr = 1000, 0.1
    assert lr_at(0, steps, lr) == 0.0
    assert lr_at(25, steps, lr) == pytest.approx(0.05) and lr_at(50, steps, lr) == pytest.approx(0.1)     # linear ramp over 5 %
    assert all(lr_at(k, steps, lr) == pytest.approx(0.1) for k in (50, 400, 750))
    assert lr_at(875, steps, lr) == pytest.approx(0.05) and 0 < lr_at(999, steps, lr) < 1e-4              # cosine over the last 25 %
    assert all(lr_at(k + 1, steps, lr) < lr_at(k, steps, lr) for k in range(750, 999))


# ------------------------------------------------------------------ the command line
def test_project_parses():
    from musicgan_amd.__main__ import _LATENT_MODES, _MODES, build_parser
    assert list(_MODES) == ["create_dataset", "train", "generate", "view_audio", "evaluate"]
    assert list(_LATENT_MODES) == ["project"]
    module, function, _, call_args, call_kwargs = _LATENT_MODES["project"]
    assert (module, function) == ("project", "project")
    a = build_parser().parse_args(["project", "gen.pt", "32", "clip.wav", "-o", "out"])
    assert call_args(a) == ("gen.pt", 32, "clip.wav", "out")
    assert call_kwargs(a) == dict(level=7, steps=1000, lr=0.1, candidates=16, batch_size=6, seed=0)
    a = build_parser().parse_args("project gen.pt 8 clip.flac -o out --level 2 --steps 10 --lr 0.05 --candidates 4 --batch-size 3 "
                                  "--seed 9 --format flac --griffin-lim 4 --resample".split())
    assert call_args(a) == ("gen.pt", 8, "clip.flac", "out")
    assert call_kwargs(a) == dict(level=2, steps=10, lr=0.05, candidates=4, batch_size=3, seed=9, audio_format="flac", griffin_lim=4,
                                  resample=True)
    import inspect
    from musicgan_amd.project import project
    sig = inspect.signature(project)
    assert list(sig.parameters)[:4] == ["gen_dict_state", "rand_channels", "audio_path", "output_dir"]
    assert set(call_kwargs(a)) <= {k for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY}
    assert {k: sig.parameters[k].default for k in ("level", "steps", "lr", "candidates", "batch_size", "seed")} == \
        dict(level=7, steps=1000, lr=0.1, candidates=16, batch_size=6, seed=0)


def test_generate_parses_the_latent_flags():
    from musicgan_amd.__main__ import _MODES, build_parser
    _, _, _, call_args, call_kwargs = _MODES["generate"]
    a = build_parser().parse_args(["generate", "gen.pt", "32", "-o", "out"])
    assert call_kwargs(a) == {} and call_args(a) == ("out", 32, "gen.pt", 10, 5)
    a = build_parser().parse_args("generate gen.pt 32 -o out --latents a.pt --morph-to b.pt --seed 3".split())
    assert call_kwargs(a) == {"latents": "a.pt", "morph_to": "b.pt", "seed": 3}
    a = build_parser().parse_args("generate gen.pt 32 -o out --seed 0".split())
    assert call_kwargs(a) == {"seed": 0}


# ------------------------------------------------------------------ generate(latents=...) refuses before the device
def _latents_file(path, n, rc, level=7):
    torch.save({"latents": torch.randn(n, rc, 2, 2), "loss": torch.zeros(n, dtype=torch.float64),
                "loss_start": torch.zeros(n, dtype=torch.float64), "rand_channels": rc, "level": level, "steps": 1, "seed": 0,
                "source": "x.wav"}, path)
    return str(path)


def test_generate_refuses_bad_latents_before_touching_the_device(tmp_path):
    """every one of these is a ValueError from the host-side checks: on a machine without a GPU, reaching the device raises another
    error, and nothing is written"""
    from musicgan_amd.generate import generate
    a, b3 = _latents_file(tmp_path / "a.pt", 2, 8), _latents_file(tmp_path / "b3.pt", 3, 8)
    low = _latents_file(tmp_path / "low.pt", 2, 8, level=5)
    out = str(tmp_path / "out")
    torch.save({"weights": 1}, tmp_path / "other.pt")
    for kw in (dict(rand_channels=16, latents=a),                      # the file says rand_channels = 8
               dict(rand_channels=8, latents=low),                     # projected at level 5
               dict(rand_channels=8, morph_to=a),                      # morph_to alone
               dict(rand_channels=8, latents=a, morph_to=b3),          # 2 windows against 3
               dict(rand_channels=8, latents=a, morph_to=a, nb_music=1),
               dict(rand_channels=8, latents=str(tmp_path / "other.pt"))):
        with pytest.raises(ValueError):
            generate(out, kw.pop("rand_channels"), "no_such_checkpoint.pt", 1, kw.pop("nb_music", 2), **kw)
    assert not os.path.exists(out)


def test_wide_latent_and_load():
    from musicgan_amd import project
    z = torch.arange(3 * 2 * 2 * 2, dtype=torch.float32).reshape(3, 2, 2, 2)
    wide = project.wide_latent(z)
    assert wide.shape == (1, 2, 2, 6) and wide.is_contiguous()
    for i in range(3):
        assert torch.equal(wide[0, :, :, 2 * i:2 * i + 2], z[i])
    assert project.window_seed(3, 1) != project.window_seed(3, 2) != project.window_seed(4, 1)

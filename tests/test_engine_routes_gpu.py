"""The launch sequence of `networks/engine.py` on the paths the committed default-switch lists do not reach, and the rule that a
later pass of a step follows the routes its forward pass took.

`census_engine_switches.txt` next to this file holds, per setting of SETTINGS, every launch of one critic + one generator update at
level 3, batch 8, alpha 0.5 in CALL ORDER (not the distinct ones): one `routing_census.spec` line per launch, filtered as
`launch_checks._launch` does -- and the `conv3x3_wgrad` calls kept as well, since the weight-gradient helpers of the engine are what
a change there is most likely to disturb.  Level 3 is the smallest committed configuration with the old head and the old stem live
and a critic deep enough for the SmallNet tail.  The file was recorded from the commit its first line names, before the engine's
passes were given named records; `test_launch_sequence` replays each setting and compares line by line.  Run as a script
(`python tests/test_engine_routes_gpu.py <commit> [path]`) this module writes the file; under pytest it only reads it.

`test_backward_follows_the_forward_tail` and `test_tangent_pass_follows_the_forward_stem` flip a switch BETWEEN two passes of one
step: the later pass reads the route from the context the forward pass made (DiscCtx.tail, DiscCtx.fused_stem) and does not ask
the environment again, so the saved tensors are read in the layout they were written in."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from launch_checks import DEV, _launch, step_census  # noqa: E402
from routing_census import census, spec  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "census_engine_switches.txt")
LEVEL, BATCH = 3, 8
# (name, switches, fused steps?)
SETTINGS = [("defaults", {}, True), ("MG_PN_STAGED=0", {"MG_PN_STAGED": "0"}, True), ("MG_SMALLNET=1", {"MG_SMALLNET": "1"}, True),
            ("MG_FUSE_ENDS=0", {"MG_FUSE_ENDS": "0"}, True), ("MG_TILEMASK=0", {"MG_TILEMASK": "0"}, True),
            ("MG_WINOUPS=0", {"MG_WINOUPS": "0"}, True), ("MG_HEAD_FUSE=0", {"MG_HEAD_FUSE": "0"}, True),
            ("module path", {}, False)]


def _recorded(name: str) -> bool:
    return _launch(name) or name == "conv3x3_wgrad"


def _lines(monkeypatch, switches, fused):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    c = step_census(monkeypatch, LEVEL, BATCH, fused_d_step=fused)
    return [spec(r) for r in c.calls if _recorded(r[0])]


def _committed():
    out, cur = {}, None
    with open(FIXTURE) as f:
        for row in f.read().splitlines()[1:]:
            if row.startswith("["):
                cur = out[row[1:-1]] = []
            elif row.strip():
                cur.append(row)
    return out


@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_launch_sequence(setting, monkeypatch):
    name, switches, fused = setting
    want, got = _committed()[name], _lines(monkeypatch, switches, fused)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: launch {i} of {len(want)} differs\n  now:       {a}\n  committed: {b}"
    assert len(got) == len(want), f"{name}: {len(got)} launches, committed {len(want)}"


# ------------------------------------------------------------------ routes follow the forward pass
def _critic(n):
    import bench
    _, disc = bench.build_nets(LEVEL, 32, DEV)
    rng = torch.Generator(device=DEV).manual_seed(1234)
    side = bench.LEVEL_SIDE[LEVEL]
    xs = [torch.rand(n, 2, side, side, device=DEV, generator=rng) * 2 - 1 for _ in range(2)]
    return disc, xs, torch.rand(n, 1, 1, 1, device=DEV, generator=rng)


def _forward_then_backward(monkeypatch, flip):
    """disc_forward under MG_SMALLNET=1, then (`flip`: under MG_SMALLNET=0) disc_backward on its context -> (census of the backward
    pass, [gx, every kept masked gradient, every parameter gradient])."""
    from musicgan_amd.networks import engine
    monkeypatch.setenv("MG_SMALLNET", "1")
    disc, (x, _), _ = _critic(2)
    W, cache = disc._weights(), disc._pack_cache
    with torch.no_grad():
        out, ctx = engine.disc_forward(W, x, 0.5, cache, save=True)
        if flip:
            monkeypatch.setenv("MG_SMALLNET", "0")
        sink = engine.GradSink()
        with census() as c:
            gx, hs = engine.disc_backward(W, ctx, torch.ones_like(out), cache, sink, need_gx=True, keep_h=True)
        torch.cuda.synchronize()
    kept = [gx, hs.stem, hs.old] + [t for pair in hs.blocks for t in pair] + [sink.get(p) for p in W.tensors()]
    assert all(t is not None for t in kept)
    return c, [t.clone() for t in kept]


def test_backward_follows_the_forward_tail(monkeypatch):
    """The forward pass took the SmallNet tail (its records hold what the chain stored); with MG_SMALLNET switched off before the
    backward pass that pass still runs the tail's chain, and gives the bits of a step during which the switch never moved."""
    c_same, same = _forward_then_backward(monkeypatch, flip=False)
    c_flip, flipped = _forward_then_backward(monkeypatch, flip=True)
    assert "SmallNet.run" in c_same.ops() and "SmallNet.run" in c_flip.ops()
    assert [spec(r) for r in c_flip.calls if _recorded(r[0])] == [spec(r) for r in c_same.calls if _recorded(r[0])]
    assert len(same) == len(flipped)
    for k, (a, b) in enumerate(zip(flipped, same)):
        assert torch.equal(a, b), f"tensor {k} of the backward pass differs after the switch moved"


def test_tangent_pass_follows_the_forward_stem(monkeypatch):
    """MG_FUSE_ENDS goes from 1 to 0 in the middle of disc_step_fused (behind the launch that precedes the tangent pass): the
    forward pass ran the paired stem, so the tangent pass still issues stem_pair(masked=True)."""
    from musicgan_amd.networks import engine
    monkeypatch.setenv("MG_FUSE_ENDS", "1")
    disc, (x_real, x_fake), eps = _critic(2)

    def post(name, rec, out):
        if name == "sumsq_per_sample":
            monkeypatch.setenv("MG_FUSE_ENDS", "0")
        return out

    with torch.no_grad(), census() as c:
        c.post = post
        engine.disc_step_fused(disc._weights(), x_real, x_fake, eps, 0.5, disc._pack_cache, engine.GradSink())
        torch.cuda.synchronize()
    names = [r[0] for r in c.calls]
    fwd = [r for r in c.calls[:names.index("sumsq_per_sample")] if r[0] == "stem_pair"]
    after = [r for r in c.calls[names.index("sumsq_per_sample"):] if r[0] == "stem_pair"]
    assert len(fwd) == 1 and not dict(fwd[0][1]).get("masked", False)
    assert len(after) == 1 and dict(after[0][1]).get("masked") is True


if __name__ == "__main__":
    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    rows = [f"# one critic + one generator update at level {LEVEL}, batch {BATCH}, alpha 0.5, recorded from commit {commit}"]
    for name, switches, fused in SETTINGS:
        with pytest.MonkeyPatch.context() as mp:
            rows += [f"[{name}]"] + _lines(mp, switches, fused) + [""]
    with open(path, "w") as f:
        f.write("\n".join(rows))
    print(f"wrote {len(rows)} rows to {path}")

"""The per-launch net of test_headline_shapes_gpu.py (level 5, batch 64) under the other configurations the benchmark reports:
level 3 batch 8 and level 4 batch 32 (BASELINE.json's configs[0..1]), level 6 batch 6 and level 7 batch 6 (the batch the reference
trains with).  None of their launches is at a headline shape.  What the committed lists show of the batch- and size-dependent
routing there: ops the headline step never launches -- `head_pair`, `axpby` and `blend_lrelu_bwd` (level 3, `head_pair` also at
level 4: the fade-in ends where the head or the blend is not fused into the conv next to it), `stem_pair` without a tile mask
(level 3), plain `winoups3x3` (levels 6 and 7) -- and, at their own sizes, `winoups3x3_dgrad`, the direct `conv3x3` with `ups`, the
small-map kernel with its un-pooling and block-sum epilogues, weight-gradient sweeps of 10 + 8 up to 18 + 16 layers, and the
16- and 32-channel layers at 256 x 256 and 512 x 512.  No list holds an `upconv3x3_dgrad` launch; the one `upconv3x3` (level 4) has
64 output channels.

Levels 0, 1 and 2 (2x4x4, 8x8, 16x16: the first three stages of a training run) follow, at batch 6 (the batch the reference and
train.py train with: 18 images through the critic) and batch 64 (192 images, the benchmark's batch), appended so that the ids and
the de-duplication order of the configurations above stay as they were.  What their lists add: level 0 has no fade-in, so both
ends are lone `conv1x1` launches -- the generator's head with `tanh` (into the step's `out` buffer, or a fresh tensor), the critic's
stem with `lrelu`, its tangent form written over the activation it takes its mask from, and its data gradient (`transposed`) --
which no other level launches and `launch_checks._check_conv1x1` restates; there is no `stem_pair`, `head_pair`, blend or
`conv3x3_fade` there, and the only generator head gradient is a `gen_head_bwd` without `g_in`.  Levels 1 and 2 take the fade-in
ends at 8x8 and 16x16 (`head_pair`, `stem_pair` without a tile mask and in its tangent form, `stem_pair_gx`, `blend_up_bwd`,
`axpby` / `blend_lrelu_bwd` where the blend is not fused), the small-map kernel on nearly every 3x3 layer above 1x1 at batch 6
(all but the critic's 18 images at 16x16) and the Winograd kernels on the 8x8 and 16x16 maps at batch 64, with tile masks (level 2
is the lowest level that launches `conv3x3_fade`, in all three modes, at 8x8), and weight-gradient sweeps of 4 + 2 up to 8 + 6
layers on maps of 1x1 to 16x16.  The multi-layer `SmallNet` chains are opt-in (MG_SMALLNET=1) and appear in no list.

`census_level<L>_batch<B>.txt` next to this file is the routing census (tests/routing_census.py) of one critic + one generator
update of that configuration, committed: under `[launches]` its distinct launches, under `[critic sweep]` / `[generator sweep]`
the deferred weight gradients of each flush in call order, one `routing_census.spec` line per row.
`test_step_launches_are_all_covered` runs the step and fails on a launch that is not listed; `test_launch_against_float64` runs
every listed launch on its own, at exactly that shape and those flags, against the float64 host restatement of
tests/launch_checks.py over every image, with the bound of that kernel's per-op test -- a line the headline list or an earlier
configuration's list already holds is checked there, once; `test_weight_gradient_sweep` replays each sweep into one WgradDefer
and compares every tensor in full (bound: the larger of 3e-6 and twice plain fp32 PyTorch's own deviation from float64, printed).

`test_check_notices_one_wrong_element`: every comparison of every kind of launch is run once more with ONE value of the kernel's
output changed by four times what its bound allows (one bit of a tile mask), first an interior element, then the very last one
(last image, last row), and must fail with the AssertionError of that comparison."""
import os

import pytest

from launch_checks import _launch, check_launch, check_sweep, listen, must_notice, step_census, sweeps_of
from routing_census import parse, spec
from test_headline_shapes_gpu import LAUNCHES as HEADLINE

pytestmark = pytest.mark.gpu

CONFIGS = [(3, 8), (4, 32), (6, 6), (7, 6), (0, 6), (1, 6), (2, 6), (0, 64), (1, 64), (2, 64)]
SECTIONS = ("launches", "critic sweep", "generator sweep")


def _committed(level, batch):
    out, cur = {s: [] for s in SECTIONS}, None
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), f"census_level{level}_batch{batch}.txt")) as f:
        for row in f.read().splitlines():
            if row.startswith("["):
                cur = out[row.strip("[]")]
            elif row.strip():
                cur.append(row)
    return out


CENSUS = {cfg: _committed(*cfg) for cfg in CONFIGS}
IDS = [f"{level}-{batch}" for level, batch in CONFIGS]


def _new_lines():
    """(configuration, index in its list, line) of every line no earlier list holds: the headline's first, then CONFIGS in order."""
    seen, out = set(HEADLINE), []
    for cfg in CONFIGS:
        for i, line in enumerate(CENSUS[cfg]["launches"]):
            if line not in seen:
                seen.add(line)
                out.append((cfg, i, line))
    return out


NEW = _new_lines()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_step_launches_are_all_covered(cfg, monkeypatch):
    """Every launch of the step is in the configuration's committed list (a SUBSET: a new shape or flag combination fails until it
    is listed and checked below), no weight gradient is left outside a flushed sweep, and the two sweeps are the committed ones,
    layer for layer."""
    level, batch = cfg
    c = step_census(monkeypatch, level, batch)
    listed = set(CENSUS[cfg]["launches"])
    missing = [s for s in (spec(r) for r in c.distinct if _launch(r[0])) if s not in listed]
    assert not missing, f"launches of the level-{level} batch-{batch} step without a check at that shape:\n" + "\n".join(missing)
    assert all(r[0] != "conv3x3_wgrad" or dict(r[1]).get("defer") == "WgradDefer" for r in c.calls)
    assert sweeps_of(c.calls) == [CENSUS[cfg]["critic sweep"], CENSUS[cfg]["generator sweep"]]


@pytest.mark.parametrize("line", [line for _, _, line in NEW],
                         ids=[f"{cfg[0]}-{cfg[1]}-{i:03d}-{line.split()[0]}" for cfg, i, line in NEW])
def test_launch_against_float64(line):
    check_launch(line)


@pytest.mark.parametrize("sweep", ["critic", "generator"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_weight_gradient_sweep(cfg, sweep):
    terms = check_sweep(CENSUS[cfg][f"{sweep} sweep"], sweep)
    print(f"level {cfg[0]} batch {cfg[1]} {sweep} sweep: largest fp32 term w {max(t[0] for t in terms):.2e} b {max(t[1] for t in terms):.2e}")


# ------------------------------------------------------------------ would the checks notice?
def _kind(line):
    """The kind of launch a line is for the sensitivity cases: its op, and for the 3x3 convs (conv3x3, conv3x3_small) the branch of
    launch_checks._check_conv that compares it, in that function's order: the fused un-pooling through a tile mask or a float
    activation, the block sums, the tile mask it writes, the tile-mask bytes or the float activation it reads (writing over the
    activation, pooled), PixelNorm, the pooled pair, the plain conv (up-sampled input or not)."""
    name, args = parse(line)
    a = dict(args)
    if name in ("conv3x3", "conv3x3_small"):
        pooled = a.get("pool", False) or a.get("pool_out") is not None
        mask = a.get("mask_aux")
        if a.get("unpool_mask") is not None:
            kind = "unpool_mask"
        elif a.get("unpool_aux") is not None:
            kind = "unpool_aux"
        elif a.get("upsum"):
            kind = "upsum"
        elif a.get("mask_out"):
            kind = "mask_out"
        elif mask is not None:
            kind = ("mask_bytes" if mask[0] == "u8" else "mask_float") + ("_out" if a.get("out") is not None else "") + \
                ("_pooled" if pooled else "")
        elif a.get("pixnorm"):
            kind = "pixnorm"
        elif pooled:
            kind = "pooled"
        else:
            kind = "ups" if a.get("ups") else "plain"
        return f"{name}-{kind}"
    if name == "conv3x3_fade":
        return f"{name}-mode{a['mode']}"
    if name == "conv1x1":  # the comparison of launch_checks._check_conv1x1 it takes
        kind = "transposed" if a.get("transposed") else "tanh" if a.get("tanh") else "lrelu" if a.get("lrelu") else "masked"
        return f"{name}-{kind}"
    return name


def _first_of_each_kind():
    """kind -> the first line of that kind, in the order of CONFIGS ((3, 8) for nearly all; (0, 6) for the lone 1x1 convs)."""
    out = {}
    for cfg in CONFIGS:
        for line in CENSUS[cfg]["launches"]:
            out.setdefault(_kind(line), line)
    return out


KINDS = _first_of_each_kind()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_check_notices_one_wrong_element(kind):
    line = KINDS[kind]
    whats = []
    check_launch(line, listen(whats))
    must_notice(lambda hook: check_launch(line, hook), whats)


def test_sweep_check_notices_one_wrong_element():
    """The same for the weight and bias gradient of the first and the last layer of the (3, 8) critic sweep."""
    lines = CENSUS[CONFIGS[0]]["critic sweep"]
    whats = []
    check_sweep(lines, "critic", listen(whats))
    assert len(whats) == 2 * len(lines)
    must_notice(lambda hook: check_sweep(lines, "critic", hook), whats[:2] + whats[-2:])

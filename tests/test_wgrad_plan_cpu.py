"""The weight gradient's launch planner (csrc/wino_wgrad_plan.h) without a device: compiled by plain g++ (tests/wgrad_plan_shim.py).

1. tests/wgrad_plans.txt holds what the library answered on an MI355X BEFORE the planner was separated from the kernels' file, for
   every weight-gradient sweep the tests hold (the four census files and the headline step), under four switch settings: form,
   workspace bytes and each returned job's nsplit / CinP / CoutP.  The planner must give the same numbers for that CU count.
2. Over a grid of layers, device sizes and rows modes the census does not reach: the invariants a launch relies on -- above all
   that no re-plan (row-staged, grouped) uses more splits than the chunk plan the workspace was sized by.
3. "Small enough to share a grouped launch" is one rule: the form query and the sweep planner agree on it."""
import itertools
import os

import numpy as np
import pytest

import wgrad_plan_shim as shim

HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = {"group32": (32, {}), "group0": (0, {}), "rows0": (32, {"rows": 0}), "rows2": (32, {"rows": 2})}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return shim.load(tmp_path_factory.mktemp("wgrad_plan"))  # that the header compiles with plain g++ is the first assertion


def recorded():
    """(n_cu, [(sweep name, [layer dict])]) of tests/wgrad_plans.txt; a layer the sweep hands to another kernel has nsplit None."""
    n_cu, sweeps = None, []
    for line in open(os.path.join(HERE, "wgrad_plans.txt")):
        line = line.strip()
        if line.startswith("#"):
            if "n_cu=" in line:
                n_cu = int(line.split("n_cu=")[1].split()[0])
        elif line.startswith("["):
            sweeps.append((line[1:line.index("]")], []))
        elif line:
            kv = dict(t.split("=", 1) for t in line.split())
            layer = {k: int(kv[k]) for k in ("N", "Cin", "Cout", "H", "W", "ups")}
            layer["ws_bytes"] = None if kv["ws_bytes"] == "-" else int(kv["ws_bytes"])
            for s in SETTINGS:
                layer[s] = [None if v == "-" else int(v) for v in kv[s].split(",")]  # form, nsplit, CinP, CoutP
            sweeps[-1][1].append(layer)
    return n_cu, sweeps


def shapes_of(layers):
    return np.array([[a["N"], a["Cin"], a["Cout"], a["H"], a["W"], a["ups"]] for a in layers], dtype=np.int32)


def test_fixture_covers_every_sweep_the_tests_hold():
    n_cu, sweeps = recorded()
    assert n_cu == 256
    assert [name for name, _ in sweeps] == [f"{lv} {s}" for lv in ("level3_batch8", "level4_batch32", "level6_batch6", "level7_batch6",
                                                                   "level5_batch64") for s in ("critic", "generator")]
    from routing_census import parse
    import test_headline_shapes_gpu as headline
    for lv in ("level3_batch8", "level4_batch32", "level6_batch6", "level7_batch6", "level5_batch64"):
        text = open(os.path.join(HERE, f"census_{lv}.txt")).read() if lv != "level5_batch64" else None
        for s in ("critic", "generator"):
            lines = text.split(f"[{s} sweep]\n")[1].split("\n[")[0].strip().split("\n") if text is not None else \
                (headline.CRITIC_SWEEP if s == "critic" else headline.GENERATOR_SWEEP)
            got = dict(sweeps)[f"{lv} {s}"]
            assert len(got) == len(lines)
            for a, line in zip(got, lines):
                r = dict(parse(line)[1])
                assert (a["N"], a["Cin"], a["Cout"], a["H"], a["W"], a["ups"]) == (*r["gy"][:1], r["x"][1], *r["gy"][1:], int(r.get("ups", False)))


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_planner_reproduces_the_recorded_plans(lib, setting):
    n_cu, sweeps = recorded()
    group, sw = SETTINGS[setting]
    checked = 0
    for name, layers in sweeps:
        taken = [a for a in layers if a[setting][1] is not None]  # the layers that reached mg_wino3x3_wgrad_partial_multi
        p = shim.plan(lib, shapes_of(taken), len(taken), group, n_cu, shim.switches(lib, **sw))
        assert p.broken == 0
        for i, a in enumerate(taken):
            form, nsplit, cinp, coutp = a[setting]
            got = (int(p.form[i]), int(p.nsplit[i]), int(p.CinP[i]), int(p.CoutP[i]), 4 * int(p.ws_floats[i]))
            assert got == (form, nsplit, cinp, coutp, a["ws_bytes"]), (name, i, setting, got, a)
            checked += 1
        rest = [a for a in layers if a[setting][1] is None and a[setting][0] >= 0]  # never planned as a sweep: the form query only
        if rest:
            q = shim.plan(lib, shapes_of(rest), 1, group, n_cu, shim.switches(lib, **sw))
            assert [int(f) for f in q.form] == [a[setting][0] for a in rest]
    assert checked >= 100


def test_the_small_layer_rule_exists_once(lib):
    """Form query and sweep planner on every recorded layer: grouped-as-small is the same answer from both."""
    n_cu, sweeps = recorded()
    for name, layers in sweeps:
        layers = [a for a in layers if a["H"] % 2 == 0 and a["W"] % 2 == 0]
        grouped = shim.plan(lib, shapes_of(layers), len(layers), 32, n_cu, shim.switches(lib))
        alone = shim.plan(lib, shapes_of(layers), len(layers), 0, n_cu, shim.switches(lib))
        small_by_sweep = grouped.small != 0
        assert not alone.small.any()
        # the form query says "chunk-staged" for a small layer whatever its row-staged form would be, and nothing else differs
        assert (grouped.form == np.where(small_by_sweep, 0, alone.form)).all(), name
        assert ((grouped.rows != 0) == (~small_by_sweep & (alone.rows != 0))).all(), name
        assert ((grouped.group >= 0) <= small_by_sweep).all(), name  # only small layers are ever in a group


# ------------------------------------------------------------------ invariants over a grid
CH = (2, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 256)
MAPS = [(s, s) for s in (2, 4, 8, 16, 32, 64, 128, 256, 512)] + [(32, 64), (64, 32), (512, 32)]


def grid():
    g = np.array([(n, ci, co, h, w, u) for n, ci, co, (h, w), u in itertools.product((1, 2, 6, 8, 24, 64), CH, CH, MAPS, (0, 1))],
                 dtype=np.int64)
    ok = (g[:, 0] * np.maximum(g[:, 1], g[:, 2]) * g[:, 3] * g[:, 4]) < (1 << 29)  # the entry points refuse the others
    return g[ok].astype(np.int32)


def check_layers(p, where):
    """What every launch relies on, for final plans (after rows / group re-planning)."""
    chunk = p.rows == 0
    assert ((p.CT >= 1) & (p.CT <= 4) & (p.OT >= 1) & (p.OT <= 4)).all(), where
    assert (p.CT * p.ncb * 16 >= p.CinP).all() and (p.OT * p.nob * 16 >= p.CoutP).all(), where
    assert ((p.TBW * p.TBH * p.TBN)[chunk] == 8).all(), where
    assert ((1 << p.lgTBW) == p.TBW).all() and ((1 << p.lgTBH) == p.TBH).all(), where
    assert (p.nblk == p.blocks_x * p.blocks_y * p.blocks_n).all(), where
    assert (p.nsplit >= 1).all() and (p.per * p.nsplit >= p.nblk).all() and (p.per * (p.nsplit - 1) < p.nblk).all(), where  # no empty slab
    assert (p.ws_floats == p.nsplit_ws * (9 * p.CinP * p.CoutP + p.CoutP)).all(), where
    assert (p.nsplit <= p.nsplit_ws).all(), where  # the workspace invariant: rows and group members alike
    rows = ~chunk
    assert not ((p.CT == 4) & (p.OT == 4) & rows).any() and ((p.W % 32)[rows] == 0).all(), where
    assert ((p.TBW == 16) & (p.TBH == 1) & (p.TBN == 1))[rows].all(), where
    fast = p.fast != 0
    assert ((p.TBW == 8) & (p.TBH == 1) & (p.TBN == 1) & (p.W % 16 == 0))[fast].all(), where
    # the reduce: every job gets at least one workgroup (increasing prefix sums) and its workgroups cover the padded filter
    assert np.isin(p.reduce_lanes, (8, 32)).all() and (p.reduce_blocks >= 1).all(), where
    assert (p.reduce_blocks * (512 // p.reduce_lanes) >= p.CinP * p.CoutP).all(), where
    assert ((p.reduce_blocks - 1) * (512 // p.reduce_lanes) < p.CinP * p.CoutP).all(), where


@pytest.mark.parametrize("n_cu", [64, 256, 304])
@pytest.mark.parametrize("rows", [0, 1, 2])
def test_invariants_over_the_grid(lib, n_cu, rows):
    g, sw = grid(), shim.switches(lib, rows=rows)
    per = 18
    inlined = [lib.shim_var(ct, ot, u) for ct in (3, 4) for ot in (3, 4) for u in (0, 1)]
    for group in (0, 32):
        p = shim.plan(lib, g, per, group, n_cu, sw)
        where = (n_cu, rows, group)
        assert p.broken == 0, where
        assert (p.table[:, :5] == g[:, :5]).all()
        check_layers(p, where)
        if rows == 0:
            assert not p.rows.any()
        if group == 0:
            assert (p.group == -1).all() and not p.small.any()
            continue
        # every layer is launched exactly once: in one group of its own sweep, or alone
        sweep = np.arange(len(g)) // per
        assert ((p.group >= -1) & (p.group < lib.shim_limits(1) // 2)).all()
        member = p.group >= 0
        assert member.any() and (~member).any()
        gid = sweep[member] * 64 + p.group[member]  # one number per group
        ids, inverse, size = np.unique(gid, return_inverse=True, return_counts=True)
        assert (size >= 2).all() and (size <= lib.shim_limits(0)).all(), where
        # members: chunk-staged, of a block shape the group kernel has inlined (each member carries its own: the kernel selects
        # the body per member, so a group may mix them)
        assert (p.small[member] != 0).all() and (p.rows[member] == 0).all(), where
        assert np.isin(p.var[member], inlined).all() and ((p.CT >= 3) & (p.OT >= 3))[member].all(), where
        # a group fills the chip at most once, unless it cannot shrink any further
        wgs = np.bincount(inverse, weights=(p.nsplit * p.ncb * p.nob)[member]).astype(np.int64)
        floor = np.bincount(inverse, weights=(p.nsplit[member] > 1)) == 0
        assert ((wgs <= n_cu) | floor).all(), where

"""The forward / data-gradient Winograd convolution's launch planner (csrc/wino_plan.h) without a device: compiled by plain g++
(tests/wino_plan_shim.py).

1. tests/wino_plans.txt holds what the library decided BEFORE the planner was separated from the kernels' files, for every Winograd
   call the tests hold (the four census files and the headline step) at 256 CUs, under six switch settings.  Per call, one line per
   setting and per_cu (what the strip kernel's occupancy query answered; 0 where the staged kernel takes the call, which does not ask):
     <setting> <per_cu> strip  <status> niw nwave kind pool rows g_full g_pad grid lds
     <setting> <per_cu> staged <status> cfg wt TBW TBH TBN blocks_x blocks_y blocks_n grid_x grid_y lds      (status != 0: status only)
   The planner must give the same numbers.
2. Over a grid of layers, flags, device sizes and switches the census does not reach: the invariants a launch relies on -- above all
   that the strip kernel's own decode of blockIdx.x finds every workgroup of the planned grid a row and a place in it."""
import itertools
import os

import numpy as np
import pytest

import wino_plan_shim as shim
from routing_census import parse

HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = {"default": {}, "strip0": {"strip": 0}, "strip2": {"strip": 2}, "cfg2wt4": {"cfg": 2, "wt": 4}, "narrow0": {"narrow": 0},
            "niw3": {"strip_niw": 3}}
LEVELS = ("level3_batch8", "level4_batch32", "level6_batch6", "level7_batch6", "level5_batch64")
STRIP_COLS = "niw nwave kind pool rows g_full g_pad grid lds".split()
STAGED_COLS = "cfg wt TBW TBH TBN blocks_x blocks_y blocks_n grid_x grid_y st_lds".split()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return shim.load(tmp_path_factory.mktemp("wino_plan"))  # that the header compiles with plain g++ is the first assertion


def recorded():
    """(n_cu, [(level, [(record line, [(setting, per_cu, form, [numbers])])])]) of tests/wino_plans.txt"""
    n_cu, levels = None, []
    for line in open(os.path.join(HERE, "wino_plans.txt")):
        if line.startswith("#"):
            if "n_cu=" in line:
                n_cu = int(line.split("n_cu=")[1].split(")")[0])
        elif line.startswith("["):
            levels.append((line.strip()[1:-1], []))
        elif line.startswith(" "):
            setting, per_cu, form, *nums = line.split()
            levels[-1][1][-1][1].append((setting, int(per_cu), form, [int(v) for v in nums]))
        elif line.strip():
            levels[-1][1].append((line.strip(), []))
    return n_cu, levels


def wino_calls(level):
    """The distinct Winograd conv records the tests hold for a level, in order of first appearance."""
    if level == "level5_batch64":
        import test_headline_shapes_gpu as headline
        lines = headline.LAUNCHES
    else:
        lines = [ln.strip() for ln in open(os.path.join(HERE, f"census_{level}.txt")) if ln.strip() and not ln.startswith("[")]
    return list(dict.fromkeys(ln for ln in lines if ln.split()[0] in ("conv3x3", "conv3x3_fade") and shim.layer_of(parse(ln)) is not None))


def test_fixture_covers_every_winograd_call_the_tests_hold():
    n_cu, levels = recorded()
    assert n_cu == 256
    assert [lv for lv, _ in levels] == list(LEVELS)
    for lv, calls in levels:
        want = wino_calls(lv)
        assert len(want) >= 10, lv
        assert [parse(line) for line, _ in calls] == [parse(line) for line in want], lv
        for line, rows in calls:
            assert {r[0] for r in rows} == set(SETTINGS), line
    # data-gradient calls (bias-free, masked or un-pooling) and the three fade modes are among them
    recs = [dict(parse(line)[1]) | {"op": parse(line)[0]} for _, calls in levels for line, _ in calls]
    assert {r["mode"] for r in recs if r["op"] == "conv3x3_fade"} == {1, 2, 3}
    assert any(r.get("unpool_mask") is not None for r in recs) and any(r["op"] == "conv3x3" and r.get("bias") is None for r in recs)


def test_planner_reproduces_the_recorded_plans(lib):
    n_cu, levels = recorded()
    rows_in_file = sum(1 for line in open(os.path.join(HERE, "wino_plans.txt")) if line.startswith(" "))
    checked = 0
    for lv, calls in levels:
        layers = np.array([shim.layer_of(parse(line)) for line, _ in calls], dtype=np.int32)
        for setting, kw in SETTINGS.items():
            for per_cu in (0, 1, 2, 4):
                p = shim.plan(lib, layers, n_cu, max(per_cu, 1), shim.switches(lib, **kw))
                for i, (line, rows) in enumerate(calls):
                    for s, pc, form, nums in rows:
                        if (s, pc) != (setting, per_cu):
                            continue
                        assert form == ("strip" if p.strip[i] else "staged"), (lv, line, s, pc)
                        cols = ["status"] + (STRIP_COLS if form == "strip" else STAGED_COLS if nums[0] == 0 else [])
                        got = [0 if (c == "status" and form == "strip") else int(getattr(p, c)[i]) for c in cols]
                        assert got == nums, (lv, line, s, pc, dict(zip(cols, got)), nums)
                        checked += 1
    assert checked == rows_in_file and checked >= 1500


# ------------------------------------------------------------------ invariants over a grid
F = shim.FLAGS
CH = (2, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160)
MAPS = [(s, s) for s in (2, 4, 8, 16, 32, 64, 128, 256, 512)] + [(32, 64), (64, 32), (2, 1024), (512, 32), (6, 10)]
# (flags, has_bias, has_y) as ops.conv3x3 / ops._conv3x3_tilemask / ops.conv3x3_fade can produce them
KINDS = [(lr | pool, b, 1) for lr in (0, F["LRELU"]) for pool in (0, F["POOL_OUT"]) for b in (0, 1)] + \
        [(F["MASK_AUX"] | pool, b, 1) for pool in (0, F["POOL_OUT"]) for b in (0, 1)] + \
        [(F["LRELU"] | F["PIXNORM"], b, y) for b in (0, 1) for y in (0, 1)] + \
        [(F["UNPOOL"], 0, 1), (F["MASK_AUX"] | F["MASK_BYTES"], 0, 1)] + \
        [(F["LRELU"] | F["POOL_OUT"] | F["MASK_OUT"], b, 1) for b in (0, 1)] + \
        [(F["MASK_AUX"] | F["POOL_OUT"] | F["MASK_BYTES"], b, 0) for b in (0, 1)] + \
        [(F["BLEND"] | F["LRELU"], b, 1) for b in (0, 1)] + [(F["BLEND"] | F["MASK_AUX"] | F["MASK_BYTES"], b, 1) for b in (0, 1)] + \
        [(F["BLEND_BWD"], 0, 1)]
NINE = {(1, 2), (1, 4), (1, 8), (2, 2), (2, 4), (3, 2), (3, 4), (4, 2), (4, 4)}
LDS_MAX = 160 * 1024


def grid():
    g = np.array([(n, ci, co, h, w, fl, b, y) for n, ci, co, (h, w), (fl, b, y) in
                  itertools.product((1, 2, 6, 8, 18, 24, 64, 192), CH, CH, MAPS, KINDS)], dtype=np.int64)
    ok = ~((g[:, 5] & F["PIXNORM"] != 0) & (g[:, 2] > 64))  # the entry point refuses PixelNorm over more than 64 channels
    return g[ok].astype(np.int32)


def cdiv(a, b):
    return (a + b - 1) // b


def shape_conditions(p):
    """mgi_wino_strip_takes' shape conditions, written out again."""
    nt, pn = p.Cout // 16, (p.flags & F["PIXNORM"]) != 0
    masked = (p.flags & (F["MASK_AUX"] | F["UNPOOL"] | F["BLEND_BWD"])) != 0
    return ((p.Cin % 16 == 0) & (p.Cout % 16 == 0) & (nt <= 10) & (p.W % 32 == 0) & ((p.H // 2) % 8 == 0) & (p.H % 2 == 0) &
            ~(pn & ((nt > 2) | (p.has_y != 0))) & ~(masked & (p.has_bias != 0)) &
            (p.Cout * p.H * p.W * 16 < 2**31) & (p.Cin * p.H * p.W * 4 < 2**31))


def check_staged(p, n_cu, where):
    ok = (p.strip == 0) & (p.status == 0)
    bad = (p.strip == 0) & (p.status != 0)
    mb_y = (p.flags & (F["MASK_BYTES"] | F["POOL_OUT"] | F["BLEND"])) == F["MASK_BYTES"]
    assert ((p.status[bad] == 1) == mb_y[bad]).all() and not mb_y[ok].any(), where
    p = shim.Plans(p.table[ok])
    nt, pn = cdiv(p.Cout, 16), (p.flags & F["PIXNORM"]) != 0
    assert set(zip(p.cfg.tolist(), p.wt.tolist())) <= NINE, where
    assert (cdiv(nt, p.cfg) * p.cfg <= p.NT).all() and (p.nchunk == cdiv(p.Cin, 8)).all(), where
    assert (p.TBW * p.TBH * p.TBN == 16 * p.wt).all(), where
    for v, lg in ((p.TBW, p.lgTBW), (p.TBH, p.lgTBH), (p.TBN, None)):
        assert ((v & (v - 1)) == 0).all() and (v >= 1).all() and (lg is None or ((1 << lg) == v).all()), where
    assert (p.blocks_x * p.TBW >= p.W // 2).all() and (p.blocks_y * p.TBH >= p.H // 2).all() and (p.blocks_n * p.TBN >= p.N).all(), where
    assert (p.TBN * p.Cin * p.H * p.W < 2**29).all(), where
    assert (p.grid_y == cdiv(nt, p.cfg)).all() and (p.grid_y[pn] == 1).all(), where
    blocks = p.blocks_x * p.blocks_y * p.blocks_n
    fewer = p.grid_x < blocks
    assert (p.grid_x >= 1).all() and (p.grid_x <= blocks).all() and (fewer == (p.persistent != 0)).all(), where
    assert (p.wt[fewer] >= 4).all() and (p.grid_x[fewer] == n_cu).all(), where
    niw, wc = np.where(p.cfg == 4, 2, 1), np.where(p.cfg == 4, 2, p.cfg)
    lds = 4 * (16 * (16 * p.wt) * 8 + wc * niw * 2048 + wc * (16 * p.wt) * 4)  # launch_wino
    assert (p.st_lds == lds).all() and (lds <= LDS_MAX).all(), where


def decode(rows, g_full, g_pad, niw, grid):
    """wino3x3_strip's own decode of blockIdx.x, for every workgroup of a grid: (row, place in the row, one-tile body)."""
    idx = np.arange(grid)
    row = np.where(idx < (rows - (1 if g_pad else 0)) * g_full, idx // g_full, rows - 1)
    wg = idx - row * g_full
    return row, wg, (niw == 2) & (g_pad != 0) & (row == rows - 1)


def check_strip(p, where):
    assert ((p.strip != 0) <= shape_conditions(p)).all() and (shape_conditions(p) == (p.shape_ok != 0)).all(), where
    p = shim.Plans(p.table[p.strip != 0])
    nt, pn = p.Cout // 16, (p.flags & F["PIXNORM"]) != 0
    assert np.isin(p.niw, (1, 2, 3)).all() and (nt[p.niw == 3] == 3).all() and (p.nwave == np.where(p.niw == 3, 4, 8)).all(), where
    assert ((p.niw == nt) & (nt <= 2))[pn].all(), where
    assert (p.lds == (p.Cin // 8) * p.niw * 8192).all() and (p.lds <= LDS_MAX).all(), where
    assert (p.rows == cdiv(nt, p.niw)).all() and (p.s_nchunk * 8 == p.Cin).all(), where
    assert ((p.s_blocks_x == p.W // 32) & (p.s_blocks_y == p.H // 2)).all(), where
    nitems = p.N * (p.s_blocks_y // p.nwave) * p.s_blocks_x
    has_pad = p.g_pad != 0
    assert ((p.niw == 2) & (nt % 2 == 1) & (p.rows > 1))[has_pad].all(), where
    assert ((p.g_full >= 1) & (p.g_full <= nitems) & (p.g_pad >= 0) & (p.g_pad <= nitems)).all(), where
    assert (p.grid == (p.rows - has_pad) * p.g_full + p.g_pad).all(), where
    # the kernel's decode over every workgroup index, once per distinct grid layout
    assert ((p.g_full < 2**20) & (p.g_pad < 2**20) & (p.rows < 16)).all(), where
    for key in np.unique(((p.g_full * 2**20 + p.g_pad) * 16 + p.rows) * 4 + p.niw).tolist():
        g_full, g_pad, rows, niw = key >> 26, (key >> 6) & (2**20 - 1), (key >> 2) & 15, key & 3
        grid = (rows - (1 if g_pad else 0)) * g_full + g_pad
        row, wg, one_tile = decode(rows, g_full, g_pad, niw, grid)
        count = np.where((np.arange(rows) == rows - 1) & (g_pad != 0), g_pad, g_full)
        assert (row >= 0).all() and (row < rows).all() and (wg >= 0).all() and (wg < count[row]).all(), (where, rows, g_full, g_pad)
        assert (np.bincount(row, minlength=rows) == count).all(), (where, rows, g_full, g_pad)
        assert (one_tile <= (row == rows - 1)).all() and one_tile[row == rows - 1].all() == bool(g_pad and niw == 2), where
    # the kinds that are instantiated: pooled or not as the epilogue has it
    pooled = (p.flags & F["POOL_OUT"]) != 0
    assert ((p.pool != 0) == pooled).all(), where


def check_both(p, strip_mode, where):
    mb = p.flags == (F["MASK_AUX"] | F["MASK_BYTES"])
    assert ((p.mask_bytes_y != 0)[mb] == (p.strip != 0)[mb]).all(), where
    if strip_mode == 0:
        assert not p.strip.any() and not p.mask_bytes_y.any(), where
    if strip_mode == 2:  # every shape that passes the shape conditions and whose filter bank fits LDS
        nt, pn = p.Cout // 16, (p.flags & F["PIXNORM"]) != 0
        fits = (p.Cin // 8) * np.where(pn, nt, 1) * 8192 <= LDS_MAX
        assert ((p.strip != 0) == (shape_conditions(p) & fits)).all(), where


STAGED_SWITCHES = [{"cfg": c, "wt": w} for c in (None, 2, 3, 4, 0) for w in (None, 2, 4, 0)] + \
    [{"narrow": 0}, {"narrow_wt": 4}, {"narrow_wt": 8}, {"few": 0}, {"persist": 0}]  # (0: set, to no value the override takes)
STRIP_SWITCHES = [{}, {"strip": 2}, {"strip_niw": 1}, {"strip_niw": 2}, {"strip_niw": 3}, {"strip": 2, "strip_niw": 3}, {"strip_wgs": 1},
                  {"strip_wgs": 3}, {"strip_wgs": 8}, {"strip_padw": 0.6}, {"strip_padw": 1.0}, {"strip_min_blocks": 1},
                  {"strip_min_blocks": 4096}, {"strip_ablate": 6}]


@pytest.mark.parametrize("n_cu", [64, 256, 304])
def test_staged_invariants_over_the_grid(lib, n_cu):
    g = grid()
    # every flag combination under every switch: everything on the staged kernel (strip = 0), what the strip kernel leaves it, and
    # under the default switches also what it leaves when it takes all it can
    for kw in [{"strip": 2}] + STAGED_SWITCHES:
        kw = {k: v for k, v in kw.items() if v is not None}
        for strip in (kw["strip"],) if "strip" in kw else (0, 1):
            p = shim.plan(lib, g, n_cu, 1, shim.switches(lib, **{"strip": strip, **kw}))
            assert (p.table[:, :8] == g).all()
            check_staged(p, n_cu, (n_cu, kw, strip))
            check_both(p, strip, (n_cu, kw, strip))
            staged = (p.strip == 0) & (p.status == 0)
            if kw.get("cfg") in (2, 4):
                assert (p.cfg[staged & ((p.flags & F["PIXNORM"]) == 0)] == kw["cfg"]).all()
            if kw.get("wt") in (2, 4):
                assert (p.wt[staged] == kw["wt"]).all()
            if kw.get("persist") == 0:
                assert not p.persistent.any()


@pytest.mark.parametrize("n_cu", [64, 256, 304])
def test_strip_invariants_over_the_grid(lib, n_cu):
    g = grid()
    g = g[shape_conditions(shim.Plans(np.pad(g.astype(np.int64), ((0, 0), (0, len(shim.FIELDS) - 8)))))]  # (the others: the test below)
    taken = 0
    for kw in STRIP_SWITCHES:
        # every admissible per_cu: the planner caps it at 16 / NWAVE, i.e. at 2 unless strip_niw = 3 makes four-wave workgroups;
        # strip_wgs replaces it
        for per_cu in (1,) if "strip_wgs" in kw else (1, 2, 3, 4) if kw.get("strip_niw") == 3 else (1, 2):
            p = shim.plan(lib, g, n_cu, per_cu, shim.switches(lib, **kw))
            check_strip(p, (n_cu, kw, per_cu))
            check_staged(p, n_cu, (n_cu, kw, per_cu))
            check_both(p, kw.get("strip", 1) if "strip_niw" not in kw else None, (n_cu, kw, per_cu))
            assert (p.ablate == kw.get("strip_ablate", 0))[p.strip != 0].all()
            if per_cu == 2 and kw.get("strip_niw") != 3:  # (the cap)
                assert (shim.plan(lib, g, n_cu, 4, shim.switches(lib, **kw)).table == p.table).all()
            taken += int(p.strip.sum())
    assert taken > 100000


def test_strip_never_takes_what_fails_its_shape_conditions(lib):
    g = grid()
    for strip in (1, 2):
        p = shim.plan(lib, g, 256, 2, shim.switches(lib, strip=strip))
        check_strip(p, strip)
        check_both(p, strip, strip)
        assert p.strip.any() and (p.strip == 0).any()

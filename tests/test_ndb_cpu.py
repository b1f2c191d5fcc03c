"""CPU: the NDB / JSD statistics on hand examples, the float64 restatement of k-means (tests/ndb_ref.py, the yardstick of
test_ndb_gpu.py) on the GPU tests' own cases -- whose margins must be wide enough to mean something by the reference alone --, the
`ndb` value of the `evaluate` sub-command's `--metrics`, the wrappers' docstrings and argument checks, and the scratch use of the new
kernels."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ndb_ref as N  # noqa: E402


@pytest.mark.parametrize("index", range(len(N.HAND)), ids=["two_bins", "same", "empty_bin", "one_bin"])
def test_hand_examples(index):
    from musicgan_amd import metrics
    a, b, different, ndb, jsd = N.HAND[index]
    for got in (N.statistics(a, b), metrics.ndb_statistics(a, b)):       # the yardstick and the module-level function
        assert got["different"] == different and got["ndb"] == ndb
        assert abs(got["jsd"] - jsd) <= 1e-9, got["jsd"]
        assert len(got["z"]) == len(a)
    z = metrics.ndb_statistics(a, b)["z"]
    if index == 0:
        assert abs(z[0] + 2.8867513459) <= 1e-9 and abs(z[1] - 2.8867513459) <= 1e-9
    if index == 1:
        assert z == [0.0] * 4 and metrics.ndb_statistics(a, b)["jsd"] == 0.0
    if index == 2:
        assert z[4] == 0.0 and abs(max(abs(v) for v in z) - 1.129) <= 1e-3   # the empty bin has se = 0
    assert metrics.NDB_Z == N.Z == 1.959963984540054


def test_statistics_refuse_what_is_no_pair_of_histograms():
    from musicgan_amd import metrics
    for a, b in (((1, 2), (1, 2, 3)), ((), ()), ((1, -1), (1, 1)), ((0, 0), (1, 1)), ((1, 1), (0, 0)), ((1.5, 1), (1, 1))):
        with pytest.raises(ValueError):
            metrics.ndb_statistics(a, b)


@pytest.mark.parametrize("index", range(len(N.PLANTED)), ids=N.PLANTED_IDS)
def test_planted_cases_keep_their_margin_by_the_reference_alone(index):
    """at every assignment, every point's gap between its best and any other float64 distance is at least 100 x the sum of the two
    derived distance bounds: a GPU within the bounds must find the float64 labels.  Measured with this recipe: 1.44e4, 1.55e4,
    1.66e4 x.  The float64 k-means finds the planted blobs at the first assignment and changes nothing afterwards."""
    from musicgan_amd import nn_ops
    p = N.planted(index, nn_ops.nn_chunk())
    n, d, k, iters = N.PLANTED[index]
    print(f"planted {N.PLANTED_IDS[index]}: margin {p['margin']:.1f} x the bounds, changed {p['changed']}, sizes {p['count']}")
    assert p["margin"] >= N.MARGIN
    assert torch.equal(p["labels"], p["truth"]) and p["changed"] == [n] + [0] * iters
    assert p["count"] == [(n - j + k - 1) // k for j in range(k)]
    assert p["centroids"].dtype == torch.float32
    assert bool(((p["centroids"].double() - p["mean"]).abs() <= p["bound"]).all())     # the reference meets its own bound


@pytest.mark.parametrize("index", range(len(N.GENERAL)), ids=N.GENERAL_IDS)
def test_general_cases_leave_few_points_undecided_by_the_reference_alone(index):
    from musicgan_amd import nn_ops
    g = N.general(index, nn_ops.nn_chunk())
    print(f"general {N.GENERAL_IDS[index]}: undecided points {100 * g['undecided']:.2f} %")
    assert g["undecided"] <= N.UNDECIDED_CAP
    assert len(set(g["labels"].tolist())) == g["k"]                       # every bin is used: not degenerate


def test_reference_kmeans_on_a_line():
    """points 0, 1, 2, 10, 11 with centroids at the rows 0 and 1: 0 | 1 2 10 11 -> means 0, 6 -> 0 1 2 | 10 11 -> means 1, 10.5"""
    x = torch.tensor([[0.0], [1.0], [2.0], [10.0], [11.0]])
    c, labels, changed, _ = N.kmeans(x, (0, 1), 3)
    assert labels.tolist() == [0, 0, 0, 1, 1] and c.reshape(-1).tolist() == [1.0, 10.5] and changed == [5, 2, 0, 0]
    tie = torch.tensor([[1.0, 1.0, 0.5], [2.0, 1.0, 1.0], [3.0, 3.0, 3.0]], dtype=torch.float64)
    assert N.argmin_first(tie).tolist() == [2, 1, 0]
    mean, bnd, count = N.means(x, torch.tensor([0, 0, 0, 2, 2]), torch.tensor([[7.0], [8.0], [9.0]]))
    assert mean.reshape(-1).tolist() == [1.0, 8.0, 10.5] and count == [3, 0, 2] and float(bnd[1]) == 0.0


def test_metrics_option_of_the_evaluate_parser_accepts_ndb():
    from musicgan_amd.__main__ import _METRICS, _METRICS_ALL, _METRICS_EVERY, _MODES, build_parser
    p = build_parser()
    _, _, _, pos, kw = _MODES["evaluate"]
    today = ["evaluate", "g.pt", "8", "-i", "d", "--level", "2", "-n", "8"]
    assert "metrics" not in kw(p.parse_args(today))
    assert kw(p.parse_args(today + ["--metrics", "ndb"]))["metrics"] == ("ndb",)
    assert kw(p.parse_args(today + ["--metrics", "swd,msssim,nn,prdc,ndb"]))["metrics"] == ("swd", "msssim", "nn", "prdc", "ndb")
    assert _METRICS == ("swd", "msssim", "nn") and _METRICS_ALL == _METRICS + ("prdc",) and _METRICS_EVERY == _METRICS_ALL + ("ndb",)
    for bad in ("fid", "ndb,fid", "", "ndb,ndb", "swd,ndb,swd"):
        with pytest.raises(SystemExit):
            p.parse_args(today + ["--metrics", bad])
    sub = [a for a in p._subparsers._group_actions[0].choices["evaluate"]._actions if a.dest == "metrics"][0]
    assert sub.metavar == "swd,msssim,nn,prdc,ndb" and "ndb_real" in sub.help


def test_evaluate_knows_the_metric_and_refuses_bad_requests_before_any_work():
    import musicgan_amd
    assert callable(musicgan_amd.evaluate)                                # (loads the module: the package's attributes are lazy)
    mod = sys.modules["musicgan_amd.evaluate"]
    assert mod.METRICS == ("swd", "msssim", "nn") and mod.METRICS_ALL == mod.METRICS + ("prdc",) and mod.METRICS_ALL[-1] == "prdc"
    assert mod.METRICS_EVERY == mod.METRICS_ALL + ("ndb",)
    for bad in (("ndb", "ndb"), ("ndb", "fid"), ()):
        with pytest.raises(ValueError):
            musicgan_amd.evaluate("missing.pt", 8, "missing", bad)
    with pytest.raises(ValueError, match="at least 8"):
        musicgan_amd.evaluate("missing.pt", 8, "missing", ("ndb",), nb_images=7)       # before the file is opened
    assert [mod._ndb_bins(h) for h in (4, 39, 40, 60, 999, 1000, 4096)] == [2, 2, 2, 3, 49, 50, 50]


def test_every_new_wrapper_names_what_it_writes():
    from musicgan_amd import km_ops, nn_ops, ops
    doc = km_ops.km_assign.__doc__
    assert "all of label" in doc and "all of mind" in doc and "overwritten, not accumulated" in doc
    doc = km_ops.km_order.__doc__
    assert "all of start" in doc and "all of order" in doc
    assert "in place" in km_ops.km_update.__doc__ and "keeps its bits" in km_ops.km_update.__doc__
    assert "accumulated in place" in km_ops.km_count.__doc__
    assert "host query" in km_ops.km_update_ws_bytes.__doc__
    assert {"km_assign", "km_order", "km_update", "km_update_ws_bytes", "km_count"} <= set(vars(km_ops))
    assert not [n for n in vars(ops) if "km_" in n.lower() or "kmeans" in n.lower()]
    assert not [n for n in vars(nn_ops) if "km_" in n.lower() or "kmeans" in n.lower()]


def test_host_query_and_argument_checks_need_no_gpu():
    from musicgan_amd import _lib, km_ops, metrics
    assert km_ops.km_update_ws_bytes(4096, 32768, 50) == (4096 // 32 + 50) * 32768 * 8   # a slot per 32 members and one per bin
    assert km_ops.km_update_ws_bytes(37, 231, 5) == (1 + 5) * 231 * 8
    assert km_ops.km_update_ws_bytes(0, 8, 2) == 0 and km_ops.km_update_ws_bytes(8, 0, 2) == 0
    z = torch.zeros
    f64, i64, i32 = dict(dtype=torch.float64), dict(dtype=torch.int64), dict(dtype=torch.int32)
    with pytest.raises(_lib.MusicGanHipError):
        km_ops.km_assign(z(4, 3, **f64), z(4, **i32), z(4, **f64), z(1, **i64))
    with pytest.raises(_lib.MusicGanHipError):
        km_ops.km_order(z(4, **i32), 3)
    with pytest.raises(_lib.MusicGanHipError):
        km_ops.km_update(z(4, 8), z(4, **i32), z(4, **i32), z(3, 8))
    with pytest.raises(_lib.MusicGanHipError):
        km_ops.km_count(z(4, **i32), z(3, **i64))
    for kw in (dict(bins=1), dict(bins=1025), dict(bins=2.0), dict(bins=True), dict(bins=4, iterations=0), dict(bins=4, iterations=2.5),
               dict(bins=4, iterations=True), dict(bins=4, block_bytes=0), dict(bins=3, init_ids=[0, 1]), dict(bins=3, init_ids=[0, 1, 1]),
               dict(bins=3, init_ids=[0, 1, -2]), dict(bins=3, init_ids=[0, 1, 2.5]), dict(bins=3, seed=1.5)):
        with pytest.raises(ValueError):
            metrics.KMeans(**kw)
    km = metrics.KMeans(bins=3, init_ids=(4, 0, 2))
    assert km.init_ids == [4, 0, 2] and km.iterations == 25 and km.seed == 0
    for use in (km.fit, lambda: km.centroids, lambda: km.assign(z(2, 8))):
        with pytest.raises(ValueError):
            use()                                                         # nothing fed
    with pytest.raises(ValueError):
        km.feed(z(0, 2, 8, 8))
    with pytest.raises(ValueError):
        km.feed(z(4))
    with pytest.raises(_lib.MusicGanHipError):
        km.feed(z(4, 2, 8, 8))                                            # all in order, but not on a GPU
    ndb = metrics.NDB(km)
    with pytest.raises(ValueError):
        ndb.result()                                                      # nothing fed
    with pytest.raises(ValueError):
        ndb.per_bin()
    with pytest.raises(ValueError):
        metrics.NDB("kmeans")
    assert metrics.NDB.KEYS == N.KEYS == ("ndb", "jsd")


def test_kmeans_kernels_do_not_use_scratch_memory():
    from musicgan_amd import _build
    _build.build()
    usage = _build.resource_usage()
    for pat in (r"km_zero_k", r"km_assign_k", r"km_hist_k", r"km_place_k", r"km_partial_k", r"km_finish_k", r"km_count_k"):
        hits = {k: v for k, v in usage.items() if re.search(pat, k)}
        assert hits, f"no kernel matches {pat}"
        for name, u in hits.items():
            assert u.get("ScratchSize [bytes/lane]", 0) == 0, f"{name}: {u.get('ScratchSize [bytes/lane]')} B/lane of scratch memory"
            assert u.get("VGPRs", 0) > 0
    assert len([k for k in usage if re.search(r"km_partial_k", k)]) == 2      # the 16-byte and the element-wise loads

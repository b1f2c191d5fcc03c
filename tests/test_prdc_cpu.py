"""CPU: the float64 restatement of precision / recall / density / coverage (tests/prdc_ref.py, the yardstick of test_prdc_gpu.py)
on a hand example and on the GPU tests' own cases -- whose intervals must be narrow enough to mean something by the reference
alone --, the `prdc` value of the `evaluate` sub-command's `--metrics`, the wrappers' docstrings and argument checks, and the scratch
use of the new kernels."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prdc_ref as P  # noqa: E402


def test_hand_example():
    """reals at 0, 1, 2, 3, fakes at 0.5 and 10, k = 1: every real ball has squared radius 1 and holds 0.5 for the reals 0 and 1;
    both fake balls (squared radius 90.25) hold every real but 0, which is 100 from the fake at 10"""
    real, fake = torch.tensor([[0.0], [1.0], [2.0], [3.0]]), torch.tensor([[0.5], [10.0]])
    got, per = P.prdc(real, fake, 1)
    assert got == {"precision": 0.5, "recall": 1.0, "density": 1.0, "coverage": 0.5}
    assert per["radius_real"].tolist() == [1.0] * 4 and per["radius_fake"].tolist() == [90.25] * 2
    assert per["count_fake"].tolist() == [2, 0] and per["count_real"].tolist() == [1, 2, 2, 2]
    assert per["nearest_fake"].tolist() == [0.25, 0.25, 2.25, 6.25]


@pytest.mark.parametrize("index", range(len(P.CASES)), ids=P.IDS)
def test_the_caps_of_the_gpu_tests_hold_by_the_reference_alone(index):
    """at most 0.5 % of the (query, column) pairs are within the bound of their radius, every number's interval is at most 0.05
    wide, and the inputs are not degenerate.  Measured with this recipe (seeds 90 + n_real), share of undecided pairs / widest
    interval: 64x64x2x32x32 k 3: 0.05 % / 0.010; 40x56x3x7x11 k 2: 0 / 0; 128x96x2x128x128 k 5: 0.10 % / 0.025;
    48x48x2x16x16 k 16: 0.04 % / 0.001."""
    from musicgan_amd import nn_ops
    real, fake, k, iv = P.case(index, nn_ops.nn_chunk())
    widths = {name: iv["hi"][name] - iv["lo"][name] for name in P.KEYS}
    print(f"prdc {P.IDS[index]}: exact {iv['exact']}, undecided pairs {100 * iv['unsure']:.3f} %, widths {widths}")
    assert iv["unsure"] <= P.PAIR_CAP, iv["unsure"]
    for name in P.KEYS:
        assert iv["lo"][name] <= iv["exact"][name] <= iv["hi"][name], name
        assert 0.0 <= widths[name] <= P.WIDTH_CAP, (name, widths[name])
    assert bool((iv["count_fake_lo"] <= iv["per"]["count_fake"]).all()) and bool((iv["per"]["count_fake"] <= iv["count_fake_hi"]).all())
    assert bool((iv["count_real_lo"] <= iv["per"]["count_real"]).all()) and bool((iv["per"]["count_real"] <= iv["count_real_hi"]).all())
    assert 0.1 < iv["exact"]["precision"] and 0.1 < iv["exact"]["recall"] < 0.95      # not degenerate
    assert bool((iv["per"]["radius_real"] > 0).all()) and bool((iv["per"]["radius_fake"] > 0).all())


def test_metrics_option_of_the_evaluate_parser_accepts_prdc():
    from musicgan_amd.__main__ import _METRICS, _METRICS_ALL, _MODES, build_parser
    p = build_parser()
    _, _, _, pos, kw = _MODES["evaluate"]
    today = ["evaluate", "g.pt", "8", "-i", "d", "--level", "2", "-n", "8"]
    assert "metrics" not in kw(p.parse_args(today))
    assert kw(p.parse_args(today + ["--metrics", "prdc"]))["metrics"] == ("prdc",)
    assert kw(p.parse_args(today + ["--metrics", "swd,msssim,nn,prdc"]))["metrics"] == ("swd", "msssim", "nn", "prdc")
    assert _METRICS == ("swd", "msssim", "nn") and _METRICS_ALL == _METRICS + ("prdc",)
    for bad in ("fid", "prdc,fid", "", "prdc,prdc", "swd,prdc,swd"):
        with pytest.raises(SystemExit):
            p.parse_args(today + ["--metrics", bad])


def test_evaluate_knows_the_metric_and_refuses_bad_requests_before_any_work():
    import musicgan_amd
    assert callable(musicgan_amd.evaluate)
    mod = sys.modules["musicgan_amd.evaluate"]
    assert mod.METRICS == ("swd", "msssim", "nn") and mod.METRICS_ALL == mod.METRICS + ("prdc",) and mod.METRICS_ALL[-1] == "prdc"
    assert mod._PRDC_K == 3
    for bad in (("prdc", "prdc"), ("prdc", "fid"), ("swd", "prdc", "swd")):
        with pytest.raises(ValueError):
            musicgan_amd.evaluate("missing.pt", 8, "missing", bad)
    with pytest.raises(ValueError, match="at least 8"):
        musicgan_amd.evaluate("missing.pt", 8, "missing", ("prdc",), nb_images=7)      # two halves of k + 1: before the file is opened


def test_every_new_wrapper_names_what_it_writes():
    from musicgan_amd import nn_ops, ops
    assert "all of out" in nn_ops.nn_sqdist_tiled.__doc__
    doc = nn_ops.prdc_scan.__doc__
    assert "count" in doc and "rowmin" in doc and "accumulated in place" in doc
    assert "host query" in nn_ops.nn_tiled_ws_bytes.__doc__
    assert {"nn_sqdist_tiled", "nn_tiled_ws_bytes", "prdc_scan"} <= set(vars(nn_ops))
    assert not [n for n in vars(ops) if "prdc" in n.lower() or "tiled" in n.lower()]


def test_host_query_and_argument_checks_need_no_gpu():
    from musicgan_amd import _lib, metrics, nn_ops
    assert nn_ops.nn_tiled_ws_bytes(256, 16, 32768) == 16 * 256 * 16 * 8         # 16 float64 per pair, whatever D is
    assert nn_ops.nn_tiled_ws_bytes(5, 37, 231) == 16 * 5 * 37 * 8 == nn_ops.nn_tiled_ws_bytes(5, 37, 1 << 20)
    assert nn_ops.nn_tiled_ws_bytes(0, 16, 64) == 0 and nn_ops.nn_tiled_ws_bytes(4, 4, 0) == 0
    z = torch.zeros
    f64, i64 = dict(dtype=torch.float64), dict(dtype=torch.int64)
    with pytest.raises(_lib.MusicGanHipError):
        nn_ops.nn_sqdist_tiled(z(4, 8), z(3, 8), z(4, **f64), z(3, **f64))
    with pytest.raises(_lib.MusicGanHipError):
        nn_ops.prdc_scan(z(4, 3, **f64), z(3, **f64), z(4, **i64), z(4, **f64))
    for k in (0, 17, -1, 1.5, True):
        with pytest.raises(ValueError):
            metrics.PRDC(k=k)
    with pytest.raises(ValueError):
        metrics.PRDC(block_bytes=0)
    prdc = metrics.PRDC(k=3)
    with pytest.raises(ValueError):
        prdc.result()                                                  # nothing fed
    with pytest.raises(ValueError):
        prdc.feed_real(z(0, 2, 8, 8))
    with pytest.raises(ValueError):
        prdc.feed_fake(z(4))
    with pytest.raises(_lib.MusicGanHipError):
        prdc.feed_real(z(4, 2, 8, 8))                                  # all in order, but not on a GPU
    assert metrics.PRDC.KEYS == P.KEYS


def test_the_row_store_refuses_in_the_words_of_the_class_that_feeds_it():
    """PRDC (two stores, one trailing shape between them) and KMeans (one) keep what they are fed in metrics._RowStore: an empty
    batch, another trailing shape and a CPU tensor are refused with the text each class has always given, and nothing is kept"""
    from musicgan_amd import _lib, metrics
    z = torch.zeros
    prdc, km = metrics.PRDC(k=3), metrics.KMeans(bins=2)
    feeds = (("PRDC", "feed_real", prdc.feed_real, prdc), ("PRDC", "feed_fake", prdc.feed_fake, prdc), ("KMeans", "feed", km.feed, km))
    for owner, what, feed, obj in feeds:
        store = metrics._RowStore(owner)
        for add in (feed, lambda batch: store.add(batch, what, obj.shape)):
            for empty in (z(0, 2, 8, 8), z(4), z(4, 0, 8)):
                with pytest.raises(ValueError) as err:
                    add(empty)
                assert str(err.value) == f"{what}: a non-empty batch (B, ...) expected, got {tuple(empty.shape)}"
            with pytest.raises(_lib.MusicGanHipError) as err:
                add(z(4, 2, 8, 8))                                         # all in order, but not on a GPU
            assert str(err.value) == f"{owner}.{what}: tensors on a ROCm GPU expected (no CPU fallback)"
        assert obj.shape is None                                           # a refused batch does not set the shape
        obj.shape = (2, 8, 8)                                              # as after a first batch of 2 x 8 x 8 images
        for add in (feed, lambda batch: store.add(batch, what, obj.shape)):
            for other in (z(4, 2, 8, 4), z(4, 128)):
                with pytest.raises(ValueError) as err:
                    add(other)
                assert str(err.value) == f"{what}: a batch (B, 2, 8, 8) expected, got {tuple(other.shape)}"
        obj.shape = None
        assert store.n == 0 and not store._parts
    assert prdc._real.n == prdc._fake.n == km._fed.n == 0
    with pytest.raises(ValueError, match="0 real and 0 fake images fed"):
        prdc.result()


def test_prdc_kernels_do_not_use_scratch_memory():
    from musicgan_amd import _build
    _build.build()
    usage = _build.resource_usage()
    for pat in (r"prdc_dot_k", r"prdc_finish_k", r"prdc_scan_k"):
        hits = {k: v for k, v in usage.items() if re.search(pat, k)}
        assert hits, f"no kernel matches {pat}"
        for name, u in hits.items():
            assert u.get("ScratchSize [bytes/lane]", 0) == 0, f"{name}: {u.get('ScratchSize [bytes/lane]')} B/lane of scratch memory"
            assert u.get("VGPRs", 0) > 0
    assert len([k for k in usage if re.search(r"prdc_dot_k", k)]) == 2      # the 16-byte and the element-wise loads

"""CPU: the float64 restatement of the nearest-neighbour search (tests/nn_ref.py, the yardstick of test_nn_gpu.py) against itself,
the host queries and argument checks of musicgan_amd.metrics / nn_ops, the `nn` value of the `evaluate` sub-command's `--metrics`,
and the scratch use of the new kernels."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_ref as R  # noqa: E402


class Cuda:   # stands for a device tensor: the checks read these attributes only
    def __init__(self, t, contiguous=True):
        self.is_cuda, self.dtype, self._c, self.shape = True, t.dtype, contiguous, t.shape

    def is_contiguous(self):
        return self._c

    def dim(self):
        return len(self.shape)


def test_host_queries_need_no_gpu():
    from musicgan_amd import nn_ops
    c = nn_ops.nn_chunk()
    assert c >= 16 and c % 16 == 0 and c <= 4096
    assert nn_ops.nn_ws_bytes(256, 16, 32768) == (32768 // c) * 256 * 16 * 4
    assert nn_ops.nn_ws_bytes(5, 37, 3 * 7 * 11) == -(-231 // c) * 5 * 37 * 4      # a partial chunk counts as one
    assert nn_ops.nn_ws_bytes(0, 16, 64) == 0 and nn_ops.nn_ws_bytes(4, 4, 0) == 0
    assert nn_ops.MAX_K == 16 and nn_ops.EMPTY == torch.finfo(torch.float64).max


def test_gamma_follows_from_the_chunk_length():
    from musicgan_amd import nn_ops
    c = nn_ops.nn_chunk()
    g = R.gamma(2 * 512 * 512, c)
    assert c * 2.0 ** -24 < g < 1.001 * c * 2.0 ** -24 + 2 * 512 * 512 * 2.0 ** -52
    assert g < 1e-4    # small enough to mean something: 1e-4 of |q|^2 + |r|^2 + 2 sum |q r| is below the gap of a planted neighbour


@pytest.mark.parametrize("case", [(6, 20, (2, 16, 16), 2), (5, 37, (3, 7, 11), 3), (4, 12, (2, 128, 128), 1)])
def test_the_float64_expansion_equals_the_direct_form_within_the_bound(case):
    """nn_ref's own consistency, and that the bound is a bound for the float32 CPU evaluation of a chunk-free expansion too at
    these sizes only by way of 2 x its own error -- so only the float64 side is asserted here"""
    from musicgan_amd import nn_ops
    nq, nr, shape, seed = case
    q, r, planted = R.inputs(nq, nr, shape, seed)
    d, e, b = R.sqdist(q, r), R.expansion(q, r), R.bound(q, r, nn_ops.nn_chunk())
    assert d.dtype == torch.float64 and tuple(d.shape) == (nq, nr) and bool((d >= 0).all())
    assert bool(((d - e).abs() <= b).all()), float(((d - e).abs() / b).max())
    assert float(((d - e).abs() / b).max()) < 1e-6           # float64 against float64: far inside a float32 bound
    val, idx = R.ranking(d)
    for i, j, a in planted:
        assert int(idx[i, 0]) == j
        assert float(val[i, 1] - val[i, 0]) > 100 * float(b[i].max()), (i, j, a)    # the planted neighbour is unmistakable
        if a == 0:
            assert float(val[i, 0]) == 0.0


def test_ranking_orders_ties_by_id_and_bars_the_query_itself():
    d = torch.tensor([[1.0, 0.5, 0.5, 2.0], [0.0, 3.0, 1.0, 1.0]], dtype=torch.float64)
    val, idx = R.ranking(d, ids=[9, 7, 3, 1])
    assert idx.tolist() == [[3, 7, 9, 1], [9, 1, 3, 7]] and val[0].tolist() == [0.5, 0.5, 1.0, 2.0]
    val, idx = R.ranking(d, ids=[9, 7, 3, 1], query_ids=[3, 9])
    assert idx[0, :3].tolist() == [7, 9, 1] and idx[1, :3].tolist() == [1, 3, 7] and bool(torch.isinf(val[:, 3]).all())


def test_argument_errors_are_value_errors_before_any_gpu_work():
    from musicgan_amd import metrics
    z = torch.zeros
    for k in (0, 17, -1, 1.5):
        with pytest.raises(ValueError):
            metrics.NearestNeighbours(z(4, 2, 8, 8), k=k)
    with pytest.raises(ValueError):
        metrics.NearestNeighbours(z(0, 2, 8, 8))                       # Q = 0
    with pytest.raises(ValueError):
        metrics.NearestNeighbours(z(4))                                # no image axes
    with pytest.raises(ValueError):
        metrics.NearestNeighbours(z(4, 0))                             # D = 0
    with pytest.raises(ValueError):
        metrics.pairwise_sqdist(z(2, 2, 8, 8), z(3, 2, 8, 4))          # unequal trailing shapes
    with pytest.raises(ValueError):
        metrics.pairwise_sqdist(z(0, 8), z(3, 8))
    with pytest.raises(ValueError):
        metrics.pairwise_sqdist(z(3, 8), z(0, 8))


def test_cpu_tensors_wrong_types_and_strides_are_refused_loudly():
    from musicgan_amd import _lib, metrics, nn_ops, ops
    z = torch.zeros
    f64, i64 = dict(dtype=torch.float64), dict(dtype=torch.int64)
    with pytest.raises(_lib.MusicGanHipError):
        metrics.NearestNeighbours(z(4, 2, 8, 8))
    with pytest.raises(_lib.MusicGanHipError):
        metrics.pairwise_sqdist(z(4, 2, 8, 8), z(3, 2, 8, 8))
    with pytest.raises(_lib.MusicGanHipError):
        nn_ops.nn_sqnorm(z(4, 8))
    with pytest.raises(_lib.MusicGanHipError):
        nn_ops.nn_sqdist(z(4, 8), z(3, 8), z(4, **f64), z(3, **f64))
    with pytest.raises(_lib.MusicGanHipError):
        nn_ops.nn_merge(z(4, 3, **f64), z(3, **i64), z(4, 1, **f64), z(4, 1, **i64))
    # the type and layout checks themselves, on the checker the wrappers share
    ops._chk_typed("x", Cuda(z(1)))
    with pytest.raises(_lib.MusicGanHipError):
        ops._chk_typed("x", Cuda(z(1, **f64)))
    with pytest.raises(_lib.MusicGanHipError):
        ops._chk_typed("x", Cuda(z(1), contiguous=False))
    with pytest.raises(_lib.MusicGanHipError):
        ops._chk_typed("x", Cuda(z(1)), dtype=torch.float64)
    with pytest.raises(_lib.MusicGanHipError):
        ops._chk_typed("x", Cuda(z(1, **f64)), dtype=torch.int64)
    # shapes are checked after the device, before any launch
    with pytest.raises(ValueError):
        nn_ops.nn_sqnorm(Cuda(z(4)))
    with pytest.raises(ValueError):
        nn_ops.nn_sqnorm(Cuda(z(0, 8)))
    with pytest.raises(ValueError):
        nn_ops.nn_sqdist(Cuda(z(4, 8)), Cuda(z(3, 9)), Cuda(z(4, **f64)), Cuda(z(3, **f64)))
    with pytest.raises(ValueError):
        nn_ops.nn_merge(Cuda(z(4, 3, **f64)), Cuda(z(3, **i64)), Cuda(z(4, 17, **f64)), Cuda(z(4, 17, **i64)))   # k = 17
    with pytest.raises(ValueError):
        nn_ops.nn_merge(Cuda(z(4, 3, **f64)), Cuda(z(3, **i64)), Cuda(z(4, 0, **f64)), Cuda(z(4, 0, **i64)))     # k = 0


class _Fed:
    """a NearestNeighbours whose constructor did not run: feed's own checks come before anything touches the device"""

    def __new__(cls, shape, k=1):
        from musicgan_amd import metrics
        nn = object.__new__(metrics.NearestNeighbours)
        nn.k, nn.shape, nn._fed = k, shape, 0
        return nn


def test_feed_and_result_refuse_bad_input_before_any_launch():
    from musicgan_amd import _lib
    z = torch.zeros
    nn = _Fed((2, 8, 8), k=2)
    with pytest.raises(ValueError):
        nn.result()                                                    # nothing fed
    with pytest.raises(ValueError):
        nn.feed(z(3, 2, 8, 4), [0, 1, 2])                              # another image shape
    with pytest.raises(ValueError):
        nn.feed(z(0, 2, 8, 8), [])                                     # B = 0
    with pytest.raises(ValueError):
        nn.feed(z(3, 2, 8, 8), [0, 1, 1])                              # a repeated id within one feed
    with pytest.raises(ValueError):
        nn.feed(z(3, 2, 8, 8), torch.tensor([5, 4, 5]))
    with pytest.raises(ValueError):
        nn.feed(z(3, 2, 8, 8), [0, 1])                                 # one id per image
    with pytest.raises(ValueError):
        nn.feed(z(3, 2, 8, 8), [0, 1, -1])                             # -1 stands for "no id"
    with pytest.raises(ValueError):
        nn.feed(z(3, 2, 8, 8), [0.5, 1, 2])
    with pytest.raises(_lib.MusicGanHipError):
        nn.feed(z(3, 2, 8, 8), [0, 1, 2])                              # all in order, but not on a GPU
    nn._fed = 1
    with pytest.raises(ValueError):
        nn.result()                                                    # fewer references than k


def test_ops_gains_no_public_name():
    """the wrappers live in nn_ops: musicgan_amd.ops names nothing of the nearest-neighbour search"""
    from musicgan_amd import nn_ops, ops
    assert not [n for n in vars(ops) if "nn_" in n.lower()]
    assert {"nn_chunk", "nn_ws_bytes", "nn_sqnorm", "nn_sqdist", "nn_merge"} <= set(vars(nn_ops))


def test_every_wrapper_names_what_it_writes():
    from musicgan_amd import nn_ops
    assert "all of out" in nn_ops.nn_sqnorm.__doc__ and "all of out" in nn_ops.nn_sqdist.__doc__
    assert "best_d" in nn_ops.nn_merge.__doc__ and "best_i" in nn_ops.nn_merge.__doc__ and "rewritten whole" in nn_ops.nn_merge.__doc__


def test_metrics_option_of_the_evaluate_parser_accepts_nn():
    from musicgan_amd.__main__ import _MODES, build_parser
    p = build_parser()
    _, _, _, pos, kw = _MODES["evaluate"]
    today = ["evaluate", "g.pt", "8", "-i", "d", "--level", "2", "-n", "8", "--batch-size", "4", "--seed", "3", "-o", "e.json"]
    assert kw(p.parse_args(today)) == dict(level=2, nb_images=8, batch_size=4, seed=3, output="e.json")     # as without the option
    assert kw(p.parse_args(today + ["--metrics", "nn"]))["metrics"] == ("nn",)
    a = p.parse_args(today + ["--metrics", "swd,msssim,nn"])
    assert pos(a) == ("g.pt", 8, "d") and kw(a)["metrics"] == ("swd", "msssim", "nn")
    for bad in ("fid", "nn,fid", "", "swd,swd", "nn,nn"):
        with pytest.raises(SystemExit):
            p.parse_args(today + ["--metrics", bad])


def test_evaluate_knows_the_metric_and_refuses_repeats_before_any_work():
    import musicgan_amd
    assert callable(musicgan_amd.evaluate)
    mod = sys.modules["musicgan_amd.evaluate"]
    assert mod.METRICS == ("swd", "msssim", "nn")
    assert (mod._NN_QUERIES, mod._NN_SIDE, mod._NN_K) == (256, 128, 1)
    for bad in (("nn", "nn"), ("nn", "fid"), ()):
        with pytest.raises(ValueError):
            musicgan_amd.evaluate("missing.pt", 8, "missing", bad)


def test_nn_kernels_do_not_use_scratch_memory():
    from musicgan_amd import _build
    _build.build()
    usage = _build.resource_usage()
    for pat in (r"nn_sqnorm_k", r"nn_dot_k", r"nn_dist_k", r"nn_merge_k"):
        hits = {k: v for k, v in usage.items() if re.search(pat, k)}
        assert hits, f"no kernel matches {pat}"
        for name, u in hits.items():
            assert u.get("ScratchSize [bytes/lane]", 0) == 0, f"{name}: {u.get('ScratchSize [bytes/lane]')} B/lane of scratch memory"
            assert u.get("VGPRs", 0) > 0
    assert len([k for k in usage if re.search(r"nn_dot_k", k)]) == 2      # the 16-byte and the element-wise loads

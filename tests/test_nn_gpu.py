"""GPU: the nearest-neighbour kernels (csrc/nn.hip) and musicgan_amd.metrics.NearestNeighbours / pairwise_sqdist / evaluate against
the float64 definition in tests/nn_ref.py.  Every bound is derived there (the rounding analysis of a float32 chain of the chunk's
length, or twice the float32 CPU evaluation's own error), none is fitted to what the kernels give.

Ranking: every computed distance of a query lies within e = max_j bound(q, j) of its float64 value, and sorting two lists whose
entries differ by at most e gives lists whose entries differ by at most e rank by rank.  So the computed distance at rank i is
within e of the i-th smallest float64 distance, and the float64 distance of the reference returned there within 2 e of it; where
the float64 gaps to both adjacent ranks exceed 2 e the reference itself is determined."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_ref as R  # noqa: E402
from eval_corpus import tiny_corpus  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(32, 256, (2, 128, 128), 4), (8, 48, (2, 512, 512), 2), (64, 512, (2, 16, 16), 16), (5, 37, (3, 7, 11), 3)]
IDS = ["x".join(map(str, (q, m) + s + (k,))) for q, m, s, k in CASES]
# the tensor arguments the wrappers of musicgan_amd/nn_ops.py write, each all of it (their docstrings)
INPLACE = {
    "nn_sqnorm": ("out",),                 # "all of out (n,)"
    "nn_sqdist": ("out",),                 # "all of out (nq, nr)"
    "nn_merge": ("best_d", "best_i"),      # "both rewritten whole"
}


def _chunk():
    from musicgan_amd import nn_ops
    return nn_ops.nn_chunk()


def _fed(q, r, ids, k, splits, query_ids=None, order=None):
    """a NearestNeighbours over q fed r in consecutive batches of the sizes `splits`, in the given order of the batches"""
    from musicgan_amd import metrics
    nn = metrics.NearestNeighbours(q, k=k, query_ids=query_ids)
    cuts, lo = [], 0
    for n in splits:
        cuts.append((lo, lo + n))
        lo += n
    assert lo == r.shape[0]
    for b in (order if order is not None else range(len(cuts))):
        lo, hi = cuts[b]
        nn.feed(r[lo:hi].contiguous(), ids[lo:hi])
    return nn.result()


def _parity(case, seed=70):
    nq, nr, shape, k = case
    from musicgan_amd import metrics
    q, r, planted = R.inputs(nq, nr, shape, seed + nq)
    d64, d32, b = R.sqdist(q, r), R.expansion(q, r, torch.float32), R.bound(q, r, _chunk())
    own = (d32 - d64).abs()
    # ---- the distance matrix
    got = metrics.pairwise_sqdist(q.to(DEV), r.to(DEV))
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (nq, nr)
    got = got.cpu()
    tol = torch.maximum(b, 2 * own)
    err = (got - d64).abs()
    assert bool((got >= 0).all())
    # ---- the neighbours
    ids = [3 * j + 1 for j in range(nr)]                                     # ids are names, not positions
    dist, idx = _fed(q.to(DEV), r.to(DEV), ids, k, [nr])
    assert dist.dtype == torch.float64 and idx.dtype == torch.int64 and dist.is_cuda and idx.is_cuda
    assert tuple(dist.shape) == (nq, k) and tuple(idx.shape) == (nq, k)
    dist, idx = dist.cpu(), idx.cpu()
    val, want = R.ranking(d64, ids)
    col = (idx - 1) // 3
    assert bool(((idx - 1) % 3 == 0).all()) and bool(((col >= 0) & (col < nr)).all())
    true_of_got = d64.gather(1, col)                                         # float64 distance of what was returned
    e = b.max(1, keepdim=True).values                                        # (nq, 1)
    rank_err = (true_of_got - val[:, :k]).abs()
    dist_err = (dist - true_of_got).abs()
    dist_tol = tol.gather(1, col)
    gap = torch.full((nq, k), float("inf"), dtype=torch.float64)
    gap[:, 1:] = val[:, 1:k] - val[:, :k - 1]
    gap = torch.minimum(gap, val[:, 1:k + 1] - val[:, :k])                   # to both adjacent ranks (nr > k everywhere)
    sure = gap > 2 * e
    print(f"nn {case}: d {float(d64.min()):.4g} .. {float(d64.max()):.4g}, bound {float(b.min()):.3e} .. {float(b.max()):.3e}; "
          f"matrix err {float(err.max()):.3e} (fp32 CPU {float(own.max()):.3e}), worst err / bound {float((err / tol).max()):.4f}; "
          f"returned distance worst err / bound {float((dist_err / dist_tol).max()):.4f}; rank err / (2 e) "
          f"{float((rank_err / (2 * e)).max()):.4f}; identity asserted at {int(sure.sum())} of {nq * k} places")
    assert bool((err <= tol).all()), float((err / tol).max())
    assert bool((dist_err <= dist_tol).all()), float((dist_err / dist_tol).max())
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())                         # ascending
    assert bool((rank_err <= 2 * e).all()), float((rank_err / (2 * e)).max())
    assert torch.equal(idx[sure], want[:, :k][sure])
    for i, j, a in planted:
        assert float(val[i, 1] - val[i, 0]) > 100 * float(e[i]) and bool(sure[i, 0]), (i, j, a)   # on the float64 side
        assert int(idx[i, 0]) == ids[j], (i, j, a)
        if a == 0:
            assert 0.0 <= float(dist[i, 0]) <= float(b[i, j])                # d(x, x): clamped, never negative
    return dist, idx


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_distances_and_neighbours_match_the_float64_definition(case):
    _parity(case)


@pytest.mark.parametrize("case", [(32, 64, (2, 32, 32), 4), (5, 37, (3, 7, 11), 3), (16, 30, (2, 128, 128), 16)],
                         ids=["32x64x2048", "odd", "k16"])
def test_any_split_and_any_order_of_the_batches_give_the_same_bits(case):
    from musicgan_amd import metrics
    nq, nr, shape, k = case
    q, r, _ = R.inputs(nq, nr, shape, 71)
    q, r = q.to(DEV), r.to(DEV)
    ids = list(range(100, 100 + nr))
    dist, idx = _fed(q, r, ids, k, [nr])
    threes = [3] * (nr // 3) + ([nr % 3] if nr % 3 else [])
    gen = torch.Generator().manual_seed(72)
    runs = [([1, nr - 1], None), (threes, None), ([1, nr - 1], [1, 0]), (threes, list(reversed(range(len(threes))))),
            (threes, torch.randperm(len(threes), generator=gen).tolist())]
    for splits, order in runs:
        d2, i2 = _fed(q, r, ids, k, splits, order=order)
        assert torch.equal(d2, dist) and torch.equal(i2, idx), (splits, order)
    # the matrix: a pair's value depends on its two rows alone -- not on the batch, its position in it, or the other operand's size
    full = metrics.pairwise_sqdist(q, r)
    assert torch.equal(metrics.pairwise_sqdist(q, r[5:6].contiguous()), full[:, 5:6])
    assert torch.equal(metrics.pairwise_sqdist(q[1:3].contiguous(), r[3:].contiguous()), full[1:3, 3:])
    assert torch.equal(metrics.pairwise_sqdist(r.flip(0).contiguous(), q).T.flip(1), full)    # and q.r = r.q, bit for bit
    assert torch.equal(dist[:, 0], full.min(1).values)


def test_a_long_reference_batch_goes_through_in_pieces_with_the_same_bits(monkeypatch):
    from musicgan_amd import metrics
    q, r, _ = R.inputs(6, 70, (2, 16, 16), 73)
    q, r = q.to(DEV), r.to(DEV)
    full = metrics.pairwise_sqdist(q, r)
    monkeypatch.setattr(metrics, "_NN_WS_BYTES", 1)         # pieces of 16 rows
    assert torch.equal(metrics.pairwise_sqdist(q, r), full)


def test_ties_go_to_the_smaller_id_whichever_is_fed_first():
    q, r, _ = R.inputs(4, 10, (2, 16, 16), 74)
    r[7] = r[2]
    q[0] = r[2]                                             # two references at distance 0 from query 0
    q, r = q.to(DEV), r.to(DEV)
    ids = [50, 51, 99, 53, 54, 55, 56, 11, 58, 59]          # the twins are 99 (fed first in order) and 11
    for splits, order in (([10], None), ([5, 5], None), ([5, 5], [1, 0]), ([1] * 10, list(reversed(range(10))))):
        dist, idx = _fed(q, r, ids, 2, splits, order=order)
        assert idx[0].tolist() == [11, 99] and float(dist[0, 0]) == float(dist[0, 1]), (splits, order, idx[0], dist[0])
        d1, i1 = _fed(q, r, ids, 1, splits, order=order)
        assert int(i1[0, 0]) == 11 and torch.equal(d1[:, 0], dist[:, 0])
        for row in range(1, 4):                             # every query sees the twins at one distance
            twins = [int(i) for i in idx[row] if int(i) in (11, 99)]
            assert twins in ([], [11, 99]) or (twins == [11] and int(idx[row, 1]) == 11), idx[row]


def test_leave_one_out():
    q, r, _ = R.inputs(2, 40, (2, 32, 32), 75)
    r = r.to(DEV)
    ids = list(range(200, 240))
    queries, own = r[:12].contiguous(), ids[:12]
    b = R.bound(queries.cpu(), queries.cpu(), _chunk()).diagonal()
    dist, idx = _fed(queries, r, ids, 3, [7, 33], query_ids=own)
    assert not bool((idx.cpu() == torch.tensor(own)[:, None]).any())
    d64 = R.sqdist(queries.cpu(), r.cpu())
    val, want = R.ranking(d64, ids, own)
    e = R.bound(queries.cpu(), r.cpu(), _chunk()).max(1, keepdim=True).values
    gap = torch.minimum(val[:, 1:4] - val[:, :3], torch.cat([torch.full((12, 1), float("inf"), dtype=torch.float64),
                                                             val[:, 1:3] - val[:, :2]], 1))
    sure = gap > 2 * e                                      # unrelated uniform images: most gaps are far above the bound, not all
    assert int(sure.sum()) >= 24, int(sure.sum())
    assert torch.equal(idx.cpu()[sure], want[:, :3][sure])
    col = idx.cpu() - 200
    assert bool(((d64.gather(1, col) - val[:, :3]).abs() <= 2 * e).all())
    # -1 stands for "no id": such a query is not barred from anything
    mixed = [o if i % 2 else -1 for i, o in enumerate(own)]
    dist_m, idx_m = _fed(queries, r, ids, 3, [40], query_ids=mixed)
    dist_0, idx_0 = _fed(queries, r, ids, 3, [40])
    assert torch.equal(idx_m[1::2], idx[1::2]) and torch.equal(idx_m[0::2], idx_0[0::2])
    # without ids a query finds itself, at a distance within the bound of 0 and never negative
    assert idx_0[:, 0].tolist() == own
    assert bool((dist_0[:, 0].cpu() >= 0).all()) and bool((dist_0[:, 0].cpu() <= b).all()), (dist_0[:, 0], b)
    assert torch.equal(idx_0[:, 1:3], idx[:, :2])


def test_too_few_usable_references_is_an_error():
    from musicgan_amd import metrics
    q, r, _ = R.inputs(2, 6, (2, 8, 8), 76)
    r = r.to(DEV)
    nn = metrics.NearestNeighbours(r[:2].contiguous(), k=3)
    with pytest.raises(ValueError):
        nn.result()
    nn.feed(r[:2].contiguous(), [0, 1])
    with pytest.raises(ValueError):
        nn.result()                                         # 2 references, k = 3
    nn.feed(r[2:3].contiguous(), [2])
    assert nn.result()[1].shape == (2, 3)
    loo = metrics.NearestNeighbours(r[:2].contiguous(), k=3, query_ids=[0, 1])
    loo.feed(r[:3].contiguous(), [0, 1, 2])
    with pytest.raises(ValueError):
        loo.result()                                        # 3 references, one of them the query itself
    loo.feed(r[3:4].contiguous(), [3])
    assert sorted(loo.result()[1][0].tolist()) == [1, 2, 3]
    with pytest.raises(ValueError):
        loo.feed(r[4:6].contiguous(), [4, 4])
    with pytest.raises(ValueError):
        loo.feed(r[4:6, :, :4].contiguous(), [4, 5])


def test_feeding_does_not_synchronise():
    from musicgan_amd import metrics
    q, r, _ = R.inputs(8, 24, (2, 32, 32), 77)
    q, r = q.to(DEV), r.to(DEV)
    nn = metrics.NearestNeighbours(q, k=2)
    ids = [torch.arange(lo, lo + 8) for lo in (0, 8, 16)]   # on the host: the copy to the device is asynchronous for the caller
    nn.feed(r[:8], ids[0])                                  # warm-up: library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in (1, 2):
            nn.feed(r[8 * i:8 * i + 8], ids[i])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    dist, idx = nn.result()
    d2, i2 = _fed(q, r, list(range(24)), 2, [24])
    assert torch.equal(dist, d2) and torch.equal(idx, i2)


@pytest.mark.parametrize("case", [(5, 37, (3, 7, 11), 3), (32, 64, (2, 32, 32), 16)], ids=["odd", "k16"])
def test_parity_body_on_poisoned_memory(case):
    """the parity body and split feeds under poison.rule pointed at nn_ops: no guard band damaged by any launch, no argument changed
    that the table does not name, equal digests under both fills (nothing read that nobody wrote), nothing non-finite"""
    from musicgan_amd import nn_ops

    def run(p):
        p.best = _parity(case)
        nq, nr, shape, k = case
        q, r, _ = R.inputs(nq, nr, shape, 78)
        p.split = _fed(q.to(DEV), r.to(DEV), list(range(nr)), k, [1, nr - 1], query_ids=list(range(nq)))
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=nn_ops, inplace=INPLACE)
    for a, b in zip(r0.best + r0.split, r1.best + r1.split):
        assert torch.equal(a, b)
    names = {name for name, _, _ in r1.calls}
    assert {"nn_sqnorm", "nn_sqdist", "nn_merge"} <= names, names
    assert all(outs for name, _, outs in r1.calls if name in INPLACE)
    print(f"POISON nn {case}: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")


def test_evaluate_with_nn_on_a_tiny_corpus(tmp_path, capsys, monkeypatch):
    import musicgan_amd
    from musicgan_amd import audio, ops
    from musicgan_amd.__main__ import main
    from musicgan_amd.networks import Generator
    data_dir, ck = tiny_corpus(tmp_path, files=2, seed=5, level=2)      # 2 files x 2 samples
    capsys.readouterr()
    kw = dict(level=2, nb_images=8, batch_size=3, seed=1)
    before = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("swd", "msssim"), **kw)
    text = capsys.readouterr().out
    assert list(before) == ["16", "avg", "msssim_real", "msssim_fake"] and "NN RMS" not in text     # without nn: as it was
    new = ["nn_fake", "nn_real", "nn_fake_min", "nn_real_min"]
    full = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("swd", "msssim", "nn"), **kw)
    text = capsys.readouterr().out
    assert list(full) == list(before) + new
    assert all(full[k] == before[k] for k in before)
    assert all(isinstance(full[k], float) and full[k] >= 0.0 and full[k] == full[k] and full[k] != float("inf") for k in new), full
    assert full["nn_fake_min"] <= full["nn_fake"] and full["nn_real_min"] <= full["nn_real"]
    assert "NN RMS [fake]" in text and "NN RMS [real]" in text and "memorised" in text
    js = str(tmp_path / "eval.json")
    main(["evaluate", ck, "8", "-i", str(data_dir), "--level", "2", "-n", "8", "--batch-size", "3", "--seed", "1",
          "--metrics", "swd,msssim,nn", "-o", js])
    with open(js) as f:
        assert json.load(f) == full                                            # the identical result through the CLI
    assert list(json.load(open(js))) == list(full)
    for bs in (1, 16):                                                          # ... and at any batch size
        assert musicgan_amd.evaluate(ck, 8, str(data_dir), ("swd", "msssim", "nn"), **dict(kw, batch_size=bs)) == full, bs
    only = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("nn",), **kw)
    assert only == {k: full[k] for k in new} and list(only) == new
    with pytest.raises(ValueError):
        musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("nn",), level=2, nb_images=1)
    # the values against the float64 definition: the 4 dataset images at 16 x 16, the generator's 4 samples
    dataset = audio.PackedAudioDataset(str(data_dir)) if audio.has_packed(str(data_dir)) else audio.AudioDataset(str(data_dir))
    assert len(dataset) == 4
    real = ops.input_transform(torch.stack([dataset[i] for i in range(4)]).to(DEV).contiguous(), 16).cpu()
    d_rr = R.sqdist(real, real)
    d_rr.fill_diagonal_(float("inf"))
    comps = real[0].numel()
    rms_bound = float((R.bound(real, real, _chunk()).max() / comps).sqrt())     # |sqrt(a) - sqrt(b)| <= sqrt(|a - b|)
    want_real = (d_rr.min(1).values / comps).sqrt()
    assert abs(full["nn_real"] - float(want_real.mean())) <= rms_bound and abs(full["nn_real_min"] - float(want_real.min())) <= rms_bound
    # a "generator" that replays the dataset: SWD and MS-SSIM cannot tell, the nearest neighbours can
    state = {"next": 0}

    def replay(self, z, alpha):
        n = z.shape[0]
        out = torch.stack([real[(state["next"] + i) % 4] for i in range(n)]).to(z.device)
        state["next"] += n
        return out

    monkeypatch.setattr(Generator, "forward", replay)
    copied = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("nn",), **kw)
    print(f"evaluate nn: honest {only}, replaying {copied}, RMS bound {rms_bound:.3e}")
    assert 0.0 <= copied["nn_fake_min"] <= rms_bound and 0.0 <= copied["nn_fake"] <= rms_bound
    assert copied["nn_fake"] < copied["nn_real"]
    assert copied["nn_real"] == full["nn_real"] and copied["nn_real_min"] == full["nn_real_min"]

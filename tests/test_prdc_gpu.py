"""GPU: the tiled distance kernel and the ball-membership scan (csrc/prdc.hip), musicgan_amd.metrics.PRDC and the `prdc` metric of
evaluate.  The tiled kernel has an exact oracle: nn_ops.nn_sqdist on the same rows, bit for bit.  PRDC is held against the float64
definition in tests/prdc_ref.py: every count between the surely-inside and the not-surely-outside count, every number inside the
interval those give (narrow by the reference alone: test_prdc_cpu.py), and exactly equal wherever the interval is a point."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_ref as R  # noqa: E402
from eval_corpus import tiny_corpus  # noqa: E402
import poison  # noqa: E402
import prdc_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the tensor arguments the new wrappers of musicgan_amd/nn_ops.py write (their docstrings), next to those of test_nn_gpu.py
INPLACE = {
    "nn_sqnorm": ("out",),
    "nn_sqdist": ("out",),
    "nn_merge": ("best_d", "best_i"),
    "nn_sqdist_tiled": ("out",),               # "all of out (nq, nr)"
    "prdc_scan": ("count", "rowmin"),          # "both accumulated in place"
}
# (nq, nr, D): one element; scalar loads; whole tiles; ragged tiles and a D tail; 18 chunks, so two slices hold two; 40 chunks;
# 128 chunks with more than one workgroup along the queries
SHAPES = [(1, 1, 1), (5, 37, 231), (64, 64, 2048), (70, 130, 2052), (33, 17, 256 * 17 + 8), (16, 16, 256 * 40), (130, 70, 32768)]


def _chunk():
    from musicgan_amd import nn_ops
    return nn_ops.nn_chunk()


def _rand(n, d, seed):
    return (torch.rand(n, d, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


def _both(q, r):
    from musicgan_amd import nn_ops
    qn, rn = nn_ops.nn_sqnorm(q), nn_ops.nn_sqnorm(r)
    return nn_ops.nn_sqdist_tiled(q, r, qn, rn), nn_ops.nn_sqdist(q, r, qn, rn)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_tiled_distances_are_bit_for_bit_those_of_nn_sqdist(shape):
    nq, nr, d = shape
    q, r = _rand(nq, d, 80 + nq), _rand(nr, d, 81 + nr)
    tiled, plain = _both(q, r)
    assert tiled.dtype == torch.float64 and tuple(tiled.shape) == (nq, nr)
    assert torch.equal(tiled, plain), int((tiled != plain).sum())
    assert bool((tiled >= 0).all())


def test_tiled_distances_of_misaligned_rows_and_of_identical_rows():
    """an operand that starts one float into its storage (rows at 4 bytes past a 16-byte boundary, D a multiple of 4), and a set
    against itself: the diagonal is clamped, never negative, and the same bits as nn_sqdist"""
    nq, nr, d = 21, 35, 520
    base = _rand(nq * d + 1, 1, 82).reshape(-1)
    q, r = base[1:].view(nq, d), _rand(nr, d, 83)
    assert q.data_ptr() % 16 == 4 and q.is_contiguous()
    tiled, plain = _both(q, r)
    assert torch.equal(tiled, plain)
    tiled, plain = _both(r, q)
    assert torch.equal(tiled, plain)
    tiled, plain = _both(r, r)
    assert torch.equal(tiled, plain) and bool((tiled.diagonal() >= 0).all())


def test_tiled_distances_match_the_float64_definition_within_the_bound():
    nq, nr, d = 70, 130, 2052
    q, r = _rand(nq, d, 80 + nq), _rand(nr, d, 81 + nr)
    tiled, _ = _both(q, r)
    d64, b = R.sqdist(q.cpu(), r.cpu()), R.bound(q.cpu(), r.cpu(), _chunk())
    err = (tiled.cpu() - d64).abs()
    print(f"tiled {nq} x {nr} x {d}: worst err / bound {float((err / b).max()):.4f}")
    assert bool((err <= b).all()), float((err / b).max())


@pytest.mark.parametrize("shape", [(3, 5), (7, 130), (66, 257), (130, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_scan_counts_and_minima_exactly_whole_and_in_column_blocks(shape):
    from musicgan_amd import nn_ops
    nq, nr = shape
    gen = torch.Generator().manual_seed(84 + nq)
    dist = torch.rand(nq, nr, generator=gen, dtype=torch.float64).to(DEV)
    radius = torch.rand(nr, generator=gen, dtype=torch.float64).to(DEV)
    dist[0, nr // 2] = radius[nr // 2]                          # equality counts as inside
    dist[nq - 1] = radius + 0.5                                 # a row inside no ball
    want_c, want_m = (dist <= radius).sum(1), dist.min(1).values
    assert int(want_c[nq - 1]) == 0 and int(want_c[0]) >= 1
    for step in (nr, 1, 7, 64):
        count = torch.zeros(nq, dtype=torch.int64, device=DEV)
        rowmin = torch.full((nq,), float("inf"), dtype=torch.float64, device=DEV)
        for lo in range(0, nr, step):
            nn_ops.prdc_scan(dist[:, lo:lo + step].contiguous(), radius[lo:lo + step].contiguous(), count, rowmin)
        assert torch.equal(count, want_c) and torch.equal(rowmin, want_m), step
    nn_ops.prdc_scan(dist, radius, count, rowmin)               # accumulated in place: a second pass doubles the counts
    assert torch.equal(count, 2 * want_c) and torch.equal(rowmin, want_m)


def _feed(prdc, real, fake, splits=None):
    """feed both sets in consecutive batches of `splits` images (None: one batch each), real and fake batches taking turns"""
    cut = lambda x: [x] if splits is None else [x[lo:lo + splits].contiguous() for lo in range(0, x.shape[0], splits)]
    reals, fakes = cut(real), cut(fake)
    for i in range(max(len(reals), len(fakes))):
        if i < len(fakes):
            prdc.feed_fake(fakes[i])
        if i < len(reals):
            prdc.feed_real(reals[i])
    return prdc


def _parity(index):
    from musicgan_amd import metrics
    real, fake, k, iv = P.case(index, _chunk())
    prdc = _feed(metrics.PRDC(k=k), real.to(DEV), fake.to(DEV))
    got, per = prdc.result(), prdc.per_sample()
    assert list(got) == list(P.KEYS) and all(isinstance(v, float) for v in got.values())
    assert set(per) == {"radius_real", "radius_fake", "count_fake", "count_real", "nearest_fake"}
    for name, t in per.items():
        assert t.is_cuda and t.dtype == (torch.int64 if name.startswith("count") else torch.float64), name
    cpu = {name: t.cpu() for name, t in per.items()}
    ref = iv["per"]
    print(f"prdc {P.IDS[index]}: got {got}, lo {iv['lo']}, hi {iv['hi']}; radius err / bound "
          f"{float(((cpu['radius_real'] - ref['radius_real']).abs() / iv['rb_real']).max()):.4f}, "
          f"{float(((cpu['radius_fake'] - ref['radius_fake']).abs() / iv['rb_fake']).max()):.4f}; nearest err / bound "
          f"{float(((cpu['nearest_fake'] - ref['nearest_fake']).abs() / iv['nb']).max()):.4f}")
    assert bool(((cpu["radius_real"] - ref["radius_real"]).abs() <= iv["rb_real"]).all())
    assert bool(((cpu["radius_fake"] - ref["radius_fake"]).abs() <= iv["rb_fake"]).all())
    assert bool(((cpu["nearest_fake"] - ref["nearest_fake"]).abs() <= iv["nb"]).all())
    for name in ("count_fake", "count_real"):
        lo, hi = iv[name + "_lo"], iv[name + "_hi"]
        assert bool((lo <= cpu[name]).all()) and bool((cpu[name] <= hi).all()), name
        point = lo == hi
        assert torch.equal(cpu[name][point], ref[name][point]), name          # a decided sample agrees exactly
    covered = cpu["nearest_fake"] <= cpu["radius_real"]
    point = iv["covered_lo"] == iv["covered_hi"]
    assert torch.equal(covered[point], iv["covered_lo"][point])
    for name in P.KEYS:
        assert iv["lo"][name] <= got[name] <= iv["hi"][name], (name, got[name], iv["lo"][name], iv["hi"][name])
    assert got == P.numbers(cpu["count_fake"], cpu["count_real"], covered, k)  # the numbers are those of the per-sample tensors
    return [per[name] for name in sorted(per)]


@pytest.mark.parametrize("index", range(len(P.CASES)), ids=P.IDS)
def test_prdc_lies_inside_the_intervals_of_the_float64_definition(index):
    _parity(index)


@pytest.mark.parametrize("index", [1, 0], ids=[P.IDS[1], P.IDS[0]])
def test_any_split_any_order_and_any_block_size_give_the_same_bits(index):
    from musicgan_amd import metrics
    real, fake, k, _ = P.case(index, _chunk())
    real, fake = real.to(DEV), fake.to(DEV)
    base = _feed(metrics.PRDC(k=k), real, fake)
    want, want_n = base.per_sample(), base.result()
    runs = [(1, 256 << 20), (3, 256 << 20), (None, 1), (3, 40000)]
    for splits, block_bytes in runs:
        other = _feed(metrics.PRDC(k=k, block_bytes=block_bytes), real, fake, splits)
        got = other.per_sample()
        for name in want:
            assert torch.equal(got[name], want[name]), (name, splits, block_bytes)
        assert other.result() == want_n
    swapped = metrics.PRDC(k=k)                                  # all fakes first, then the reals, in two pieces
    swapped.feed_fake(fake)
    swapped.feed_real(real[:5].contiguous())
    swapped.feed_real(real[5:].contiguous())
    got = swapped.per_sample()
    assert all(torch.equal(got[name], want[name]) for name in want)
    with pytest.raises(ValueError):
        swapped.feed_real(real[:2, :, :4].contiguous())          # another trailing shape
    few = metrics.PRDC(k=k)
    few.feed_real(real)
    few.feed_fake(fake[:k].contiguous())
    with pytest.raises(ValueError):
        few.result()                                             # k fakes: no k-th nearest OTHER fake
    few.feed_fake(fake[k:k + 1].contiguous())
    assert set(few.result()) == set(P.KEYS)


def test_feeding_does_not_synchronise():
    from musicgan_amd import metrics
    real, fake, k, _ = P.case(1, _chunk())
    real, fake = real.to(DEV), fake.to(DEV)
    prdc = metrics.PRDC(k=k)
    prdc.feed_real(real[:8])                                     # warm-up: library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        prdc.feed_fake(fake[:20])
        prdc.feed_real(real[8:])
        prdc.feed_fake(fake[20:])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert prdc.result() == _feed(metrics.PRDC(k=k), real, fake).result()


@pytest.mark.parametrize("index", [1, 3], ids=["odd", "k16"])
def test_parity_body_on_poisoned_memory(index):
    """the parity body and a split, small-block run under poison.rule pointed at nn_ops: no guard band damaged by any launch, no
    argument changed that the table does not name, equal digests under both fills (nothing read that nobody wrote: every slice of
    the workspace is written, the empty ones with zeros), nothing non-finite"""
    from musicgan_amd import metrics, nn_ops

    def run(p):
        p.best = _parity(index)
        real, fake, k, _ = P.case(index, _chunk())
        other = _feed(metrics.PRDC(k=k, block_bytes=40000), real.to(DEV), fake.to(DEV), 3).per_sample()
        p.split = [other[name] for name in sorted(other)]
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=nn_ops, inplace=INPLACE)
    for a, b in zip(r0.best + r0.split, r1.best + r1.split):
        assert torch.equal(a, b)
    for a, b in zip(r1.best, r1.split):
        assert torch.equal(a, b)
    names = {name for name, _, _ in r1.calls}
    assert {"nn_sqnorm", "nn_merge"} <= names, names
    assert all(outs for name, _, outs in r1.calls if name in INPLACE)
    assert {"nn_sqdist_tiled", "nn_tiled_ws_bytes", "prdc_scan"} <= names, names      # the three new wrappers were all exercised
    print(f"POISON prdc {P.IDS[index]}: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")


def test_evaluate_with_prdc_on_a_tiny_corpus(tmp_path, capsys, monkeypatch):
    import musicgan_amd
    from musicgan_amd import audio, ops
    from musicgan_amd.__main__ import main
    from musicgan_amd.networks import Generator
    data_dir, ck = tiny_corpus(tmp_path, files=4, seed=6, level=2)      # 4 files x 2 samples
    dataset = audio.PackedAudioDataset(str(data_dir)) if audio.has_packed(str(data_dir)) else audio.AudioDataset(str(data_dir))
    n = len(dataset)
    assert n == 8
    capsys.readouterr()
    kw = dict(level=2, nb_images=n, batch_size=3, seed=1)
    before = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("swd", "msssim", "nn"), **kw)
    text = capsys.readouterr().out
    assert list(before) == ["16", "avg", "msssim_real", "msssim_fake", "nn_fake", "nn_real", "nn_fake_min", "nn_real_min"]
    assert "PRDC" not in text                                                   # without prdc: as it was
    new = list(P.KEYS) + [name + "_real" for name in P.KEYS]
    full = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("swd", "msssim", "nn", "prdc"), **kw)
    text_full = capsys.readouterr().out
    assert list(full) == list(before) + new
    assert all(full[name] == before[name] for name in before)
    assert text_full.startswith(text) and text_full[len(text):].count("\n") == 9  # eight numbers and how to read them, appended
    for name in new:
        assert f"PRDC [{name:>14}]" in text_full, name
    assert "off the data manifold" in text_full and "modes missing" in text_full and "_real" in text_full
    for name in new:
        v = full[name]
        assert isinstance(v, float) and v >= 0.0 and (v <= 1.0 or name.startswith("density")), (name, v)
    js = str(tmp_path / "eval.json")
    main(["evaluate", ck, "8", "-i", str(data_dir), "--level", "2", "-n", str(n), "--batch-size", "3", "--seed", "1",
          "--metrics", "swd,msssim,nn,prdc", "-o", js])
    with open(js) as f:
        loaded = json.load(f)
    assert loaded == full and list(loaded) == list(full)                        # the identical result through the CLI
    only = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("prdc",), **kw)
    assert only == {name: full[name] for name in new} and list(only) == new
    for bs in (1, 16):                                                          # ... and at any batch size
        assert musicgan_amd.evaluate(ck, 8, str(data_dir), ("prdc",), **dict(kw, batch_size=bs)) == only, bs
    with pytest.raises(ValueError):
        musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("prdc",), level=2, nb_images=7)
    # a "generator" that replays the dataset: every fake is a real image, every real image has a fake at distance 0
    real = ops.input_transform(torch.stack([dataset[i] for i in range(n)]).to(DEV).contiguous(), 16).cpu()
    state = {"next": 0}

    def replay(self, z, alpha):
        out = torch.stack([real[(state["next"] + i) % n] for i in range(z.shape[0])]).to(z.device)
        state["next"] += z.shape[0]
        return out

    monkeypatch.setattr(Generator, "forward", replay)
    copied = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("prdc",), **kw)
    assert copied["precision"] == 1.0 and copied["coverage"] == 1.0 and copied["recall"] == 1.0
    assert all(copied[name + "_real"] == only[name + "_real"] for name in P.KEYS)
    # one that returns a single image.  Its fake balls have radius d(x, x), which only a real image equal to x is inside: recall
    # <= 1 / n.  Its one point is every real's nearest fake, and real j is covered iff x is within j's k-th nearest other real.
    # For x a dataset image that is j = x itself plus x's in-degree in the k-nearest-neighbour graph of the reals; the in-degrees
    # add up to n k, so the image with the fewest has at most k (the pigeonhole; an arbitrary x has no such bound): that image
    # is the one replayed, chosen by the float64 definition.
    k = sys.modules["musicgan_amd.evaluate"]._PRDC_K
    d_rr = R.sqdist(real, real)
    rad = P.radius(d_rr, k)
    indeg = (d_rr <= rad[:, None]).sum(0) - 1                                   # column x: the reals j != x with x in their ball
    x = int(indeg.argmin())
    assert int(indeg[x]) <= k
    monkeypatch.setattr(Generator, "forward",
                        lambda self, z, alpha: real[x:x + 1].expand(z.shape[0], -1, -1, -1).contiguous().to(z.device))
    stuck = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("prdc",), **kw)
    print(f"evaluate prdc: honest {only}, replaying {copied}, stuck on image {x} (in-degree {int(indeg[x])}) {stuck}")
    assert stuck["recall"] <= 1.0 / n and stuck["coverage"] <= (k + 1) / n

"""GPU: the k-means kernels (csrc/kmeans.hip) through musicgan_amd.km_ops, musicgan_amd.metrics.KMeans / NDB and the `ndb` metric of
evaluate.  The assignment has an exact oracle (torch's row minimum of the same device matrix) and is held against the float64
definition of tests/ndb_ref.py within the derived distance bounds; the ordering is a stable sort; the update is held against exact
float64 means within the derived bound; KMeans equals its own four steps bit for bit and finds planted blobs exactly."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ndb_ref as N  # noqa: E402
from eval_corpus import tiny_corpus  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the tensor arguments the wrappers of musicgan_amd/km_ops.py write (their docstrings)
INPLACE = {
    "km_assign": ("label", "mind", "changed"),   # "all of label and all of mind are written", "changed ... is overwritten"
    "km_order": ("start", "order"),              # "all of start ... and all of order"
    "km_update": ("centroid",),                  # "updated in place"
    "km_count": ("count",),                      # "accumulated in place"
}


def _chunk():
    from musicgan_amd import nn_ops
    return nn_ops.nn_chunk()


def _dist(x, c):
    from musicgan_amd import nn_ops
    return nn_ops.nn_sqdist_tiled(x, c, nn_ops.nn_sqnorm(x), nn_ops.nn_sqnorm(c))


def _row_min(dist):
    """torch's row minimum of a device matrix, ties resolved to the smaller column"""
    m = dist.min(1, keepdim=True).values
    return (dist == m).to(torch.int8).argmax(1).to(torch.int32), m[:, 0].contiguous()


def _fresh(n):
    return torch.full((n,), -1, dtype=torch.int32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ km_assign
def _assign_body(index):
    from musicgan_amd import km_ops
    g = N.general(index, _chunk())
    n = g["x"].shape[0]
    dist = _dist(g["x"].to(DEV), g["c"].to(DEV))
    label, mind, changed = km_ops.km_assign(dist, _fresh(n))
    want_l, want_m = _row_min(dist)
    assert label.dtype == torch.int32 and mind.dtype == torch.float64 and changed.dtype == torch.int64
    assert torch.equal(label, want_l) and torch.equal(mind, want_m)
    assert int(changed) == n                                             # fresh labels of -1: every row counts
    again = km_ops.km_assign(dist, label, mind)[2]
    assert int(again) == 0 and torch.equal(label, want_l)                 # overwritten, not accumulated
    got, ref = label.cpu().long(), g["labels"]
    differ = (got != ref).nonzero().reshape(-1).tolist()
    print(f"km_assign {N.GENERAL_IDS[index]}: {len(differ)} of {n} labels differ from the float64 choice")
    assert len(differ) <= N.UNDECIDED_CAP * n
    for i in differ:                                                     # ... and only where the bounds leave the choice open
        assert float(g["ratio"][i, got[i]]) <= 1.0, (i, int(got[i]), int(ref[i]))
    return [label, mind, changed, again]


@pytest.mark.parametrize("index", range(len(N.GENERAL)), ids=N.GENERAL_IDS)
def test_assign_is_the_row_minimum_bit_for_bit_and_the_float64_choice_within_the_bounds(index):
    _assign_body(index)


@pytest.mark.parametrize("shape", [(5, 1), (70, 2), (33, 64), (9, 65), (130, 1024)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_assign_resolves_ties_to_the_smaller_column(shape):
    """a matrix of the values 0, 1, 2 (most rows have several smallest entries), a row of one value and a row of infinities"""
    from musicgan_amd import km_ops
    n, k = shape
    dist = torch.randint(0, 3, (n, k), generator=torch.Generator().manual_seed(60 + n)).double().to(DEV)
    dist[n // 2] = 7.0
    dist[n - 1] = float("inf")
    label, mind, changed = km_ops.km_assign(dist, _fresh(n))
    want_l, want_m = _row_min(dist)
    assert torch.equal(label, want_l) and torch.equal(mind, want_m)
    assert int(label[n // 2]) == 0 and int(label[n - 1]) == 0 and int(changed) == n
    label[::2] = k - 1 if k > 1 else -1                                  # every second label is rewritten, unless it was right
    stale = int((label != want_l).sum())
    changed = km_ops.km_assign(dist, label, mind, changed)[2]
    assert int(changed) == stale and torch.equal(label, want_l)


# ------------------------------------------------------------------ km_order
def _order_body(n, k):
    from musicgan_amd import km_ops
    label = torch.randint(0, k, (n,), generator=torch.Generator().manual_seed(61 + n + k)).to(torch.int32)
    label[label == k // 2] = 0                                           # an empty bin in the middle
    label[label == k - 1] = 1                                            # ... and one at the end
    label = label.to(DEV)
    start, order = km_ops.km_order(label, k)
    sizes = torch.bincount(label.long(), minlength=k)
    assert int(sizes[k // 2]) == 0 and int(sizes[k - 1]) == 0
    want_start = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), sizes.cumsum(0)]).to(torch.int32)
    want_order = torch.sort(label.long(), stable=True).indices.to(torch.int32)
    assert start.dtype == torch.int32 and tuple(start.shape) == (k + 1,) and torch.equal(start, want_start)
    assert order.dtype == torch.int32 and tuple(order.shape) == (n,) and torch.equal(order, want_order)
    return [start, order]


@pytest.mark.parametrize("shape", [(37, 5), (300, 7), (5000, 7), (5000, 1024), (300, 1024)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_order_is_a_stable_sort_by_label_with_prefix_sums(shape):
    _order_body(*shape)


def test_order_refuses_more_points_than_one_launch_sorts():
    from musicgan_amd import km_ops
    with pytest.raises(ValueError):
        km_ops.km_order(torch.zeros((1 << 20) + 1, dtype=torch.int32, device=DEV), 4)
    start, order = km_ops.km_order(torch.zeros(1 << 20, dtype=torch.int32, device=DEV), 2)      # the largest n: one bin holds all
    assert start.tolist() == [0, 1 << 20, 1 << 20] and torch.equal(order, torch.arange(1 << 20, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------ km_update
def _pattern(k, d):
    """recognisable centroids: what an untouched row must still hold"""
    return (torch.arange(k * d, dtype=torch.float32).reshape(k, d) % 251.0 - 125.0) / 64.0


def _update(x, labels, k):
    """(the updated centroids on the host, the pattern they started from)"""
    from musicgan_amd import km_ops
    start, order = km_ops.km_order(labels.to(torch.int32).to(DEV), k)
    c0 = _pattern(k, x.shape[1])
    return km_ops.km_update(x.to(DEV) if not x.is_cuda else x, order, start, c0.to(DEV)).cpu(), c0


def _check_update(x, labels, k, what):
    got, c0 = _update(x, labels, k)
    mean, bnd, count = N.means(x, labels, c0)
    err = (got.double() - mean).abs()
    used = torch.tensor(count) > 0
    print(f"km_update {what}: sizes {count}, worst err / bound {float((err[used] / bnd[used]).max()):.4f}")
    assert bool((err <= bnd).all())
    assert torch.equal(_bits(got[~used]), _bits(c0[~used]))              # a bin without members keeps its bits
    return got


def _update_body(index):
    p = N.planted(index, _chunk())
    return _check_update(p["x"], p["truth"], p["k"], N.PLANTED_IDS[index])


@pytest.mark.parametrize("index", range(len(N.PLANTED)), ids=N.PLANTED_IDS)
def test_update_is_the_float64_mean_within_the_bound(index):
    _update_body(index)


def test_update_of_bins_longer_than_a_chunk_and_of_empty_bins():
    """labels % 2 at 300 x 1024: two bins of 171 and 129 members, several chunks each with a ragged last one; then spread over the
    bins 0 and 2 of 4, so that an empty bin lies between them and another at the end"""
    p = N.planted(1, _chunk())
    got = _check_update(p["x"], p["truth"] % 2, 2, "labels % 2")
    wide = _check_update(p["x"], (p["truth"] % 2) * 2, 4, "labels % 2 in the bins 0 and 2 of 4")
    assert torch.equal(_bits(got[0]), _bits(wide[0])) and torch.equal(_bits(got[1]), _bits(wide[2]))


def test_a_centroid_depends_on_its_member_list_alone():
    """the same members at the same positions, alone in 3 bins and among 6 more bins whose members are appended; and rows that
    start 4 bytes past a 16-byte boundary (element-wise loads) against an aligned copy"""
    from musicgan_amd import km_ops
    p = N.planted(1, _chunk())
    x = p["x"]
    few, _ = _update(x[:120].contiguous(), torch.arange(120) % 3, 3)
    labels = torch.cat([torch.arange(120) % 3, 3 + torch.arange(180) % 6])
    many, _ = _update(x, labels, 9)
    assert torch.equal(_bits(few), _bits(many[:3]))
    n, d = 21, 520
    base = torch.rand(n * d + 1, generator=torch.Generator().manual_seed(62)).to(DEV)
    shifted = base[1:].view(n, d)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    start, order = km_ops.km_order((torch.arange(n) % 2).to(torch.int32).to(DEV), 2)
    a = km_ops.km_update(shifted, order, start, torch.zeros(2, d, device=DEV))
    b = km_ops.km_update(shifted.clone(), order, start, torch.zeros(2, d, device=DEV))
    assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ km_count
def _count_body():
    from musicgan_amd import km_ops
    gen = torch.Generator().manual_seed(63)
    one, two = (torch.randint(0, 9, (n,), generator=gen).to(torch.int32) for n in (1000, 37))
    two[5] = -1                                                          # outside the bins: skipped
    two[6] = 9
    count = torch.zeros(9, dtype=torch.int64, device=DEV)
    km_ops.km_count(one.to(DEV), count)
    assert torch.equal(count.cpu(), torch.bincount(one.long(), minlength=9))
    km_ops.km_count(two.to(DEV), count)                                  # accumulated in place
    inside = two[(two >= 0) & (two < 9)]
    assert torch.equal(count.cpu(), torch.bincount(one.long(), minlength=9) + torch.bincount(inside.long(), minlength=9))
    return [count]


def test_count_accumulates_over_calls():
    _count_body()


# ------------------------------------------------------------------ KMeans
def _kmeans(x, k, splits=None, **kw):
    from musicgan_amd import metrics
    km = metrics.KMeans(bins=k, **kw)
    for lo in range(0, x.shape[0], splits or x.shape[0]):
        km.feed(x[lo:lo + (splits or x.shape[0])].contiguous())
    return km.fit()


def _outputs(km):
    return [km.centroids, km.labels, km.counts, km.changed]


def test_kmeans_moves_converges_and_then_leaves_every_bit():
    """500 points in 3 dimensions, where Lloyd's iterations do move labels (the float64 restatement changes 108, 65, 27, ... and
    none from the 15th on): labels change after the first assignment, `changed` reaches 0 within 40 iterations, and a run that
    stops at the first 0 has the bits of the run that goes on"""
    x = (torch.rand(500, 3, generator=torch.Generator().manual_seed(64)) * 2 - 1).to(DEV)
    long = _kmeans(x, 8, iterations=40, init_ids=list(range(8)))
    changed = long.changed.tolist()
    print(f"kmeans 500x3x8: changed {changed}")
    assert changed[0] == 500 and changed[1] > 0 and 0 in changed
    first = changed.index(0)
    assert changed[first:] == [0] * (41 - first)                         # once 0, always 0
    short = _kmeans(x, 8, iterations=first, init_ids=list(range(8)))
    assert short.changed.tolist() == changed[:first + 1]
    for a, b in zip(_outputs(short)[:3], _outputs(long)[:3]):
        assert torch.equal(a, b)
    assert int(long.counts.sum()) == 500 and torch.equal(long.counts, torch.bincount(long.labels.long(), minlength=8))


def test_kmeans_equals_its_own_steps_bit_for_bit():
    from musicgan_amd import km_ops, nn_ops
    g = N.general(1, _chunk())
    x, k, ids, iters = g["x"].to(DEV), g["k"], g["init_ids"], 3
    km = _kmeans(x, k, iterations=iters, init_ids=ids)
    c, xn, labels, changed = x[ids].clone(), nn_ops.nn_sqnorm(x), _fresh(x.shape[0]), []
    for t in range(iters + 1):
        _, mind, ch = km_ops.km_assign(nn_ops.nn_sqdist_tiled(x, c, xn, nn_ops.nn_sqnorm(c)), labels)
        changed.append(ch.clone())
        if t < iters:
            start, order = km_ops.km_order(labels, k)
            km_ops.km_update(x, order, start, c)
    counts = km_ops.km_count(labels, torch.zeros(k, dtype=torch.int64, device=DEV))
    assert torch.equal(_bits(km.centroids), _bits(c)) and torch.equal(km.labels, labels) and torch.equal(km.counts, counts)
    assert torch.equal(km.changed, torch.cat(changed)) and int(km.changed[0]) == x.shape[0]
    assert km.centroids.dtype == torch.float32 and km.labels.dtype == torch.int32 and km.counts.dtype == torch.int64
    assert tuple(km.changed.shape) == (iters + 1,) and km.changed.is_cuda and int(km.counts.sum()) == x.shape[0]
    again_l, again_d = km.assign(x)                                      # the fed images against the fitted centroids
    assert torch.equal(again_l, labels) and torch.equal(again_d, mind)
    print(f"kmeans general: changed {km.changed.tolist()}, sizes {km.counts.tolist()}")


@pytest.mark.parametrize("index", range(len(N.PLANTED)), ids=N.PLANTED_IDS)
def test_kmeans_finds_planted_blobs_exactly_and_stays_there(index):
    p = N.planted(index, _chunk())
    x, k, iters = p["x"].to(DEV), p["k"], p["iterations"]
    km = _kmeans(x, k, iterations=iters, init_ids=p["init_ids"])
    assert torch.equal(km.labels.cpu().long(), p["truth"]) and km.counts.tolist() == p["count"]
    assert km.changed.tolist() == [x.shape[0]] + [0] * iters
    err = (km.centroids.cpu().double() - p["mean"]).abs()
    print(f"kmeans planted {N.PLANTED_IDS[index]}: worst centroid err / bound {float((err / p['bound']).max()):.4f}")
    assert bool((err <= p["bound"]).all())
    longer = _kmeans(x, k, iterations=iters + 2, init_ids=p["init_ids"])  # converged: later iterations leave every bit
    assert torch.equal(_bits(longer.centroids), _bits(km.centroids)) and torch.equal(longer.labels, km.labels)
    assert longer.changed.tolist() == [x.shape[0]] + [0] * (iters + 2)


def _split_runs(x, k, **kw):
    """[outputs] of one feed with one block, then of splits and block sizes that must not show"""
    return [_outputs(_kmeans(x, k, splits, block_bytes=bb, **kw)) for splits, bb in ((None, 256 << 20), (1, 256 << 20), (3, 40000),
                                                                                     (None, 1))]


def test_any_feed_split_and_any_block_size_give_the_same_bits():
    g = N.general(0, _chunk())
    runs = _split_runs(g["x"].to(DEV), g["k"], iterations=3, init_ids=g["init_ids"])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    from musicgan_amd import metrics
    km = metrics.KMeans(bins=4)
    km.feed(g["x"][:3].to(DEV))
    with pytest.raises(ValueError):
        km.fit()                                                         # fewer images than bins
    with pytest.raises(ValueError):
        km.feed(g["x"][:2, :8].to(DEV))                                  # another trailing shape
    with pytest.raises(ValueError):
        _kmeans(g["x"].to(DEV), 3, init_ids=[0, 1, 96])                  # a position that was not fed


def test_seed_picks_the_rows_of_the_host_permutation():
    g = N.general(0, _chunk())
    x, k = g["x"].to(DEV), g["k"]
    ids = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(11))[:k].tolist()
    seeded, listed = _kmeans(x, k, iterations=2, seed=11), _kmeans(x, k, iterations=2, init_ids=ids)
    for a, b in zip(_outputs(seeded), _outputs(listed)):
        assert torch.equal(a, b)
    first = _kmeans(x, k, iterations=1, seed=11)
    assert int(first.changed[0]) == x.shape[0]


# ------------------------------------------------------------------ NDB
def _ndb_sets():
    """280 reference points in 7 blobs of 40, and a pool of further draws from the same blobs, by blob"""
    x, truth = N.planted_inputs(2800, 231, 7, seed=70 + 280)
    pool = [x[280:][truth[280:] == b] for b in range(7)]
    return x[:280].to(DEV), pool


def _ndb(km, query, splits=None):
    from musicgan_amd import metrics
    ndb = metrics.NDB(km)
    for lo in range(0, query.shape[0], splits or query.shape[0]):
        ndb.feed(query[lo:lo + (splits or query.shape[0])].contiguous())
    return ndb


def test_ndb_on_planted_blobs():
    ref, pool = _ndb_sets()
    km = _kmeans(ref, 7, iterations=4, init_ids=list(range(7)))
    assert km.counts.tolist() == [40] * 7 and km.changed.tolist() == [280, 0, 0, 0, 0]
    same = torch.cat([pool[b][:40] for b in range(7)]).to(DEV)           # a second draw with the same counts
    ndb = _ndb(km, same)
    assert ndb.result() == {"ndb": 0.0, "jsd": 0.0} and list(ndb.result()) == list(N.KEYS)
    per = ndb.per_bin()
    assert per["reference"] == [40] * 7 and per["query"] == [40] * 7 and per["z"] == [0.0] * 7
    sizes = (0, 47, 47, 47, 47, 46, 46)                                  # blob 0 is missing
    missing = torch.cat([pool[b][:m] for b, m in enumerate(sizes)]).to(DEV)
    ndb = _ndb(km, missing)
    got, per = ndb.result(), ndb.per_bin()
    want = N.statistics([40] * 7, sizes)
    assert per["query"] == list(sizes) and got["ndb"] == 1 / 7 == want["ndb"] and abs(got["jsd"] - want["jsd"]) <= 1e-12
    assert abs(per["z"][0] - 6.56) < 0.01 and max(abs(z) for z in per["z"][1:]) <= 0.82
    for splits in (1, 13):                                               # counts are integers: any split gives the same result
        other = _ndb(km, missing, splits)
        assert other.result() == got and other.per_bin() == per
    stuck = _ndb(km, pool[0][:280].to(DEV))                              # everything in blob 0
    assert stuck.result()["ndb"] == 1.0 and stuck.per_bin()["query"] == [280, 0, 0, 0, 0, 0, 0]
    print(f"ndb planted: missing blob {got}, stuck {stuck.result()}")


def test_fit_assign_and_feed_do_not_synchronise():
    from musicgan_amd import metrics
    g = N.general(0, _chunk())
    x, k, ids = g["x"].to(DEV), g["k"], g["init_ids"]
    warm = _kmeans(x, k, 3, iterations=2, init_ids=ids, block_bytes=40000)   # warm-up: library load, pinned memory
    _ndb(warm, x[:8])
    want = _outputs(warm) + [_ndb(warm, x).per_bin()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        km = metrics.KMeans(bins=k, iterations=2, init_ids=ids, block_bytes=40000)
        km.feed(x[:40])
        km.feed(x[40:])
        km.fit()
        seeded = metrics.KMeans(bins=k, iterations=1, seed=3)
        seeded.feed(x)
        seeded.fit()
        labels, dist = km.assign(x[:10])
        ndb = metrics.NDB(km)
        ndb.feed(x[:50])
        ndb.feed(x[50:])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(_outputs(km), want):
        assert torch.equal(a, b)
    assert ndb.per_bin() == want[4] and torch.equal(labels, km.labels[:10]) and torch.equal(dist, km.assign(x)[1][:10])


def test_parity_bodies_on_poisoned_memory():
    """the parity bodies and a split, small-block KMeans + NDB run under poison.rule pointed at km_ops: no guard band damaged by any
    launch, no argument changed that the table does not name, equal digests under both fills (nothing read that nobody wrote: a
    workspace slot no chunk owns is never read), nothing non-finite"""
    from musicgan_amd import km_ops

    def run(p):
        assert km_ops.km_update_ws_bytes(300, 1024, 7) == (300 // 32 + 7) * 1024 * 8
        p.bodies = _assign_body(0) + _order_body(300, 7) + _order_body(300, 1024) + [_update_body(0), _update_body(1)] + _count_body()
        g = N.general(0, _chunk())
        x = g["x"].to(DEV)
        whole = _kmeans(x, g["k"], iterations=3, init_ids=g["init_ids"])
        split = _kmeans(x, g["k"], 3, iterations=3, init_ids=g["init_ids"], block_bytes=40000)
        p.whole, p.split = _outputs(whole), _outputs(split)
        p.ndb = [_ndb(whole, x[:50]).per_bin(), _ndb(split, x[:50], 7).per_bin()]
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=km_ops, inplace=INPLACE)
    for a, b in zip(r0.bodies + r0.whole + r0.split, r1.bodies + r1.whole + r1.split):
        assert torch.equal(a, b)
    for a, b in zip(r1.whole, r1.split):
        assert torch.equal(a, b)
    assert r0.ndb == r1.ndb and r1.ndb[0] == r1.ndb[1]
    names = {name for name, _, _ in r1.calls}
    assert all(outs for name, _, outs in r1.calls if name in INPLACE)
    assert {"km_assign", "km_order", "km_update", "km_update_ws_bytes", "km_count"} <= names, names   # all five wrappers
    print(f"POISON ndb: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")


# ------------------------------------------------------------------ evaluate
def test_evaluate_with_ndb_on_a_tiny_corpus(tmp_path, capsys, monkeypatch):
    import musicgan_amd
    from musicgan_amd import audio, ops
    from musicgan_amd.__main__ import main
    from musicgan_amd.networks import Generator
    data_dir, ck = tiny_corpus(tmp_path, files=4, seed=6, level=2)      # 4 files x 2 samples
    dataset = audio.PackedAudioDataset(str(data_dir)) if audio.has_packed(str(data_dir)) else audio.AudioDataset(str(data_dir))
    n = len(dataset)
    assert n == 8                                                        # half = 4: 2 bins
    capsys.readouterr()
    kw = dict(level=2, nb_images=n, batch_size=3, seed=1)
    before = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("swd", "msssim", "nn", "prdc"), **kw)
    text = capsys.readouterr().out
    assert "NDB" not in text and not [name for name in before if "ndb" in name or "jsd" in name]   # without ndb: as it was
    new = ["ndb", "jsd", "ndb_real", "jsd_real"]
    full = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("swd", "msssim", "nn", "prdc", "ndb"), **kw)
    text_full = capsys.readouterr().out
    assert list(full) == list(before) + new
    assert all(full[name] == before[name] for name in before)
    added = text_full[len(text):]
    assert text_full.startswith(text) and added.count("\n") == 5         # bins, little power, two lines of numbers, how to read them
    assert "NDB: 2 k-means bins fitted on 4 real images at 16 x 16" in added and "little power" in added
    assert ("changed 0 labels" in added) != ("raise the iterations" in added)
    for name in new:
        assert f"[{name:>8}] = {full[name]:.6f}" in added, name
    assert ("ndb well above ndb_real means the samples are spread over the corpus differently from the data: modes missing or "
            "over-produced; ndb_real is about 0.05 for a held-out half") in added
    for name in new:
        v = full[name]
        assert isinstance(v, float) and 0.0 <= v <= 1.0, (name, v)
    assert full["ndb"] in (0.0, 0.5, 1.0) and full["ndb_real"] in (0.0, 0.5, 1.0)                # shares of 2 bins
    js = str(tmp_path / "eval.json")
    main(["evaluate", ck, "8", "-i", str(data_dir), "--level", "2", "-n", str(n), "--batch-size", "3", "--seed", "1",
          "--metrics", "swd,msssim,nn,prdc,ndb", "-o", js])
    with open(js) as f:
        loaded = json.load(f)
    assert loaded == full and list(loaded) == list(full)                 # the identical result through the CLI
    only = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("ndb",), **kw)
    assert only == {name: full[name] for name in new} and list(only) == new
    for bs in (1, 16):                                                   # ... and at any batch size
        assert musicgan_amd.evaluate(ck, 8, str(data_dir), ("ndb",), **dict(kw, batch_size=bs)) == only, bs
    with pytest.raises(ValueError):
        musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("ndb",), level=2, nb_images=7)
    # a "generator" that replays the half the bins were fitted on, in its order: the two histograms are the same
    real = ops.input_transform(torch.stack([dataset[i] for i in range(n)]).to(DEV).contiguous(), 16).cpu()
    first = torch.randperm(n, generator=torch.Generator().manual_seed(1)).tolist()[:n // 2]
    state = {"next": 0}

    def replay(self, z, alpha):
        out = torch.stack([real[first[(state["next"] + i) % len(first)]] for i in range(z.shape[0])]).to(z.device)
        state["next"] += z.shape[0]
        return out

    monkeypatch.setattr(Generator, "forward", replay)
    copied = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("ndb",), **kw)
    assert copied["ndb"] == 0.0 and copied["jsd"] == 0.0
    assert copied["ndb_real"] == only["ndb_real"] and copied["jsd_real"] == only["jsd_real"]
    print(f"evaluate ndb: honest {only}, replaying {copied}")

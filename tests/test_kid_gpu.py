"""GPU: the kernels of csrc/kid.hip through musicgan_amd.kid_ops, metrics.poly_mmd2 / metrics.KID and the "kid" metric of
`evaluate_mel`.  Everything is held against the float64 restatement of tests/kid_ref.py within the bound derived there from the
precisions alone; every figure is printed before it is asserted."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kid_ref as K  # noqa: E402
from eval_corpus import tiny_corpus  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the tensor arguments the wrappers of musicgan_amd/kid_ops.py write (their docstrings)
INPLACE = {
    "standardise_rows": ("out",),     # "out (n, d) float32, every element written"
    "polyk_rowsums": ("out",),        # "out (subsets, ma) float64, every element written"
}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _i32(lists):
    return torch.tensor(lists, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ standardise_rows
def _standardise_case(n, d):
    x = K.logmel_like(n, d, 30 + n)
    x[:, d // 2] = -9.25                                                 # a column without variance
    mean, sd = K.moments(x)
    assert float(sd[d // 2]) == 0.0
    if d > 4:
        sd[1], sd[2] = float("nan"), float("inf")
    return x, mean, sd


def _standardise_body(shape):
    from musicgan_amd import kid_ops
    x, mean, sd = _standardise_case(*shape)
    want = K.standardise(x, mean, sd)
    got = kid_ops.standardise_rows(x.to(DEV), mean.to(DEV), sd.to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == shape and got.is_cuda
    assert torch.equal(_bits(got.cpu()), _bits(want))
    assert float(got[:, shape[1] // 2].abs().max()) == 0.0 and bool(torch.isfinite(got).all())
    # the same rows from a base 4 bytes past a 16-byte boundary, into a given tensor
    buf = torch.zeros(x.numel() + 1, device=DEV)
    shifted = buf[1:].view(shape)
    shifted.copy_(x)
    assert shifted.data_ptr() % 16 == 4
    out = torch.empty(shape, device=DEV)
    assert kid_ops.standardise_rows(shifted, mean.to(DEV), sd.to(DEV), out) is out
    assert torch.equal(_bits(out), _bits(got))
    return got


@pytest.mark.parametrize("shape", [(5, 7), (130, 520)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_standardise_rows_is_the_float64_definition_bit_for_bit(shape):
    _standardise_body(shape)


# ------------------------------------------------------------------ polyk_rowsums: the cases
SHAPES = [(1, 1, 1), (5, 37, 231), (64, 64, 256), (70, 130, 260), (130, 257, 520), (16, 16, 4096)]
_REF = {}


def _lists(ma, mb, seed):
    """two subsets each: rows of a with repeats, and rows of b permuted (subset 0) and with repeats (subset 1)"""
    gen = torch.Generator().manual_seed(seed)
    ia = torch.randint(0, ma, (2, ma), generator=gen).tolist()
    ib = [torch.randperm(mb, generator=gen).tolist(), torch.randint(0, mb, (mb,), generator=gen).tolist()]
    return ia, ib


def _reference(shape):
    """the inputs, and for every variant (lists or not, diagonal or not) the float64 row sums and their bound: computed once"""
    if shape not in _REF:
        ma, mb, d = shape
        a, b = K.gaussian(ma, d, 40 + ma), K.gaussian(mb, d, 41 + mb + d)
        ia, ib = _lists(ma, mb, 42 + d)
        variants = {}
        for lists in (False, True):
            for skip in ((False, True) if ma == mb else (False,)):
                kw = dict(ia=ia if lists else None, ib=ib if lists else None, skip_diag=skip)
                ref, bound = K.rowsums(a, b, **kw), K.rowsums_bound(a, b, **kw)
                variants[(lists, skip)] = (kw, ref, bound)
        _REF[shape] = (a, b, variants)
    return _REF[shape]


def _rowsums_body(shape):
    from musicgan_amd import kid_ops
    a, b, variants = _reference(shape)
    ad, bd, outs = a.to(DEV), b.to(DEV), []
    for (lists, skip), (kw, ref, bound) in variants.items():
        got = kid_ops.polyk_rowsums(ad, bd, _i32(kw["ia"]) if lists else None, _i32(kw["ib"]) if lists else None, skip_diag=skip)
        assert got.dtype == torch.float64 and tuple(got.shape) == tuple(ref.shape) and got.is_cuda
        assert bool(torch.isfinite(got).all())
        err = (got.cpu() - ref).abs()
        assert bool((err[bound == 0] == 0).all())                        # one row with its diagonal skipped: no terms, exactly 0
        worst = float((err / bound)[bound > 0].max()) if bool((bound > 0).any()) else 0.0
        print(f"polyk_rowsums {shape} lists={lists} skip_diag={skip}: worst err / bound {worst:.2e}; bound {float(bound.min()):.2e} .. "
              f"{float(bound.max()):.2e}; sums {float(ref.min()):.4f} .. {float(ref.max()):.4f}")
        assert worst <= 1.0
        outs.append(got)
    return outs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_polyk_rowsums_are_the_float64_definition_within_the_derived_bound(shape):
    _rowsums_body(shape)


def test_a_row_sum_depends_on_its_row_and_its_subset_alone_and_runs_are_bit_identical():
    from musicgan_amd import kid_ops
    a, b = K.gaussian(70, 260, 50).to(DEV), K.gaussian(130, 260, 51).to(DEV)
    gen = torch.Generator().manual_seed(52)
    rows = torch.randint(0, 70, (3, 70), generator=gen)
    cols = torch.stack([torch.randperm(130, generator=gen) for _ in range(3)])
    cols[0, :40], cols[2, 90:] = cols[1, :40], cols[1, 90:]              # the three lists overlap
    rows[0, :10] = rows[1, :10]
    ia, ib = rows.to(torch.int32).to(DEV), cols.to(torch.int32).to(DEV)
    three = kid_ops.polyk_rowsums(a, b, ia, ib)
    again = kid_ops.polyk_rowsums(a, b, ia, ib)
    assert torch.equal(_bits(three), _bits(again))
    alone = kid_ops.polyk_rowsums(a, b, ia[1:2].contiguous(), ib[1:2].contiguous())
    assert torch.equal(_bits(alone[0]), _bits(three[1]))
    cut = kid_ops.polyk_rowsums(a, b, ia[1:2, :3].contiguous(), ib[1:2].contiguous())
    assert tuple(cut.shape) == (1, 3) and torch.equal(_bits(cut[0]), _bits(three[1, :3]))
    # the rows of a alone decide: the same rows named at other places of a longer list
    moved = kid_ops.polyk_rowsums(a, b, torch.cat([ia[0:1, :50], ia[1:2, :3]], 1).contiguous(), ib[1:2].contiguous())
    assert torch.equal(_bits(moved[0, 50:]), _bits(three[1, :3]))
    # no list is the list 0 .. m - 1, and gathered rows are the rows themselves
    plain = kid_ops.polyk_rowsums(a, b)
    listed = kid_ops.polyk_rowsums(a, b, _i32([list(range(70))]), _i32([list(range(130))]))
    copied = kid_ops.polyk_rowsums(a[rows[1]].contiguous(), b[cols[1]].contiguous())
    assert torch.equal(_bits(plain), _bits(listed)) and torch.equal(_bits(copied[0]), _bits(three[1]))
    # scalar loads (a base 4 bytes past a 16-byte boundary) add the same numbers in the same order
    buf = torch.zeros(a.numel() + 1, device=DEV)
    shifted = buf[1:].view(a.shape)
    shifted.copy_(a)
    assert shifted.data_ptr() % 16 == 4
    assert torch.equal(_bits(kid_ops.polyk_rowsums(shifted, b, ia, ib)), _bits(three))
    # the diagonal that is skipped is the one of positions, whatever rows stand there
    square = kid_ops.polyk_rowsums(a, a, ia, ia, skip_diag=True)
    full = kid_ops.polyk_rowsums(a, a, ia, ia)
    picked = a[rows[1]].cpu()
    own, bound = K.kernel(picked, picked).diagonal(), K.kernel_bound(picked, picked).diagonal()
    assert bool(((full[1] - square[1]).cpu() - own).abs().le(bound + 200 * K.U64 * full[1].cpu().abs()).all())


def test_both_launches_in_a_captured_graph_equal_the_eager_calls():
    from musicgan_amd import kid_ops
    x, mean, sd = (t.to(DEV) for t in _standardise_case(70, 260))
    b = K.gaussian(130, 260, 53).to(DEV)
    ia, ib = (_i32(v) for v in _lists(70, 130, 54))
    eager_z = kid_ops.standardise_rows(x, mean, sd)
    eager = kid_ops.polyk_rowsums(eager_z, b, ia, ib)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        z = kid_ops.standardise_rows(x, mean, sd)
        out = kid_ops.polyk_rowsums(z, b, ia, ib)
    z.zero_()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(z), _bits(eager_z)) and torch.equal(_bits(out), _bits(eager))


# ------------------------------------------------------------------ poly_mmd2 and KID
PLANT = dict(n=200, d=64, subsets=4, subset_size=50, seed=3)


def _feed(kid, real, fake, split=None, fake_first=False):
    """feed in pieces of `split` rows, the two sets in turn (the fake piece first if asked)"""
    n = max(real.shape[0], fake.shape[0])
    split = split or n
    for lo in range(0, n, split):
        pieces = [(kid.feed_real, real[lo:lo + split]), (kid.feed_fake, fake[lo:lo + split])]
        for feed, piece in (pieces[::-1] if fake_first else pieces):
            if piece.shape[0]:
                feed(piece.contiguous())
    return kid


def _planted(shift):
    """(real, fake) float32 host rows, the device moments of the real ones, the float64 reference of everything KID reports"""
    key = ("planted", shift)
    if key not in _REF:
        from musicgan_amd import mel_ops
        n, d = PLANT["n"], PLANT["d"]
        real, fake = K.logmel_like(n, d, 60), K.logmel_like(n - 8, d, 61, shift)
        mean, cov = (t.cpu() for t in mel_ops.moments(real.to(DEV)))     # mel_ops.moments has its own tests: taken as given
        sd = cov.diagonal().sqrt()
        zr, zf = K.standardise(real, mean, sd), K.standardise(fake, mean, sd)
        gen, m = torch.Generator().manual_seed(PLANT["seed"]), PLANT["subset_size"]
        values, bounds = [], []
        for _ in range(PLANT["subsets"]):
            x = zr[torch.randperm(n, generator=gen)[:m]]
            y = zf[torch.randperm(n - 8, generator=gen)[:m]]
            values.append(K.mmd2(x, y))
            bounds.append(K.mmd2_bound(x, y))
        values = np.array(values)
        _REF[key] = dict(real=real, fake=fake, zr=zr, zf=zf, kid=float(values.mean()), kid_std=float(values.std()),
                         bound=float(np.mean(bounds)), bound_std=float(np.max(bounds)), full=K.mmd2(zr, zf),
                         bound_full=K.mmd2_bound(zr, zf), witness=K.witness(zr, zf), bound_witness=K.witness_bound(zr, zf))
    return _REF[key]


def _kid_body(shift):
    from musicgan_amd import metrics
    ref = _planted(shift)
    real, fake = ref["real"].to(DEV), ref["fake"].to(DEV)
    kw = {k: PLANT[k] for k in ("subsets", "subset_size", "seed")}
    kid = _feed(metrics.KID(**kw), real, fake)
    zr, zf = kid.standardised()
    assert torch.equal(_bits(zr.cpu()), _bits(ref["zr"])) and torch.equal(_bits(zf.cpu()), _bits(ref["zf"]))
    got, witness = kid.result(), kid.per_sample()
    assert list(got) == ["kid", "kid_std", "kid_full"] and all(isinstance(v, float) for v in got.values())
    direct = metrics.poly_mmd2(zr, zf)
    worst = float(((witness.cpu() - ref["witness"]).abs() / ref["bound_witness"]).max())
    print(f"KID shift {shift}: kid {got['kid']:+.6f} (float64 {ref['kid']:+.6f}, bound {ref['bound']:.2e}), kid_std "
          f"{got['kid_std']:.6f} ({ref['kid_std']:.6f}), kid_full {got['kid_full']:+.6f} ({ref['full']:+.6f}, bound "
          f"{ref['bound_full']:.2e}); errors {abs(got['kid'] - ref['kid']):.2e}, {abs(got['kid_std'] - ref['kid_std']):.2e}, "
          f"{abs(got['kid_full'] - ref['full']):.2e}; witness: worst err / bound {worst:.2e}")
    assert abs(got["kid"] - ref["kid"]) <= ref["bound"]                  # a mean of estimates: within the mean of their bounds
    assert abs(got["kid_std"] - ref["kid_std"]) <= ref["bound_std"]      # |std(a) - std(b)| <= max |a_i - b_i|
    assert abs(got["kid_full"] - ref["full"]) <= ref["bound_full"]
    assert direct == got["kid_full"]
    assert tuple(witness.shape) == (fake.shape[0],) and witness.dtype == torch.float64 and worst <= 1.0
    # any split of the feeds, either set first: the same bits
    for split, fake_first in ((1, False), (7, True), (199, False)):
        other = _feed(metrics.KID(**kw), real, fake, split, fake_first)
        assert other.result() == got and torch.equal(_bits(other.per_sample()), _bits(witness)), (split, fake_first)
    return [zr, zf, witness]


def test_kid_of_planted_sets_is_the_reference_within_the_summed_bound_for_any_feed_split():
    _kid_body(0.0)
    _kid_body(0.5)
    same, moved = _planted(0.0), _planted(0.5)
    assert moved["full"] > 10.0 * abs(same["full"]) and moved["kid"] > 10.0 * same["kid_std"]   # the float64 values: a shift shows


def test_a_disjoint_sample_of_one_distribution_scores_within_three_deviations():
    from musicgan_amd import metrics
    x, y = K.gaussian(400, 16, 0).to(DEV), K.gaussian(400, 16, 1).to(DEV)
    got = _feed(metrics.KID(subsets=20, subset_size=100, seed=0), x, y, 64).result()
    print(f"KID of two samples of one Gaussian, 20 subsets of 100 of 400 x 16: {got}")
    assert abs(got["kid"]) <= 3.0 * got["kid_std"] and got["kid_std"] > 0.0
    whole = _feed(metrics.KID(subsets=20, subset_size=400, seed=0), x, y).result()
    assert whole["kid_std"] == 0.0 and whole["kid"] == whole["kid_full"] == got["kid_full"]   # the one subset there is
    moved = _feed(metrics.KID(subsets=20, subset_size=100, seed=0), x, K.gaussian(400, 16, 1, 0.5).to(DEV)).result()
    print(f"... and with the second set shifted by 0.5: {moved}")
    assert moved["kid"] > 20.0 * moved["kid_std"] / np.sqrt(20)


def test_kid_refuses_too_few_rows_and_another_shape():
    from musicgan_amd import _lib, metrics
    kid = metrics.KID()
    kid.feed_real(K.gaussian(5, 4, 2).to(DEV))
    kid.feed_fake(K.gaussian(1, 4, 3).to(DEV))
    with pytest.raises(ValueError):
        kid.result()
    with pytest.raises(ValueError):
        kid.feed_fake(K.gaussian(3, 5, 4).to(DEV))
    kid.feed_fake(K.gaussian(3, 4, 4).to(DEV))
    assert all(np.isfinite(v) for v in kid.result().values())            # 5 and 4 rows of 4 numbers: subsets of 4
    with pytest.raises(_lib.MusicGanHipError):
        metrics.poly_mmd2(K.gaussian(5, 4, 2), K.gaussian(5, 4, 3))      # on the host


# ------------------------------------------------------------------ poisoned memory
def test_parity_bodies_on_poisoned_memory():
    """the parity bodies under poison.rule pointed at kid_ops: no guard band damaged by any launch, no argument changed that the
    table does not name, equal digests under both fills (nothing read that nobody wrote), nothing non-finite"""
    from musicgan_amd import kid_ops

    def run(p):
        assert kid_ops.polyk_ws_bytes(2, 130, 257) == 2 * 3 * 130 * 8
        p.bodies = [_standardise_body((5, 7)), _standardise_body((130, 520))]
        for shape in ((1, 1, 1), (5, 37, 231), (64, 64, 256), (70, 130, 260), (130, 257, 520)):
            p.bodies += _rowsums_body(shape)
        p.bodies += _kid_body(0.5)
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=kid_ops, inplace=INPLACE)
    for a, b in zip(r0.bodies, r1.bodies):
        assert torch.equal(a, b)
    names = {name for name, _, _ in r1.calls}
    assert all(outs for name, _, outs in r1.calls if name in INPLACE)
    assert {"standardise_rows", "polyk_rowsums", "polyk_ws_bytes"} <= names, names   # all three wrappers
    print(f"POISON kid: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")


# ------------------------------------------------------------------ evaluate_mel
KW = dict(level=4, nb_images=16, batch_size=3, seed=1)
KID_KEYS = ["kid", "kid_std", "kid_full", "kid_real", "kid_real_std"]
FD_KEYS = ["fd", "fd_half", "fd_real"]
NDB_KEYS = ["ndb", "jsd", "ndb_real", "jsd_real"]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """16 dataset entries of 64 x 64 and a generator at level 4, the kid run and its printed text: made once for the tests below"""
    import contextlib
    import io
    import musicgan_amd
    root = tmp_path_factory.mktemp("kid")
    data_dir, ck = tiny_corpus(root, files=8, seed=7, level=4)
    fn = musicgan_amd.__getattr__("evaluate_mel")                        # the lazy export itself
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        only = fn(ck, 8, data_dir, ("kid",), **KW)
    return dict(root=root, data=data_dir, ck=ck, fn=fn, only=only, text=text.getvalue())


def test_evaluate_mel_reports_kid_in_log_mel_space(corpus):
    only, text = corpus["only"], corpus["text"]
    print(text)
    assert list(only) == KID_KEYS and all(isinstance(v, float) and np.isfinite(v) for v in only.values()), only
    assert "Evaluate 16 real and 16 generated images of 64 x 64" in text
    space = "in log-mel space (8 bands x 8 pools, standardised by the real images' moments)"
    assert f"KID [     kid] = {only['kid']:.6f} +- {only['kid_std']:.6f} {space}, 1 subset of 16 real against 16 generated" in text
    assert f"KID [kid_full] = {only['kid_full']:.6f} {space}, 16 real against 16 generated images" in text
    assert f"KID [kid_real] = {only['kid_real']:.6f} +- {only['kid_real_std']:.6f} {space}, 1 subset of 8 real against 8 real" in text
    assert "FD [" not in text and text.count("KID [") == 3
    # 16 images are fewer than a subset of 1000: the one subset there is, the whole sets
    assert only["kid_std"] == 0.0 and only["kid_real_std"] == 0.0 and only["kid"] == only["kid_full"]


def test_evaluate_mel_kid_with_other_metrics_and_through_the_cli(corpus, capsys):
    from musicgan_amd.__main__ import main
    fn, ck, data, only = corpus["fn"], corpus["ck"], corpus["data"], corpus["only"]
    mixed = fn(ck, 8, data, ("ndb", "kid", "fd"), **KW)                  # the order run is METRICS_ALL's, not the order asked for
    assert list(mixed) == FD_KEYS + NDB_KEYS + KID_KEYS
    assert {k: mixed[k] for k in KID_KEYS} == only
    js = str(corpus["root"] / "kid.json")
    capsys.readouterr()
    main(["evaluate_mel", ck, "8", "-i", data, "--level", "4", "-n", "16", "--batch-size", "3", "--seed", "1", "--metrics", "kid",
          "-o", js])
    with open(js) as f:
        loaded = json.load(f)
    assert loaded == only and list(loaded) == KID_KEYS
    assert capsys.readouterr().out == corpus["text"]
    with pytest.raises(ValueError):
        fn(ck, 8, data, ("kid",), level=4, nb_images=3)


REAL_KEYS = ["kid_real", "kid_real_std"]


def test_evaluate_mel_kid_real_side_does_not_depend_on_the_batch_size(corpus):
    """what is made of real images alone (the moments, the standardisation, the two halves) is the same for any batching"""
    fn, ck, data, only = corpus["fn"], corpus["ck"], corpus["data"], corpus["only"]
    for bs in (1, 3, 16):
        other = fn(ck, 8, data, ("kid",), **dict(KW, batch_size=bs))
        assert {k: other[k] for k in REAL_KEYS} == {k: only[k] for k in REAL_KEYS}, bs


def test_evaluate_mel_kid_results_are_equal_for_batch_sizes_3_and_16(corpus):
    """All five keys.  The generator's kernels are chosen by the batch size, so its images differ in their last float32 bits from
    one batching to another (up to 2.1e-6 between batches of 3 and of 16 at this level, measured: `kid` of this corpus moved by
    1.4e-7 of its value when the runner drew them in batches of `batch_size`); the runner draws them in batches of 16 whatever
    `batch_size` is, and a real row does not depend on its batch."""
    fn, ck, data, only = corpus["fn"], corpus["ck"], corpus["data"], corpus["only"]
    for bs in (3, 16):
        other = fn(ck, 8, data, ("kid",), **dict(KW, batch_size=bs))
        print(f"evaluate_mel kid at batch size {bs}: {other}")
        assert other == only, bs

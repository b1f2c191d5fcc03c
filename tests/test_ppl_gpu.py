"""GPU: the kernels of csrc/ppl.hip through musicgan_amd.ppl_ops, metrics.PPL and the `path_length` driver.  Everything is held
against the float64 restatement of tests/ppl_ref.py within bounds that the precisions alone give; every figure is
printed before it is asserted."""
import contextlib
import io
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppl_ref as R  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-4
# the tensor arguments the wrappers of musicgan_amd/ppl_ops.py write (their docstrings)
INPLACE = {
    "rows_sqdist": ("out",),          # "out (n,) float64, every element written"
}


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


# ------------------------------------------------------------------ slerp_pairs
T0, ANTIPODAL, EQUAL, PARALLEL, ZERO, LATE = range(6)   # the rows of a case that are not a general pair, where it has that many


def _slerp_case(n, d):
    """z0, z1 (n, d) float32 and t (n,) float64 on the host.  Row 0: t = 0; row 1: antipodal ends; row 2: equal ends at t = 1 - eps;
    row 3: ends at an angle of about 1e-7; row 4: a zero vector; row 5: a general pair at t = 1 - eps; the rest: general pairs at
    random t.  With d = 1 two vectors are parallel or antipodal: every z1 but row 1's is given the sign of its z0."""
    g = torch.Generator().manual_seed(100 * d + n)
    z0, z1 = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    t = torch.rand(n, dtype=torch.float64, generator=g)
    if d == 1:
        z1 = z1.abs() * z0.sign()
    t[T0] = 0.0
    if n > ANTIPODAL:
        z1[ANTIPODAL] = -z0[ANTIPODAL]
    if n > EQUAL:
        z1[EQUAL], t[EQUAL] = z0[EQUAL], 1.0 - EPS
    if n > PARALLEL and d > 1:
        a = z0[PARALLEL].double()
        p = z1[PARALLEL].double()
        p = p - a * (p @ a) / (a @ a)                                     # orthogonal to a
        z1[PARALLEL] = (a + 1e-7 * a.norm() * p / p.norm()).float()
    if n > ZERO:
        z0[ZERO] = 0.0
    if n > LATE:
        t[LATE] = 1.0 - EPS
    return z0, z1, t


def _slerp_body(n, d):
    from musicgan_amd import ppl_ops
    z0, z1, t = _slerp_case(n, d)
    za, zb, flag = ppl_ops.slerp_pairs(z0.to(DEV), z1.to(DEV), t.to(DEV), EPS)
    assert za.dtype == zb.dtype == torch.float32 and flag.dtype == torch.int32 and za.is_cuda
    assert tuple(za.shape) == tuple(zb.shape) == (n, d) and tuple(flag.shape) == (n,)
    ra, rb, ma, mb, rflag = R.slerp_pairs(z0.numpy(), z1.numpy(), t.numpy(), EPS)
    want_flag = [int(i == ANTIPODAL) for i in range(n)]
    assert flag.tolist() == want_flag == rflag.tolist()                   # set for the antipodal pair, and for no other
    worst = 0.0
    for got, ref, mag in ((za, ra, ma), (zb, rb, mb)):
        got = got.cpu().double().numpy()
        assert np.isfinite(got).all()
        worst = max(worst, float((np.abs(got - ref) / R.slerp_bound(ref, mag, d)).max()))
    print(f"slerp_pairs n = {n}, d = {d}: worst error / (half a float32 ulp + gamma_{d + 8} (|w0 z0| + |w1 z1|)) = {worst:.4f}")
    assert worst <= 1.0
    assert torch.equal(_bits(za[T0].cpu()), _bits(z0[T0]))                # t = 0: the first end, bit for bit
    if n > ANTIPODAL:
        assert float(za[ANTIPODAL].abs().max()) == 0.0 and float(zb[ANTIPODAL].abs().max()) == 0.0
    if n > EQUAL:
        assert torch.equal(_bits(za[EQUAL].cpu()), _bits(z0[EQUAL])) and torch.equal(_bits(zb[EQUAL].cpu()), _bits(z0[EQUAL]))
    return [za, zb, flag]


@pytest.mark.parametrize("n", [1, 5, 37])
@pytest.mark.parametrize("d", [1, 3, 32, 128, 2049])
def test_slerp_pairs_are_the_float64_definition_rounded_once(n, d):
    _slerp_body(n, d)


@pytest.mark.parametrize("d", [1, 3, 32, 128, 2049])
def test_a_pair_depends_on_its_rows_alone_and_runs_are_bit_identical(d):
    from musicgan_amd import ppl_ops
    z0, z1, t = (v.to(DEV) for v in _slerp_case(37, d))
    whole = ppl_ops.slerp_pairs(z0, z1, t, EPS)
    again = ppl_ops.slerp_pairs(z0, z1, t, EPS)
    head = ppl_ops.slerp_pairs(z0[:1].contiguous(), z1[:1].contiguous(), t[:1].contiguous(), EPS)
    rest = ppl_ops.slerp_pairs(z0[1:].contiguous(), z1[1:].contiguous(), t[1:].contiguous(), EPS)
    for w, a, h, r in zip(whole, again, head, rest):
        assert torch.equal(_bits(w), _bits(a)) and torch.equal(_bits(w), _bits(torch.cat([h, r])))
    # 4-byte loads (a base 4 bytes past a 16-byte boundary) add the same numbers in the same order
    shifted = []
    for z in (z0, z1):
        buf = torch.zeros(z.numel() + 1, device=DEV)
        s = buf[1:].view(z.shape)
        s.copy_(z)
        assert s.data_ptr() % 16 == 4
        shifted.append(s)
    for w, s in zip(whole, ppl_ops.slerp_pairs(shifted[0], shifted[1], t, EPS)):
        assert torch.equal(_bits(w), _bits(s))


# ------------------------------------------------------------------ rows_sqdist
def _sqdist_case(n, d):
    g = torch.Generator().manual_seed(7 * d + n)
    a = torch.randn(n, d, generator=g)
    b = a + 1e-3 * torch.randn(n, d, generator=g)                         # as close as the two images of a pair
    if n > 1:
        b[1] = torch.randn(d, generator=g)                                # and as far apart as two samples
    return a, b, 1.0 / (d * EPS * EPS)


def _sqdist_body(n, d):
    from musicgan_amd import ppl_ops
    a, b, scale = _sqdist_case(n, d)
    got = ppl_ops.rows_sqdist(a.to(DEV), b.to(DEV), scale)
    assert got.dtype == torch.float64 and tuple(got.shape) == (n,) and got.is_cuda
    ref = R.rows_sqdist(a.numpy(), b.numpy(), scale)
    assert (ref > 0).all()
    worst = float((np.abs(got.cpu().numpy() - ref) / (R.gamma(d + 2) * ref)).max())
    print(f"rows_sqdist n = {n}, D = {d}: worst relative error / gamma_{d + 2} = {worst:.4f}; values {ref.min():.3e} .. {ref.max():.3e}")
    assert worst <= 1.0
    out = torch.empty(n, dtype=torch.float64, device=DEV)
    assert ppl_ops.rows_sqdist(a.to(DEV), b.to(DEV), scale, out) is out and torch.equal(_bits(out), _bits(got))
    return [got]


@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 512, 2048])
def test_rows_sqdist_is_the_float64_sum_within_gamma_of_its_length(n, d):
    _sqdist_body(n, d)


@pytest.mark.parametrize("d", [1, 63, 64, 65, 512, 2048])
def test_a_distance_depends_on_its_pair_alone(d):
    from musicgan_amd import ppl_ops
    a, b, scale = _sqdist_case(70, d)
    a, b = a.to(DEV), b.to(DEV)
    whole = ppl_ops.rows_sqdist(a, b, scale)
    assert torch.equal(_bits(whole), _bits(ppl_ops.rows_sqdist(a, b, scale)))                     # from run to run
    for cut in (1, 3, 69):
        parts = [ppl_ops.rows_sqdist(a[:cut].contiguous(), b[:cut].contiguous(), scale),
                 ppl_ops.rows_sqdist(a[cut:].contiguous(), b[cut:].contiguous(), scale)]
        assert torch.equal(_bits(torch.cat(parts)), _bits(whole)), cut
    assert float(ppl_ops.rows_sqdist(a, a.clone(), scale).abs().max()) == 0.0                      # equal rows: exactly 0
    buf = torch.zeros(a.numel() + 1, device=DEV)                          # 4-byte loads: the same numbers in the same order
    shifted = buf[1:].view(a.shape)
    shifted.copy_(a)
    assert shifted.data_ptr() % 16 == 4
    assert torch.equal(_bits(ppl_ops.rows_sqdist(shifted, b, scale)), _bits(whole))
    bad = a.clone()                                                       # a NaN and an infinity stay in their pairs
    bad[1, d // 2], bad[2, 0] = float("nan"), float("inf")
    got = ppl_ops.rows_sqdist(bad, b, scale)
    assert math.isnan(float(got[1])) and float(got[2]) == float("inf")
    keep = [i for i in range(70) if i not in (1, 2)]
    assert torch.equal(_bits(got[keep]), _bits(whole[keep]))


# ------------------------------------------------------------------ metrics.PPL on an exact map
PLANT = dict(n=200, channels=8, seed=5)


class _ExactRows:
    """rows = latents times a (32, 96) integer matrix with one entry of +-1, +-2 or +-4 per column: every row element is one product
    of a float32 and a power of two, exact in float32 and in float64 alike.  Keeps the latents it was called with."""

    def __init__(self):
        g = torch.Generator().manual_seed(11)
        d = 4 * PLANT["channels"]
        self.index = torch.cat([torch.randperm(d, generator=g) for _ in range(3)])
        self.coef = (2 ** torch.randint(0, 3, (3 * d,), generator=g) * (2 * torch.randint(0, 2, (3 * d,), generator=g) - 1)).float()
        self.calls = []

    def host(self, latents):
        return latents.reshape(latents.shape[0], -1).double()[:, self.index] * self.coef.double()

    def __call__(self, latents):
        self.calls.append(latents.cpu())
        return (latents.reshape(latents.shape[0], -1)[:, self.index.to(latents.device)] * self.coef.to(latents.device)).contiguous()


def _ppl_body(feeds, sampling="full"):
    from musicgan_amd import metrics
    rows = _ExactRows()
    ppl = metrics.PPL(rows, EPS, sampling, PLANT["seed"], rand_channels=PLANT["channels"])
    for n in feeds:
        ppl.feed(n)
    values, flags, chord, result = ppl.per_pair(), ppl.flags(), ppl.per_pair_chord(), ppl.result()
    return rows, values, flags, chord, result


def test_ppl_on_an_exact_linear_map_is_the_reference_for_any_split_of_the_feeds():
    n, c = PLANT["n"], PLANT["channels"]
    rows, values, flags, chord, result = _ppl_body([n])
    assert values.dtype == torch.float64 and values.is_cuda and tuple(values.shape) == (n,) and int(flags.sum()) == 0
    calls = rows.calls
    assert [x.shape[0] for x in calls] == [16] * (2 * n // 8) and all(tuple(x.shape[1:]) == (c, 2, 2) for x in calls)
    steps, ends = torch.cat(calls[:n // 8]), torch.cat(calls[n // 8:])    # za_i, zb_i adjacent; then z0_i, z1_i adjacent
    # the latents are the draws the class documents, walked by the definition
    g = torch.Generator(device=DEV).manual_seed(PLANT["seed"])
    z0, z1 = (torch.randn(n, 4 * c, device=DEV, generator=g).cpu() for _ in range(2))
    t = torch.rand(n, dtype=torch.float64, device=DEV, generator=g).cpu()
    assert torch.equal(ends[0::2].reshape(n, -1), z0) and torch.equal(ends[1::2].reshape(n, -1), z1)
    ra, rb, ma, mb, rflag = R.slerp_pairs(z0.numpy(), z1.numpy(), t.numpy(), EPS)
    for got, ref, mag in ((steps[0::2], ra, ma), (steps[1::2], rb, mb)):
        assert float((np.abs(got.reshape(n, -1).double().numpy() - ref) / R.slerp_bound(ref, mag, 4 * c)).max()) <= 1.0
    # the per-pair values against the float64 definition on the rows of the latents the device walked: rows_sqdist's bound
    dims = 12 * c
    want = R.per_pair(rows.host(steps[0::2]).numpy(), rows.host(steps[1::2]).numpy(), EPS)
    want_chord = R.rows_sqdist(rows.host(z0).numpy(), rows.host(z1).numpy(), 1.0 / dims)
    worst = float((np.abs(values.cpu().numpy() - want) / (R.gamma(dims + 2) * want)).max())
    worst_chord = float((np.abs(chord.cpu().numpy() - want_chord) / (R.gamma(dims + 2) * want_chord)).max())
    print(f"PPL on an exact map, {n} pairs, D = {dims}: worst relative error / gamma_{dims + 2} = {worst:.4f} (chords {worst_chord:.4f}); "
          f"{result}")
    assert worst <= 1.0 and worst_chord <= 1.0
    # the keys: the reference's aggregation of the device's own values, exactly
    assert result == R.aggregate(values.cpu().numpy(), flags.cpu().numpy(), chord.cpu().numpy())
    assert list(result) == ["ppl", "ppl_mean", "ppl_chord", "ppl_ratio", "ppl_pairs"] and result["ppl_pairs"] == n
    # a near-isotropic linear map of great-circle arcs at angles near pi / 2: about (w / (2 sin(w / 2)))^2 = 1.23, and >= 1 in expectation
    assert result["ppl_ratio"] >= 1.0
    # fed as 7 + 193: the same bits
    _, values2, flags2, chord2, result2 = _ppl_body([7, 193])
    assert torch.equal(_bits(values2), _bits(values)) and torch.equal(_bits(chord2), _bits(chord)) and torch.equal(flags2, flags)
    assert result2 == result
    # "end" sampling: t = 0, no chords
    rows_e, values_e, flags_e, chord_e, result_e = _ppl_body([n], "end")
    assert chord_e is None and list(result_e) == ["ppl", "ppl_mean", "ppl_pairs"] and len(rows_e.calls) == n // 8
    first = torch.cat(rows_e.calls)[0::2].reshape(n, -1)
    assert torch.equal(_bits(first), _bits(z0))                           # za = z0, bit for bit
    assert result_e == R.aggregate(values_e.cpu().numpy(), flags_e.cpu().numpy())


def test_ppl_leaves_an_antipodal_pair_out_of_every_mean(monkeypatch):
    from musicgan_amd import metrics, ppl_ops
    real = ppl_ops.slerp_pairs

    def with_an_antipodal_pair(z0, z1, t, eps):
        z1 = z1.clone()
        z1[3] = -z0[3]
        return real(z0, z1, t, eps)

    monkeypatch.setattr(ppl_ops, "slerp_pairs", with_an_antipodal_pair)
    rows = _ExactRows()
    ppl = metrics.PPL(rows, EPS, "end", 0, rand_channels=PLANT["channels"])
    ppl.feed(20)
    values, flags, result = ppl.per_pair(), ppl.flags(), ppl.result()
    assert flags.tolist() == [int(i == 3) for i in range(20)] and math.isnan(float(values[3]))
    assert result["ppl_pairs"] == 19 and result == R.aggregate(values.cpu().numpy(), flags.cpu().numpy())
    assert math.isfinite(result["ppl"]) and math.isfinite(result["ppl_mean"])


# ------------------------------------------------------------------ poisoned memory
def test_parity_bodies_on_poisoned_memory():
    """the parity bodies under poison.rule pointed at ppl_ops: no guard band damaged by any launch, no argument changed that the
    table does not name, equal digests under both fills (nothing read that nobody wrote), nothing non-finite"""
    from musicgan_amd import ppl_ops

    def run(p):
        p.bodies = []
        for n, d in ((1, 1), (5, 3), (37, 32), (5, 128), (5, 2049)):
            p.bodies += _slerp_body(n, d)
        for n, d in ((1, 1), (3, 63), (70, 64), (3, 65), (70, 512), (3, 2048)):
            p.bodies += _sqdist_body(n, d)
        _, values, flags, chord, _ = _ppl_body([40])
        p.bodies += [values, flags, chord]
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=ppl_ops, inplace=INPLACE)
    for a, b in zip(r0.bodies, r1.bodies):
        assert torch.equal(a, b)
    names = {name for name, _, _ in r1.calls}
    assert all(outs for name, _, outs in r1.calls if name in ("slerp_pairs", "rows_sqdist"))
    assert {"slerp_pairs", "rows_sqdist"} <= names, names                 # both wrappers
    print(f"POISON ppl: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")


# ------------------------------------------------------------------ path_length
KW = dict(level=4, nb_pairs=40, seed=1)
KEYS = ["ppl", "ppl_mean", "ppl_chord", "ppl_ratio", "ppl_pairs"]


def _quiet(fn, *args, **kw):
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        result = fn(*args, **kw)
    return result, text.getvalue()


def _checkpoint(root, level, zero=False):
    """the state of Generator(8, end_layer=level) built after torch.manual_seed(0), as tests/eval_corpus.py saves it"""
    from musicgan_amd.networks import Generator
    torch.manual_seed(0)
    state = Generator(8, end_layer=level).state_dict()
    if zero:
        state = {k: torch.zeros_like(v) for k, v in state.items()}
    ck = str(root / f"gen{level}{'_zero' if zero else ''}.pt")
    torch.save(state, ck)
    return ck


@pytest.fixture(scope="module")
def run4(tmp_path_factory):
    """a generator at level 4, the run of 40 pairs on it and its printed text: made once for the tests below"""
    import musicgan_amd
    root = tmp_path_factory.mktemp("ppl")
    ck = _checkpoint(root, 4)
    fn = musicgan_amd.__getattr__("path_length")                          # the lazy export itself
    js = str(root / "ppl.json")
    result, text = _quiet(fn, ck, 8, output=js, **KW)
    return dict(root=root, ck=ck, fn=fn, js=js, result=result, text=text)


def test_path_length_reports_its_keys_in_log_mel_space(run4):
    result, text = run4["result"], run4["text"]
    print(text)
    assert list(result) == KEYS and result["ppl_pairs"] == 40 and isinstance(result["ppl_pairs"], int)
    assert all(isinstance(result[k], float) and np.isfinite(result[k]) and result[k] > 0.0 for k in KEYS[:4]), result
    assert result["ppl_ratio"] == result["ppl_mean"] / result["ppl_chord"]
    with open(run4["js"]) as f:
        assert json.load(f) == result
    space = "in log-mel space (8 bands x 8 pools)"
    for key in KEYS[:4]:
        assert f"PPL [{key:>9}] = {result[key]:.6f} {space}" in text
    assert f"PPL [ppl_pairs] = 40 {space}" in text and "PPL: ppl_ratio is the mean squared speed" in text
    assert "Walk 40 pairs of latents, epsilon = 0.0001, full sampling, images of 64 x 64" in text and text.count("PPL [") == 5


def test_path_length_is_the_same_from_run_to_run_and_through_the_cli(run4, capsys):
    from musicgan_amd.__main__ import main
    again, text = _quiet(run4["fn"], run4["ck"], 8, **KW)
    assert again == run4["result"] and text == run4["text"]
    js = str(run4["root"] / "cli.json")
    capsys.readouterr()
    main(["path_length", run4["ck"], "8", "--level", "4", "-n", "40", "--seed", "1", "-o", js])
    assert capsys.readouterr().out == run4["text"]
    with open(js) as f:
        assert json.load(f) == run4["result"]
    other, _ = _quiet(run4["fn"], run4["ck"], 8, **dict(KW, seed=2))
    assert other["ppl"] != run4["result"]["ppl"]


def test_path_length_at_the_end_of_the_arc_has_no_chord(run4):
    end, text = _quiet(run4["fn"], run4["ck"], 8, sampling="end", **KW)
    assert list(end) == ["ppl", "ppl_mean", "ppl_pairs"] and end["ppl_pairs"] == 40 and end["ppl"] > 0.0
    assert "ppl_ratio" not in text and "ppl_chord" not in text and "end sampling" in text


def test_path_length_of_a_generator_of_zeros_is_exactly_zero(run4):
    ck = _checkpoint(run4["root"], 4, zero=True)
    result, _ = _quiet(run4["fn"], ck, 8, **KW)
    assert result["ppl"] == 0.0 and result["ppl_mean"] == 0.0 and result["ppl_chord"] == 0.0 and result["ppl_pairs"] == 40
    assert math.isnan(result["ppl_ratio"])                                # 0 / 0: no path, no chord


def test_path_length_scores_the_waveforms_at_level_7(run4):
    ck = _checkpoint(run4["root"], 7)
    result, text = _quiet(run4["fn"], ck, 8, level=7, nb_pairs=4, seed=1, waveform=True)
    print(text)
    assert list(result) == KEYS and result["ppl_pairs"] == 4
    assert all(np.isfinite(result[k]) and result[k] > 0.0 for k in KEYS[:4]), result
    assert "in waveform log-mel space (64 bands x 8 pools)" in text and "images of 512 x 512" in text

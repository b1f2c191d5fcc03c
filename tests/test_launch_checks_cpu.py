"""The comparisons of tests/launch_checks.py on host tensors (no GPU): sliced over the images exactly as on the device, each of them
-- `_check` (sliced max-norm), `_report` (whole tensor), `_check_tile_mask` (sign bits) -- passes on a float32 rounding of its
float64 reference and fails, naming itself, when ONE value is off by four times what its bound allows (one bit of a tile mask):
an interior element, and the last element of the last image's last row, which sits in a short last slice.

Also what the configurations of levels 0-2 rest on: the side of a level (4 << level) is bench.LEVEL_SIDE's wherever that table has
the level, every committed census file reads back line for line, and the float64 restatement of the lone 1x1 convs
(`_check_conv1x1`), run here over a plain float32 torch stand-in of `ops.conv1x1`, passes at the committed level-0 lines and
notices one wrong element in each of its four comparisons."""
import glob
import os

import pytest
import torch
import torch.nn.functional as F

import launch_checks as L
from routing_census import parse, spec

HERE = os.path.dirname(os.path.abspath(__file__))


def _run(n, c, h, w, tol, monkeypatch, chunk):
    monkeypatch.setattr(L, "CHUNK", chunk)
    g = torch.Generator().manual_seed(n * 1000 + c)
    ref = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    got, mask = ref.float(), L._tile_mask(ref)

    def run(hook):
        with L._hooked(hook):
            L._check("sliced", got, lambda i0, i1: ref[i0:i1], tol)
            L._report("whole", got, ref, tol)
            L._check_tile_mask("mask", mask, lambda i0, i1: ref[i0:i1])
    return run


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (5, 3, 8, 6), (7, 2, 4, 4)])
def test_each_comparison_notices_one_wrong_element(shape, monkeypatch):
    run = _run(*shape, 2e-6, monkeypatch, chunk=3)  # 7 images in slices of 3: the last slice holds one image
    seen = []
    run(L.listen(seen))
    assert seen == ["sliced", "whole", "mask"]
    L.must_notice(run, seen)
    assert L._hook is None


def test_slices_cover_every_image_once_and_are_bounded_in_size():
    for n, per_image in [(192, 64 * 128 * 128), (18, 32 * 512 * 512), (6, 1), (1, 1 << 40), (17, L.SLICE // 16 + 1)]:
        sl = L._slices(n, per_image)
        assert [i for i0, i1 in sl for i in range(i0, i1)] == list(range(n))
        assert all(i1 - i0 <= L.CHUNK and ((i1 - i0) * per_image <= L.SLICE or i1 - i0 == 1) for i0, i1 in sl)
    assert L._slices(192, 64 * 128 * 128)[0] == (0, 16)  # the headline's slices: 16 images


def test_side_of_a_level_is_the_benchmarks():
    import bench
    assert sorted(bench.LEVEL_SIDE) == [3, 4, 5, 6, 7]
    for level, side in bench.LEVEL_SIDE.items():
        assert 4 << level == side


def _rows(path):
    with open(path) as f:
        return [r for r in f.read().splitlines() if r.strip()]


CENSUS_FILES = sorted(glob.glob(os.path.join(HERE, "census_level*_batch*.txt")))


def test_committed_census_files_parse():
    """Every row is a section header or a line that `parse` reads and `spec` writes back unchanged; each file has the three
    sections in order, launches only under the first, deferred weight gradients only under the other two."""
    names = {os.path.basename(p) for p in CENSUS_FILES}
    assert {f"census_level{lv}_batch{b}.txt" for lv in (0, 1, 2) for b in (6, 64)} <= names
    for path in CENSUS_FILES:
        rows = _rows(path)
        heads = [r for r in rows if r.startswith("[")]
        assert heads == ["[launches]", "[critic sweep]", "[generator sweep]"], path
        sect = None
        for r in rows:
            if r.startswith("["):
                sect = r
                continue
            rec = parse(r)
            assert spec(rec) == r, (path, r)
            if sect == "[launches]":
                assert L._launch(rec[0]), (path, r)
            else:
                assert rec[0] == "conv3x3_wgrad" and dict(rec[1]).get("defer") == "WgradDefer", (path, r)
        assert len(rows) > 3, path


class _FakeOps:
    """`ops.conv1x1` in plain float32 torch on the host."""

    @staticmethod
    def conv1x1(x, w, bias, cout, *, lrelu=False, tanh=False, mask_aux=None, transposed=False, out=None):
        y = F.conv_transpose2d(x, w) if transposed else F.conv2d(x, w, bias)
        assert y.shape[1] == cout
        if lrelu:
            y = F.leaky_relu(y, L.SLOPE)
        if tanh:
            y = torch.tanh(y)
        if mask_aux is not None:
            y = y * torch.where(mask_aux > 0, 1.0, L.SLOPE)
        return y if out is None else out.copy_(y)


CONV1X1 = [r for r in _rows(os.path.join(HERE, "census_level0_batch6.txt")) if r.startswith("conv1x1 ")]


@pytest.fixture
def on_host(monkeypatch):
    monkeypatch.setattr(L, "DEV", "cpu")
    monkeypatch.setattr(L, "_ops", lambda: _FakeOps)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)


def test_level0_lists_all_four_forms_of_the_lone_conv1x1():
    forms = {tuple(k for k in ("lrelu", "tanh", "transposed", "mask_aux") if dict(parse(r)[1]).get(k)) for r in CONV1X1}
    assert forms == {("lrelu",), ("tanh",), ("transposed",), ("mask_aux",)}


@pytest.mark.parametrize("line", CONV1X1, ids=[f"{i}" for i in range(len(CONV1X1))])
def test_conv1x1_restatement_notices_one_wrong_element(line, on_host):
    seen = []
    L.check_launch(line, L.listen(seen))
    assert len(seen) == 1 and seen[0].startswith("conv1x1 ")
    L.must_notice(lambda hook: L.check_launch(line, hook), seen)
    assert L._hook is None


def test_conv1x1_restatement_refuses_a_form_it_does_not_restate(on_host):
    for line in ("conv1x1 x=[2,2,4,4] w=[8,2,1,1] bias=None cout=8 transposed=True tanh_bwd_in=[2,2,4,4]",
                 "conv1x1 x=[2,2,4,4] w=[8,2,1,1] bias=None cout=8"):
        with pytest.raises(AssertionError, match="no headline-shape check for conv1x1"):
            L.check_launch(line)

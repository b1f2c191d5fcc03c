"""The comparisons of tests/launch_checks.py on host tensors (no GPU): sliced over the images exactly as on the device, each of them
-- `_check` (sliced max-norm), `_report` (whole tensor), `_check_tile_mask` (sign bits) -- passes on a float32 rounding of its
float64 reference and fails, naming itself, when ONE value is off by four times what its bound allows (one bit of a tile mask):
an interior element, and the last element of the last image's last row, which sits in a short last slice."""
import pytest
import torch

import launch_checks as L


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

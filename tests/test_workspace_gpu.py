"""GPU: one scratch cache for every op module (`ops.workspace`, `ops._ws_cache`).  Three domains -- the phase vocoder, true peak and
Griffin-Lim -- take turns on the one buffer of a stream, the third makes it grow, and every result is bit for bit what the same
call gives alone on a fresh cache: no call depends on what another left in the buffer, and none holds it across another's call.
No tolerance is involved."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1 << 20       # the smallest buffer `ops.workspace` allocates


def test_domains_alternating_on_one_buffer_are_bit_equal_to_each_alone(monkeypatch):
    from musicgan_amd import gl_ops, loud_ops, ops, pv_ops
    for m in (gl_ops, loud_ops, pv_ops):
        assert not hasattr(m, "_ws_cache") and not hasattr(m, "workspace")
    # the smallest Griffin-Lim whose scratch memory no longer fits the floor: the buffer the first two calls shared has to grow
    frames = next(t for t in range(8, 1 << 12) if gl_ops.griffin_lim_ws_bytes(t, 2) > FLOOR)
    g = torch.Generator().manual_seed(20)
    X = torch.view_as_complex(torch.randn(512, 37, 2, generator=g)).to(DEV)
    wave = ((torch.rand(2, 5000, generator=g) - 0.5) * 1.6).to(DEV)
    Z = torch.view_as_complex(torch.randn(512, frames, 2, generator=g)).to(DEV)
    M = Z.abs().contiguous()
    calls = [lambda: pv_ops.phase_vocoder(X, 11, 10),
             lambda: loud_ops.true_peak(wave),
             lambda: gl_ops.griffin_lim(M, Z.clone(), 2, 0.99),     # Z is rewritten in place
             lambda: pv_ops.phase_vocoder(X, 11, 10)]
    cache = {}
    monkeypatch.setattr(ops, "_ws_cache", cache)    # emptied; the buffers other tests left are back afterwards
    key = (0, torch.cuda.current_stream().cuda_stream)

    together, sizes = [], []
    for call in calls:
        together.append(call())
        assert list(cache) == [key]
        sizes.append(cache[key].numel())
    torch.cuda.synchronize()
    print(f"WORKSPACE: Griffin-Lim at {frames} frames asks for {gl_ops.griffin_lim_ws_bytes(frames, 2)} bytes; the buffer held {sizes}")
    assert sizes[0] == sizes[1] == FLOOR < gl_ops.griffin_lim_ws_bytes(frames, 2) <= sizes[2] == sizes[3]

    for i, call in enumerate(calls):
        cache.clear()
        alone = call()
        torch.cuda.synchronize()
        assert alone.dtype == together[i].dtype and torch.equal(alone, together[i]), f"call {i} differs from the same call alone"
        assert bool(torch.isfinite(torch.view_as_real(alone) if alone.is_complex() else alone).all())

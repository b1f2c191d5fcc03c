"""streams.new_stream on the GPU: a pool stream whose graph capture was invalidated refuses all work for the rest of the process, and
the helper never deals it out.  (The file sorts last on purpose: the stream it breaks stays broken until the process ends.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_new_stream_skips_a_stream_with_an_invalidated_capture():
    from musicgan_amd import streams
    dev = torch.device(DEV)
    caller = torch.cuda.current_stream(dev)
    broken = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        with torch.cuda.graph(graph, stream=broken, capture_error_mode="thread_local"):
            torch.cuda.synchronize()  # illegal during a capture: HIP invalidates it (what the stepper's eager fallback survives)
    torch.cuda.set_stream(caller)  # the failed exit leaves the capture stream current (train_step does the same)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError) as e:
        streams._probe(broken, dev)
    assert streams.is_capture_error(e.value), str(e.value)
    src = torch.arange(8, dtype=torch.float32, device=dev)
    for _ in range(40):  # more than the pool's 32: a plain torch.cuda.Stream() would have been the broken one at least once
        s = streams.new_stream(dev)
        assert s.cuda_stream != broken.cuda_stream
        s.wait_stream(caller)
        with torch.cuda.stream(s):
            out = src * 2
        s.synchronize()
        assert out.tolist() == [0.0, 2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0]

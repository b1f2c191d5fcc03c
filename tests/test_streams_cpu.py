"""streams.new_stream without a GPU: which errors make it take the next pool stream (the capture error alone) and when it gives up."""
import pytest

from musicgan_amd import streams

CAPTURE = "HIP error: operation failed due to a previous error during capture"


def _fake(monkeypatch, outcomes):
    """torch.cuda.Stream replaced by a counter, the probe by a list of outcomes (None: accepts work, else the error to raise)"""
    made, todo = [], list(outcomes)

    class Cuda:
        @staticmethod
        def Stream(device=None):
            made.append(len(made))
            return made[-1]

    class Torch:
        cuda = Cuda

    def probe(stream, device):
        err = todo.pop(0) if todo else None
        if err is not None:
            raise err
    monkeypatch.setattr(streams, "torch", Torch)
    monkeypatch.setattr(streams, "_probe", probe)
    return made


def test_the_capture_error_alone_moves_on_to_the_next_stream(monkeypatch):
    made = _fake(monkeypatch, [RuntimeError(CAPTURE), RuntimeError(CAPTURE), None])
    assert streams.new_stream("cuda:0") == 2 and made == [0, 1, 2]


def test_any_other_error_is_raised_at_once(monkeypatch):
    made = _fake(monkeypatch, [RuntimeError("HIP error: an illegal memory access was encountered"), None])
    with pytest.raises(RuntimeError, match="illegal memory access"):
        streams.new_stream("cuda:0")
    assert made == [0]
    made = _fake(monkeypatch, [ValueError(CAPTURE)])
    with pytest.raises(ValueError):
        streams.new_stream("cuda:0")


def test_a_pool_of_broken_streams_raises_the_capture_error(monkeypatch):
    made = _fake(monkeypatch, [RuntimeError(CAPTURE)] * 40)
    with pytest.raises(RuntimeError, match="previous error during capture"):
        streams.new_stream("cuda:0")
    assert len(made) == 33


def test_is_capture_error():
    assert streams.is_capture_error(RuntimeError(CAPTURE))
    assert streams.is_capture_error(RuntimeError("hipErrorStreamCaptureInvalidated"))
    assert not streams.is_capture_error(RuntimeError("out of memory")) and not streams.is_capture_error(KeyError(CAPTURE))

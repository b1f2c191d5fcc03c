"""Side streams that work.  `torch.cuda.Stream()` hands out the 32 streams of a per-device pool in turn, so two Stream objects made
far apart can be the same HIP stream -- and a stream on which a graph capture was invalidated (train_step falls back to eager updates
after one, and notes that the capture stream stays unusable) refuses every later operation with hipErrorStreamCaptureInvalidated
("operation failed due to a previous error during capture") for the rest of the process.  Every side stream of the package is made
by `new_stream`, which skips such a stream: it queues one one-element fill on the candidate, which a broken stream refuses at the
launch.  Any other error of that fill is raised as it is."""
from __future__ import annotations

import torch

_CAPTURE_ERRORS = ("previous error during capture", "StreamCaptureInvalidated")


def is_capture_error(e: BaseException) -> bool:
    """whether `e` is the runtime's refusal of a stream whose capture was invalidated"""
    return isinstance(e, RuntimeError) and any(s in str(e) for s in _CAPTURE_ERRORS)


def _probe(stream, device) -> None:
    with torch.cuda.stream(stream):
        torch.empty(1, dtype=torch.float32, device=device).zero_()


def new_stream(device) -> "torch.cuda.Stream":
    """a stream of torch's pool on `device` that accepts work; the capture error of the last candidate if all 32 refuse"""
    for attempt in range(33):  # the pool holds 32
        stream = torch.cuda.Stream(device=device)
        try:
            _probe(stream, device)
            return stream
        except RuntimeError as e:  # (torch.AcceleratorError is one)
            if not is_capture_error(e) or attempt == 32:
                raise

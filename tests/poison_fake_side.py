"""A second small ops module for tests/test_poison_cpu.py, standing beside tests/poison_fake_ops.py as the package's side modules
stand beside `musicgan_amd.ops`: it keeps no cache of its own and takes its scratch memory from the first module's `workspace`,
through the module attribute.  As there, the planted defect stays inside a buffer that tests/poison.py itself allocated."""
import torch

import poison_fake_ops as main


def _ws(x):
    return main.workspace(4 * x.numel(), x.device)


def total(x):
    """(sum x,) through the shared workspace, written before it is read"""
    ws = _ws(x)[:4 * x.numel()].view(torch.float32)
    ws.copy_(x.reshape(-1))
    out = torch.zeros((1,), dtype=torch.float32, device=x.device)
    out += ws.sum()
    return out


def read_unwritten_workspace(x):
    return x + _ws(x)[:4 * x.numel()].view(torch.float32).view(x.shape)


def write_past_workspace(x):
    buf = _ws(x).view(torch.float32)
    main._mark(main._at(buf, buf.numel()))   # one float past the payload of the shared buffer
    return total(x)

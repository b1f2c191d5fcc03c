"""CPU: the host side of the averaged generator weights -- FusedAdam(ema_decay=...) bookkeeping, the state-dict exchange with
torch.optim.Adam, Saver's `gen_ema_{k}.pt`, the `--ema-decay` option, and the build of the kernel (no launch: there is no GPU here)."""
import os
import re

import pytest
import torch

from musicgan_amd import _lib
from musicgan_amd.optim import FusedAdam


def _params(n=3):
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(4, i + 2, generator=g)) for i in range(n)]


def _with_state(opt):
    """what a first step leaves behind, without the launch"""
    for group in opt.param_groups:
        for p in group["params"]:
            opt._init_state(p)
    return opt


@pytest.mark.parametrize("decay", [-0.1, 1.0, 1.5, float("nan")])
def test_decay_outside_the_half_open_unit_interval_is_refused(decay):
    with pytest.raises(ValueError):
        FusedAdam(_params(), ema_decay=decay)
    from musicgan_amd import avg_ops
    with pytest.raises(ValueError):
        avg_ops.ema_weight(decay)


def test_ema_weight_is_one_minus_decay_rounded_once():
    import numpy as np
    from musicgan_amd import avg_ops
    for d in (0.0, 0.5, 0.99, 0.999, 0.9999, 1.0 - 2.0 ** -30):
        w = avg_ops.ema_weight(d)
        assert w == float(np.float32(1.0 - d)) and 0.0 < w <= 1.0
        assert np.float32(w) == w   # already a float32 value: the call rounds nothing more


def test_avg_ops_refuses_cpu_tensors_loudly():
    from musicgan_amd import avg_ops
    p, g, m, v, e = (torch.zeros(8) for _ in range(5))
    s = torch.zeros((), dtype=torch.int32)
    with pytest.raises(_lib.MusicGanHipError):
        avg_ops.adam_step_ema([p], [g], [m], [v], [s], [e], lr=1e-3, beta1=0.0, beta2=0.9, eps=1e-8, decay=0.999)
    with pytest.raises(ValueError):
        avg_ops.adam_step_ema([p], [g], [m], [v], [s], [], lr=1e-3, beta1=0.0, beta2=0.9, eps=1e-8, decay=0.999)
    ps = _params(1)
    ps[0].grad = torch.zeros_like(ps[0])
    with pytest.raises(_lib.MusicGanHipError):
        FusedAdam(ps, ema_decay=0.999).step()


def test_capture_signature_carries_the_decay_and_is_unchanged_without_it():
    ps = _params()
    plain = FusedAdam(ps, lr=1e-3, betas=(0.0, 0.9))
    off = FusedAdam(ps, lr=1e-3, betas=(0.0, 0.9), ema_decay=0.0)
    a = FusedAdam(ps, lr=1e-3, betas=(0.0, 0.9), ema_decay=0.999)
    b = FusedAdam(ps, lr=1e-3, betas=(0.0, 0.9), ema_decay=0.99)
    assert off.capture_signature() == plain.capture_signature()
    assert plain.capture_signature() == (0, 1.0, ((1e-3, (0.0, 0.9), 1e-8),))   # the form graphs were keyed on before
    assert len({plain.capture_signature(), a.capture_signature(), b.capture_signature()}) == 3


def test_average_starts_as_a_copy_with_the_rest_of_the_state():
    ps = _params()
    on, off = _with_state(FusedAdam(ps, ema_decay=0.999)), _with_state(FusedAdam(ps))
    for p in ps:
        assert "ema" not in off.state[p] and off.averaged(p) is p
        e = on.state[p]["ema"]
        assert e.dtype == torch.float32 and torch.equal(e, p.detach()) and e.data_ptr() != p.data_ptr()
        assert on.averaged(p) is e and not e.requires_grad
    late = torch.nn.Parameter(torch.ones(5))
    assert on.averaged(late) is late   # not (yet) a parameter of the optimizer


def test_state_dict_round_trips_with_torch_adam():
    ps = _params()
    on = _with_state(FusedAdam(ps, lr=1e-3, betas=(0.0, 0.9), ema_decay=0.999))
    off = _with_state(FusedAdam(ps, lr=1e-3, betas=(0.0, 0.9)))
    for p in ps:
        on.state[p]["ema"].mul_(0.5)     # something that is not the weights
    sd_on, sd_off = on.state_dict(), off.state_dict()
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq", "ema"} for s in sd_on["state"].values())
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd_off["state"].values())
    # -> torch.optim.Adam, extra key and all
    ref = torch.optim.Adam(ps, lr=1e-3, betas=(0.0, 0.9))
    ref.load_state_dict(sd_on)
    for p in ps:
        assert torch.equal(ref.state[p]["ema"], on.state[p]["ema"]) and torch.equal(ref.state[p]["exp_avg"], on.state[p]["exp_avg"])
        p.grad = torch.ones_like(p)
    # -> back from torch.optim.Adam's own format (no "ema"): the averages start as copies of the weights at load time
    plain = torch.optim.Adam(ps, lr=1e-3, betas=(0.0, 0.9))
    plain.step()
    back = FusedAdam(ps, lr=1e-3, betas=(0.0, 0.9), ema_decay=0.999)
    epoch = back.capture_signature()
    back.load_state_dict(plain.state_dict())
    assert back.capture_signature() != epoch
    for p in ps:
        assert torch.equal(back.state[p]["ema"], p.detach()) and back.state[p]["ema"].data_ptr() != p.data_ptr()
        assert float(back.state[p]["step"]) == 1.0 and back.state[p]["step"].device.type == "cpu"
    # -> averages restored where they were saved
    again = FusedAdam(ps, lr=1e-3, betas=(0.0, 0.9), ema_decay=0.999)
    again.load_state_dict(sd_on)
    for p in ps:
        assert torch.equal(again.state[p]["ema"], on.state[p]["ema"]) and again.state[p]["ema"].device == p.device
    # -> dropped when averaging is off
    dropped = FusedAdam(ps, lr=1e-3, betas=(0.0, 0.9))
    dropped.load_state_dict(sd_on)
    assert all("ema" not in dropped.state[p] for p in ps)
    assert all("ema" not in s for s in dropped.state_dict()["state"].values())


def test_averaged_state_dict_keeps_keys_and_order():
    from musicgan_amd.networks import Generator
    torch.manual_seed(0)
    gen = Generator(8)
    gen.next_layer()
    opt = FusedAdam(gen.parameters(), ema_decay=0.99)
    named = dict(gen.named_parameters())
    first = next(iter(named))
    for name, p in named.items():
        if name != first:                 # one parameter without a state, as one whose .grad stayed None
            opt._init_state(p)
            opt.state[p]["ema"].add_(1.0)
    sd, avg = gen.state_dict(), opt.averaged_state_dict(gen)
    assert list(avg.keys()) == list(sd.keys()) and len(sd) >= len(named) > 2
    for k in sd:
        assert avg[k].shape == sd[k].shape and avg[k].dtype == sd[k].dtype and not avg[k].requires_grad
        if k in named and k != first:
            assert torch.equal(avg[k], sd[k] + 1.0)
            assert avg[k].data_ptr() != opt.state[named[k]]["ema"].data_ptr()   # a clone: saving it cannot race the next step
        else:
            assert torch.equal(avg[k], sd[k])
    fresh = Generator(8)
    fresh.next_layer()
    fresh.load_state_dict(avg, strict=True)
    # averaging off: the module's own state dict
    plain = FusedAdam(gen.parameters()).averaged_state_dict(gen)
    assert list(plain.keys()) == list(sd.keys()) and all(torch.equal(plain[k], sd[k]) for k in sd)


def test_saver_writes_gen_ema_exactly_when_asked(tmp_path):
    from musicgan_amd.networks import Discriminator, Generator
    from musicgan_amd.utils import Saver
    torch.manual_seed(0)
    gen, disc = Generator(8), Discriminator(7)
    og, od = FusedAdam(gen.parameters(), ema_decay=0.5), FusedAdam(disc.parameters())
    for p in gen.parameters():
        og._init_state(p)
        og.state[p]["ema"].zero_()
    saver = Saver(str(tmp_path), save_every=2, rand_channels=8)
    saver._write_previews = lambda *a, **k: None    # previews run the generator: not here
    calls = []

    def ema():
        calls.append(1)
        return og.averaged_state_dict(gen)

    pt = lambda: sorted(f for f in os.listdir(tmp_path) if f.endswith(".pt"))  # noqa: E731
    assert saver.request_save(gen, disc, og, od, 1.0, gen_ema=ema) is False and pt() == [] and calls == []
    assert saver.request_save(gen, disc, og, od, 1.0, gen_ema=ema) is True and calls == [1]
    assert pt() == ["disc_0.pt", "gen_0.pt", "gen_ema_0.pt", "optim_disc_0.pt", "optim_gen_0.pt"]
    saver.request_save(gen, disc, og, od, 1.0)
    assert saver.request_save(gen, disc, og, od, 1.0, train_state=lambda: {"k": 1}) is True
    assert pt() == ["disc_0.pt", "disc_1.pt", "gen_0.pt", "gen_1.pt", "gen_ema_0.pt", "optim_disc_0.pt", "optim_disc_1.pt",
                    "optim_gen_0.pt", "optim_gen_1.pt", "train_state_1.pt"]
    raw, avg = torch.load(str(tmp_path / "gen_0.pt")), torch.load(str(tmp_path / "gen_ema_0.pt"))
    assert list(raw.keys()) == list(avg.keys())
    assert all(not bool(avg[k].any()) for k in avg) and any(bool(raw[k].any()) for k in raw)
    assert "ema" in next(iter(torch.load(str(tmp_path / "optim_gen_0.pt"))["state"].values()))


def test_ema_decay_option():
    from musicgan_amd.__main__ import _MODES, build_parser
    p = build_parser()
    a = p.parse_args(["train", "run0", "-o", "out", "-i", "data"])
    assert a.ema_decay == 0.0 and _MODES["train"][4](a) == {}          # off: train() is called as before
    a = p.parse_args(["train", "run0", "-o", "out", "-i", "data", "--ema-decay", "0.999"])
    assert a.ema_decay == 0.999 and _MODES["train"][4](a) == {"ema_decay": 0.999}
    assert _MODES["train"][3](a) == ("run0", "data", "out")
    with pytest.raises(SystemExit):
        p.parse_args(["train", "run0", "-o", "out", "-i", "data", "--ema-decay", "much"])
    import inspect
    from musicgan_amd.train import train
    assert inspect.signature(train).parameters["ema_decay"].default == 0.0


def test_record_layout_and_chunk_fit_the_argument_segment_of_the_plain_step():
    import ctypes
    from musicgan_amd._lib import AdamTensorDev, AdamTensorDevEma
    assert ctypes.sizeof(AdamTensorDev) == 48 and ctypes.sizeof(AdamTensorDevEma) == 56   # + one pointer
    assert AdamTensorDevEma.ema.offset == 48
    src = open(os.path.join(_lib._HERE, "csrc", "elementwise.hip")).read()
    plain = int(re.search(r"constexpr int ADAM_DEV_CHUNK = (\d+);", src).group(1))
    ema = int(re.search(r"constexpr int ADAM_DEV_EMA_CHUNK = (\d+);", src).group(1))
    assert ema * ctypes.sizeof(AdamTensorDevEma) <= plain * ctypes.sizeof(AdamTensorDev)
    assert "getenv" not in src[src.index("ADAM_DEV_CHUNK"):src.index("}  // namespace", src.index("ADAM_DEV_CHUNK"))]


def test_averaged_adam_kernel_uses_no_scratch_memory():
    from musicgan_amd import _build
    _build.build()
    usage = _build.resource_usage()
    for pat in (r"adam_dev_ema_k", r"adam_dev_k", r"adam_tick_k"):
        hits = {k: v for k, v in usage.items() if re.search(pat, k)}
        assert hits, f"no kernel matches {pat}"
        for name, u in hits.items():
            assert u.get("ScratchSize [bytes/lane]", 0) == 0, f"{name}: scratch memory; VGPRs {u.get('VGPRs')}"
            assert u.get("VGPRs", 0) > 0
    assert len([k for k in usage if re.search(r"adam_tick_k", k)]) == 2   # one instance per record type

"""Fused multi-tensor Adam on the HIP kernel `mg_adam_step_dev` -- one launch (+ a one-wave counter tick) per optimizer step.

Semantics and state layout are torch.optim.Adam's (amsgrad=False, weight_decay=0, maximize=False), which is what the
reference uses (/root/reference/music_gan/train.py:64-70,175,214,262-272): per-parameter `step`, `exp_avg`, `exp_avg_sq`;
parameters whose .grad is None are skipped (their step count does not advance); param groups added later start at step 0.
`state_dict()` is loadable by torch.optim.Adam and vice versa.

The step count the kernel reads lives in device memory (`step_dev`, int32) and the bias corrections are formed on the device,
so a captured HIP graph of the step stays valid from one replay to the next; `state["step"]` is the host mirror torch's format
wants (advanced here on every eager step, and by `note_replay()` after a graph replay).

`ema_decay=d` (0 < d < 1; 0, the default, is off and changes nothing) keeps an exponential running average of every parameter
in `state[p]["ema"]`: it starts as a copy of the parameter in front of the parameter's first update and moves by
ema += (p - ema) * (1 - d) after each one, inside the same launch (`mg_adam_step_dev_ema` through `avg_ops.adam_step_ema`).
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List

import torch

from . import _lib, avg_ops
from ._lib import AdamTensorDev, check


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, ema_decay: float = 0.0):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameters")
        if not 0 <= ema_decay < 1:
            raise ValueError(f"0 <= ema_decay < 1 expected, got {ema_decay!r}")
        self.ema_decay = float(ema_decay)  # 0: no averages are kept; one value for all groups, those added later included
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))
        self.grad_scale = 1.0  # multiplied into every gradient inside the kernel (data-parallel averaging)
        self._state_epoch = 0  # bumped whenever the state tensors are replaced (load_state_dict)

    def capture_signature(self) -> tuple:
        """Everything a captured HIP graph of `step()` has baked in besides the parameters themselves: the hyper-parameters travel
        as launch scalars and the moment / step-counter tensors by address.  ProGANStepper keys its graphs on this, so a changed
        `param_group['lr']` (a scheduler) or a `load_state_dict` leads to a fresh capture instead of being silently ignored."""
        sig = (self._state_epoch, float(self.grad_scale),
               tuple((float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"])) for g in self.param_groups))
        return sig + (self.ema_decay,) if self.ema_decay else sig

    def _init_state(self, p: torch.Tensor) -> dict:
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        if "step_dev" not in st:
            st["step_dev"] = torch.full((), int(st["step"]), dtype=torch.int32, device=p.device)
        if self.ema_decay and "ema" not in st:  # the average starts as a copy of the weights it has not seen move yet
            st["ema"] = p.detach().to(torch.float32, copy=True, memory_format=torch.contiguous_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            lr, eps = group["lr"], group["eps"]
            if self.ema_decay:
                self._step_group_ema(group)
                continue
            recs: List[AdamTensorDev] = []
            touched = []
            device = None
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise _lib.MusicGanHipError("FusedAdam needs parameters on a ROCm GPU (no CPU fallback)")
                g = p.grad
                if not g.is_contiguous():
                    g = g.contiguous()
                    p.grad = g
                st = self._init_state(p)
                st["step"] += 1
                recs.append(AdamTensorDev(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                          p.numel(), st["step_dev"].data_ptr()))
                touched.append(p)
                device = p.device
            if not recs:
                continue
            arr = (AdamTensorDev * len(recs))(*recs)  # host records; the library hands them to the kernel by value
            with torch.cuda.device(device):
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                check(lib.mg_adam_step_dev(ctypes.cast(arr, ctypes.c_void_p), len(recs), lr, beta1, beta2, eps,
                                           float(self.grad_scale), stream), "mg_adam_step_dev")
            for p in touched:  # the kernel wrote behind autograd's back: bump versions so packed-weight caches refresh
                torch.autograd.graph.increment_version(p)
        return loss

    def _step_group_ema(self, group: dict) -> None:
        """`step()` of one group with averaging on: the same bookkeeping, the launch that also moves the averages."""
        touched, states = [], []
        for p in group["params"]:
            if p.grad is None:
                continue
            if not p.is_cuda:
                raise _lib.MusicGanHipError("FusedAdam needs parameters on a ROCm GPU (no CPU fallback)")
            if not p.grad.is_contiguous():
                p.grad = p.grad.contiguous()
            st = self._init_state(p)
            st["step"] += 1
            touched.append(p)
            states.append(st)
        if not touched:
            return
        avg_ops.adam_step_ema([p.detach() for p in touched], [p.grad for p in touched], [st["exp_avg"] for st in states],
                              [st["exp_avg_sq"] for st in states], [st["step_dev"] for st in states],
                              [st["ema"] for st in states], lr=group["lr"], beta1=group["betas"][0], beta2=group["betas"][1],
                              eps=group["eps"], grad_scale=float(self.grad_scale), decay=self.ema_decay)
        for p in touched:
            torch.autograd.graph.increment_version(p)

    def averaged(self, p: torch.Tensor) -> torch.Tensor:
        """The running average of `p` where it has one, else `p` itself."""
        return self.state[p]["ema"] if p in self.state and "ema" in self.state[p] else p

    def averaged_state_dict(self, module: torch.nn.Module) -> dict:
        """`module.state_dict()` with every parameter that has an average replaced by it (a detached clone); same keys, same
        order, so the result loads wherever the module's own state dict does."""
        sd = module.state_dict()
        for name, p in module.named_parameters():
            if name in sd and self.averaged(p) is not p:
                sd[name] = self.averaged(p).detach().clone()
        return sd

    def note_replay(self, params: Iterable[torch.Tensor]) -> None:
        """A captured graph containing this optimizer's step over `params` was replayed: the device counters advanced by
        themselves, bring the host mirrors and the parameter versions along."""
        for p in params:
            self.state[p]["step"] += 1
            torch.autograd.graph.increment_version(p)

    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = {k: {kk: vv for kk, vv in v.items() if kk != "step_dev"} for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._state_epoch += 1  # new exp_avg / exp_avg_sq / step_dev tensors: graphs holding the old addresses are stale
        for p, st in self.state.items():
            st["step"] = torch.as_tensor(st["step"]).detach().to("cpu", torch.float32).reshape(())
            st["step_dev"] = torch.full((), int(st["step"]), dtype=torch.int32, device=p.device)
            if not self.ema_decay:
                st.pop("ema", None)  # averaging is off: a saved average would go stale
            elif "ema" in st:
                st["ema"] = st["ema"].detach().to(p.device, torch.float32).contiguous()
            else:
                self._init_state(p)  # a state without averages (torch.optim.Adam's): they start at the loaded weights

"""Exponential moving average of the weights over the flat parameter buffer (``utils/flat.py``).

``FlatEMA`` keeps ``e``, an fp32 copy of ``flat.data`` (alignment padding included), and
averages it after every optimizer step with ONE launch (``csrc/kernels/ema.hip``):

    e <- fmaf(d, e - p, p),   d = decay   or, under warm-up,   min(decay, (1 + t) / (10 + t))

with ``t`` the number of updates applied so far.  The step-count convention is the flat
optimizers' (``flat_optim.FlatOptimizer``): the host passes the number of ``update()`` calls
``k``, a launch that finds ``found_inf`` set leaves ``e`` untouched and bumps the EMA's own
device counter ``kskip``, and an applied one uses ``t = k - kskip`` -- a skipped optimizer
step is a skipped average, with no host sync.  ``d = 0`` makes ``e`` a bitwise copy of ``p``.

Evaluating with the averaged weights exchanges the *contents* of ``flat.data`` and ``e`` in
place (``swap`` / ``applied``): captured HIP graphs, the ResNet engine and the transformer's
bf16 shadow hold the addresses of the flat buffers, so the buffers stay where they are.  A swap
is a weight write like any other: the bf16 shadow is rewritten and the engine's packed conv
layouts are marked stale.

Averaged are the parameters (BatchNorm / LayerNorm scales and shifts included); running
statistics are buffers, already moving averages, and stay the model's own.  Single process and
DDP only (``check_ema_config``): the kernel is deterministic, so replicas stay bitwise equal.
The CPU / ``FDT_NATIVE=0`` path applies the same rule and skip semantics with torch ops.
"""
from __future__ import annotations

import contextlib

import torch

from ..ops import _native
from .flat_optim import _p, _slot_remap, _slot_table, _sp


def check_ema_config(ema_decay: float, fsdp: bool = False, sharded: bool = False):
    """Refuses an EMA of the weights under --fsdp and under sharded NGD (the CLIs call it when
    they parse their arguments, the trainers before they set anything up)."""
    if not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"--ema_decay must be in [0, 1), not {ema_decay}")
    if ema_decay > 0 and fsdp:
        raise ValueError("--ema_decay is not supported with --fsdp: a rank holds only a shard of the parameters, "
                         "and the evaluation swap would have to go through the unit gathers")
    if ema_decay > 0 and sharded:
        raise ValueError("--ema_decay is not supported with sharded NGD (ZeRO-2): a rank updates only the "
                         "parameters it owns, and the evaluation swap would have to go through the all-gather "
                         "(shard_ngd=False keeps whole parameters on every rank; so does any other optimizer)")


def ema_decay_at(decay: float, warmup: bool, t: int) -> float:
    """The ``d`` of the update after ``t`` applied ones, in fp32 as the kernel computes it."""
    d = torch.tensor(float(decay), dtype=torch.float32)
    if warmup:
        tt = torch.tensor(float(t), dtype=torch.float32)
        d = torch.minimum(d, (1.0 + tt) / (10.0 + tt))
    return float(d)


class FlatEMA:
    def __init__(self, flat, decay: float, warmup: bool = True):
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"EMA decay must be in [0, 1], not {decay}")
        if not hasattr(flat, "slots"):
            raise ValueError("FlatEMA needs whole parameter slots (a FlatParams buffer, not a shard view)")
        if flat.data.dtype != torch.float32:
            raise ValueError("FlatEMA averages fp32 master weights")
        self.flat = flat
        self.decay, self.warmup = float(decay), bool(warmup)
        self.e = flat.data.detach().clone()
        self.k = 0  # update() calls
        self.kskip = torch.zeros(1, device=flat.device, dtype=torch.int32)  # skipped on the device
        self.swapped = False  # flat.data currently holds the averaged weights
        self._native = flat.data.is_cuda and _native.enabled()

    # ------------------------------------------------------------------ update
    @torch.no_grad()
    def update(self, found_inf: torch.Tensor | None = None):
        if self.swapped:
            raise RuntimeError("FlatEMA.update() while the averaged weights are swapped in")
        flat = self.flat
        if self._native:
            _native.native().ema_update(flat.data.data_ptr(), self.e.data_ptr(), flat.numel, self.decay,
                                        int(self.warmup), self.k, self.kskip.data_ptr(), _p(found_inf), _sp())
        elif found_inf is not None and bool(found_inf.item() != 0):
            self.kskip += 1
        else:
            d = ema_decay_at(self.decay, self.warmup, self.applied_k)
            self.e.sub_(flat.data).mul_(d).add_(flat.data)  # p + d (e - p); d = 0: p, bit for bit
        self.k += 1

    @property
    def applied_k(self) -> int:
        """Applied updates so far (host view: synchronises with the device)."""
        return self.k - int(self.kskip.item())

    def decay_eff(self) -> float | None:
        """``d`` of the last applied update (host view: synchronises), None before the first."""
        t = self.applied_k
        return ema_decay_at(self.decay, self.warmup, t - 1) if t > 0 else None

    # ------------------------------------------------------------------ swap
    @torch.no_grad()
    def swap(self):
        """Exchange the contents of ``flat.data`` and ``e`` in place; the bf16 shadow follows and
        the engine's packed conv layouts are marked stale."""
        flat = self.flat
        if self._native:
            _native.native().ema_swap(flat.data.data_ptr(), self.e.data_ptr(), _p(flat.shadow), flat.numel, _sp())
            flat.invalidate_packed()
        else:
            # (chunked: no temporary of model size)
            n, step = flat.numel, 1 << 20
            for a in range(0, n, step):
                p, e = flat.data[a:a + step], self.e[a:a + step]
                t = p.clone()
                p.copy_(e)
                e.copy_(t)
            flat.refresh_shadow()  # (invalidates the packed layouts too)
        self.swapped = not self.swapped

    @contextlib.contextmanager
    def applied(self):
        """The averaged weights in place of the trained ones for the duration of the block."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # ------------------------------------------------------------------ state
    def state_dict(self):
        if self.swapped:
            raise RuntimeError("FlatEMA.state_dict() while the averaged weights are swapped in")
        return {"e": self.e.detach().clone().cpu(), "k": self.k, "kskip": self.kskip.detach().clone().cpu(),
                "decay": self.decay, "warmup": self.warmup, "numel": self.flat.numel,
                "slots": _slot_table(self.flat)}

    def load_state_dict(self, sd):
        if "slots" not in sd:
            raise ValueError("EMA state carries no slot table: its parameter order cannot be verified")
        remap = _slot_remap([tuple(s) for s in sd["slots"]], self.flat)
        e = remap(sd["e"])
        if e.numel() != self.flat.numel:
            raise ValueError("EMA state was saved for a different parameter layout")
        self.e.copy_(e.to(self.e.device))
        self.k = int(sd["k"])
        self.kskip.copy_(sd["kskip"].to(self.kskip.device))
        self.decay, self.warmup = float(sd["decay"]), bool(sd["warmup"])

    def model_state_dict(self, model):
        """The averaged weights as ``model``'s state_dict (compact CPU clones; buffers such as
        running statistics are the model's own)."""
        with self.applied():
            return {k: (v.detach().clone().cpu() if torch.is_tensor(v) else v) for k, v in model.state_dict().items()}

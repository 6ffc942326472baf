"""Recorded results of the reference implementation as a numerics oracle.

The reference (SuperbTUM/Faster-Distributed-Training) is not part of this repository, so
the tests compare against what its pure-torch modules (resnet.py, transformer.py,
ngd_optimizer.py) computed on fixed inputs: ``tests/golden/*.npz`` / ``*.json``, written
once by ``scripts/make_golden.py`` from a checkout of the reference.  Inputs that would
be too large to store (model weights) are regenerated here from a seed by ``fill_state``,
the same function the recording used.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SAMPLE = 512  # gradient elements recorded per parameter (all of them for smaller parameters)


def golden(name: str) -> dict:
    """``tests/golden/<name>.npz`` as a dict of torch tensors (missing file = test error)."""
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def golden_json(name: str):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def schema(sd) -> list:
    """[key, shape, dtype] of every state-dict entry, in order."""
    return [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()]


def fill_state(sd, seed: int) -> None:
    """Overwrite every floating-point entry of a state dict, in place and in key order, with
    seeded values of a trained-network-like scale (He-scaled weights, gains near 1, small
    biases and means, positive variances)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in sd.items():
            if not v.is_floating_point():
                continue
            if k.endswith("running_var"):
                t = 1.0 + 0.1 * torch.rand(v.shape, generator=g, dtype=torch.float64)
            elif v.dim() >= 2:
                t = torch.randn(v.shape, generator=g, dtype=torch.float64) * math.sqrt(2.0 / v[0].numel())
            elif k.endswith("weight"):
                t = 1.0 + 0.1 * torch.randn(v.shape, generator=g, dtype=torch.float64)
            else:
                t = 0.1 * torch.randn(v.shape, generator=g, dtype=torch.float64)
            v.copy_(t)


def resnet_batch(seed: int = 1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(4, 3, 32, 32, generator=g, dtype=torch.float64)
    y = torch.randint(0, 10, (4,), generator=g)
    return x, y


def sample_index(numel: int) -> torch.Tensor:
    """The recorded elements of a flattened gradient: all of a small one, else SAMPLE of them
    spread over the whole tensor by a multiplicative hash (no RNG involved)."""
    if numel <= SAMPLE:
        return torch.arange(numel)
    return (torch.arange(SAMPLE, dtype=torch.int64) * 2654435761 + 12345) % numel


def projection(numel: int) -> torch.Tensor:
    """Fixed dense direction (|w_i| <= 1) for a whole-tensor check of a sampled gradient."""
    return torch.cos(torch.arange(numel, dtype=torch.float64) * 0.7390851332 + 1.0)


def grad_record(grads) -> dict:
    """What is kept of a list of flattened fp64 gradients: sample, norm and projection."""
    return {"sample": torch.cat([g[sample_index(g.numel())] for g in grads]),
            "norm": torch.stack([g.norm() for g in grads]),
            "proj": torch.stack([g @ projection(g.numel()) for g in grads])}


def assert_grads_match(named_grads, rec, tol: float) -> None:
    """Every gradient against its record: the recorded elements to ``tol`` (relative L2, as
    the full-tensor comparison was), and norm and projection of the WHOLE tensor within what
    a relative L2 error of ``tol`` allows (|(a-b).w| <= |a-b| |w|, ||a|-|b|| <= |a-b|)."""
    off = 0
    for i, (n, g) in enumerate(named_grads):
        g = g.detach().reshape(-1).double()
        idx = sample_index(g.numel())
        want = rec["sample"][off:off + idx.numel()]
        off += idx.numel()
        assert ((g[idx] - want).norm() / want.norm()).item() < tol, n
        norm = rec["norm"][i].item()
        assert abs(g.norm().item() - norm) < tol * norm, n
        w = projection(g.numel())
        assert abs((g @ w).item() - rec["proj"][i].item()) < tol * norm * w.norm().item(), n
    assert off == rec["sample"].numel()

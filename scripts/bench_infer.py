#!/usr/bin/env python3
"""ResNet-50 eval-forward latency: batch statistics (the default eval path) against frozen
running statistics (``eval_stats="running"``, ops/resnet_fused.py resnet_frozen_forward), and
a batch-128 training step with FusedConvBN statistics tracking on against off.

    python scripts/bench_infer.py                       # batch 1, 128, 1024; eager and graph replay
                                                        # (batch_stats | running | running_graph)
    python scripts/bench_infer.py --batches 128 --no-train

The modes ALTERNATE inside one process: each round times every mode once (device events over
``--iters`` forwards after ``--warmup``), the figure of a mode is the median over ``--rounds``
rounds and its spread the (max - min) / median of those rounds.  One JSON line per batch size,
one for the training step; launch counts are the native entry-point calls of one forward."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def summarize(samples):
    med = statistics.median(samples)
    return {"median_ms": round(med, 4), "spread": round((max(samples) - min(samples)) / med, 4),
            "rounds": [round(s, 4) for s in samples]}


def count_launches(fn):
    """Native entry-point calls of one ``fn()`` (the engine's kernel launches), by name."""
    from faster_distributed_training_amd.ops import _native
    real = _native.native()
    calls = {}

    class Recording:
        def __getattr__(self, name):
            f = getattr(real, name)
            if not callable(f):
                return f

            def wrapped(*a, **kw):
                calls[name] = calls.get(name, 0) + 1
                return f(*a, **kw)
            return wrapped

    orig = _native.native
    _native.native = lambda: Recording()
    try:
        fn()
    finally:
        _native.native = orig
    return calls


def make_model(dev, graphs):
    from faster_distributed_training_amd.models import resnet as R
    torch.manual_seed(0)
    m = R.resnet50(10).to(dev)
    m.fast_path = True
    m.graph_engine = graphs
    return m


def bench_eval(dev, batch, a):
    from faster_distributed_training_amd.models import resnet as R
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, 32, 32, generator=g).to(dev)
    models = {}
    modes = [("batch_stats", "batch", False)]
    if hasattr(R, "enable_running_stats"):  # (a tree from before the frozen forward: the baseline alone)
        modes += [("running", "running", False), ("running_graph", "running", True)]
    for name, stats, graphs in modes:
        m = make_model(dev, graphs)
        if stats == "running":
            R.enable_running_stats(m)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                R.calibrate_running_stats(m, [torch.randn(max(batch, 32), 3, 32, 32, generator=g).to(dev)])
        m.eval()
        if stats == "running":
            m.eval_stats = stats
        models[name] = m

    def fwd(m):
        def run():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return m(x)
        return run

    fns = {k: fwd(m) for k, m in models.items()}
    launches = {k: count_launches(fns[k]) for k in ("batch_stats", "running") if k in fns}
    for f in fns.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():  # alternate the modes inside every round
            samples[k].append(timed(f, a.iters))
    rec = {"bench": "resnet50_eval_forward", "batch": batch, "iters": a.iters, "rounds": a.rounds}
    for k in fns:
        rec[k] = summarize(samples[k])
    rec["launches"] = {k: {"total": sum(v.values()), "conv": v.get("conv_igemm", 0) + v.get("conv_igemm_join", 0)}
                       for k, v in launches.items()}
    print(json.dumps(rec), flush=True)


def bench_train(dev, a, batch=128):
    from faster_distributed_training_amd.models import resnet as R
    from faster_distributed_training_amd.optim.flat_optim import MADGRAD
    from faster_distributed_training_amd.utils.flat import FlatParams
    g = torch.Generator().manual_seed(2)
    x = torch.randn(batch, 3, 32, 32, generator=g).to(dev)
    y = torch.randint(0, 10, (batch,), generator=g).to(dev)
    steps = {}
    variants = [("tracking_off", False)] + ([("tracking_on", True)] if hasattr(R, "enable_running_stats") else [])
    for name, track in variants:
        m = make_model(dev, True)
        if track:
            R.enable_running_stats(m)
        m.train()
        flat = FlatParams(m, device=dev)
        opt = MADGRAD(flat, lr=2e-7)

        def step(m=m, flat=flat, opt=opt):
            flat.grad.zero_()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = m(x)
            F.cross_entropy(out.float(), y).backward()
            opt.step()
        steps[name] = step
    for f in steps.values():
        for _ in range(max(a.warmup, 4)):
            f()
    torch.cuda.synchronize()
    samples = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, f in steps.items():
            samples[k].append(timed(f, a.iters))
    rec = {"bench": "resnet50_train_step", "batch": batch, "iters": a.iters, "rounds": a.rounds}
    for k in steps:
        rec[k] = summarize(samples[k])
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 128, 1024])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for b in a.batches:
        bench_eval(dev, b, a)
    if not a.no_train:
        bench_train(dev, a)


if __name__ == "__main__":
    main()

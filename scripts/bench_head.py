#!/usr/bin/env python3
"""The classifier head in isolation and inside the ResNet-50 step, fused (csrc/kernels/head.hip)
against the PyTorch ops it replaces (mean -> autocast F.linear -> autograd backward).

    python scripts/bench_head.py                     # kernels, training step, frozen forward
    python scripts/bench_head.py --only kernels      # or: train, frozen

kernels: head forward + backward under HIP-graph replay at K = 100 (the wide MFMA head) and
         K = 10 (the narrow head), C = 2048, HW = 16, N in {128, 1024}; also the forward alone
         (``fused_fwd`` / ``torch_fwd``: the inference head).
train:   ResNet-50 with 100 classes, one training step (graphs on) at batch 128 and 1024, the
         model's ``fused_head`` on against off (off = the head as eager PyTorch ops).
frozen:  its frozen (running-statistics) forward under graph replay at batch 1, 128 and 1024.

The modes ALTERNATE inside one process: each round times every mode once (device events over
``--iters`` calls after ``--warmup``); the figure of a mode is the median over ``--rounds`` rounds
and its spread the (max - min) / median of those rounds.  One JSON line per comparison."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

BF = torch.bfloat16


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
    return {"median_ms": round(med, 5), "spread": round((max(samples) - min(samples)) / med, 4),
            "rounds": [round(s, 5) for s in samples]}


def alternate(fns, a, rec):
    for f in fns.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():
            samples[k].append(timed(f, a.iters))
    for k in fns:
        rec[k] = summarize(samples[k])
    print(json.dumps(rec), flush=True)


def captured(fn):
    """``fn`` captured into one graph after a side-stream warm-up; returns its replay."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def bench_kernels(dev, a, N, K, C=2048, HW=16):
    from faster_distributed_training_amd.ops import _native
    nat = _native.native()
    gen = torch.Generator(device=dev).manual_seed(0)
    body = torch.randn(N, HW, C, device=dev, generator=gen).relu().to(BF)
    W = torch.randn(K, C, device=dev, generator=gen) * C ** -0.5
    b = torch.randn(K, device=dev, generator=gen)
    dl = torch.randn(N, K, device=dev, generator=gen).to(BF)
    pooled = torch.empty(N, C, device=dev, dtype=BF)
    logits = torch.empty(N, K, device=dev, dtype=BF)
    dpool = torch.empty(N, C, device=dev, dtype=BF)
    gW, gb = torch.zeros_like(W), torch.zeros_like(b)

    def fused():
        sp = _native.stream_ptr()
        nat.head_fwd(body.data_ptr(), W.data_ptr(), b.data_ptr(), pooled.data_ptr(), logits.data_ptr(), N, HW, C, K, sp)
        nat.head_bwd(dl.data_ptr(), W.data_ptr(), pooled.data_ptr(), dpool.data_ptr(), gW.data_ptr(), gb.data_ptr(),
                     N, HW, C, K, sp)

    tb = body.clone().requires_grad_(True)
    tW, tb_ = W.clone().requires_grad_(True), b.clone().requires_grad_(True)

    def torch_head():
        for t in (tb, tW, tb_):
            t.grad = None
        with torch.autocast("cuda", dtype=BF):
            out = F.linear(tb.mean(dim=1, dtype=torch.float32), tW, tb_)
        out.backward(dl)

    def fused_fwd():
        nat.head_fwd(body.data_ptr(), W.data_ptr(), b.data_ptr(), pooled.data_ptr(), logits.data_ptr(), N, HW, C, K,
                     _native.stream_ptr())

    def torch_fwd():  # (the inference head: no graph of the backward is kept)
        with torch.no_grad(), torch.autocast("cuda", dtype=BF):
            return F.linear(body.mean(dim=1, dtype=torch.float32), W, b)

    fns = {"fused": captured(fused), "torch": captured(torch_head), "fused_fwd": captured(fused_fwd),
           "torch_fwd": captured(torch_fwd)}
    a = argparse.Namespace(**{**vars(a), "iters": 10 * a.iters})  # (tens of microseconds per replay)
    alternate(fns, a, {"bench": "head_fwd_bwd_graph_replay", "N": N, "K": K, "C": C, "HW": HW, "iters": a.iters,
                       "rounds": a.rounds})


def r50_100(dev, fused):
    from faster_distributed_training_amd.models import resnet as R
    torch.manual_seed(0)
    m = R.resnet50(100).to(dev)
    m.fast_path = True
    m.graph_engine = True
    m.fused_head = fused
    return m


def bench_train(dev, a, batch):
    from faster_distributed_training_amd.optim.flat_optim import MADGRAD
    from faster_distributed_training_amd.utils.flat import FlatParams
    g = torch.Generator().manual_seed(2)
    x = torch.randn(batch, 3, 32, 32, generator=g).to(dev)
    y = torch.randint(0, 100, (batch,), generator=g).to(dev)
    steps, models = {}, {}
    for name, fused in (("fused_head", True), ("torch_head", False)):
        m = models[name] = r50_100(dev, fused)
        m.train()
        flat = FlatParams(m, device=dev)
        opt = MADGRAD(flat, lr=2e-7)

        def step(m=m, flat=flat, opt=opt):
            flat.grad.zero_()
            with torch.autocast("cuda", dtype=BF):
                out = m(x)
            F.cross_entropy(out.float(), y).backward()
            opt.step()
        steps[name] = step
    rec = {"bench": "resnet50_100class_train_step", "batch": batch, "iters": a.iters, "rounds": a.rounds}
    alternate(steps, a, rec)
    assert models["fused_head"]._plan.head_on and not models["torch_head"]._plan.head_on


def bench_frozen(dev, a, batch):
    from faster_distributed_training_amd.models import resnet as R
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, 32, 32, generator=g).to(dev)
    fns, models = {}, {}
    for name, fused in (("fused_head", True), ("torch_head", False)):
        m = models[name] = r50_100(dev, fused)
        R.enable_running_stats(m)
        with torch.autocast("cuda", dtype=BF):
            R.calibrate_running_stats(m, [torch.randn(max(batch, 32), 3, 32, 32, generator=g).to(dev)])
        m.eval()
        m.eval_stats = "running"

        def run(m=m):
            with torch.no_grad(), torch.autocast("cuda", dtype=BF):
                return m(x)
        fns[name] = run
    rec = {"bench": "resnet50_100class_frozen_forward_graph", "batch": batch, "iters": a.iters, "rounds": a.rounds}
    alternate(fns, a, rec)
    assert models["fused_head"]._plan.head_on and not models["torch_head"]._plan.head_on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["kernels", "train", "frozen"], default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.only in (None, "kernels"):
        for N in (128, 1024):
            for K in (100, 10):
                bench_kernels(dev, a, N, K)
    if a.only in (None, "train"):
        for b in (128, 1024):
            bench_train(dev, a, b)
    if a.only in (None, "frozen"):
        for b in (1, 128, 1024):
            bench_frozen(dev, a, b)


if __name__ == "__main__":
    main()

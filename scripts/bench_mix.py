#!/usr/bin/env python3
"""The mixing step and the loss kernel in isolation: CutMix against input mixup, the
label-smoothed cross entropy against the unsmoothed one (csrc/kernels/mixup.hip).

    python scripts/bench_mix.py                  # both comparisons
    python scripts/bench_mix.py --only mix       # or: loss

mix:   batch 1024 of 32 x 32 x 8 bf16 padded-NHWC images (the device CIFAR loader's layout):
       ``mixup_prep + mixup_fwd`` against ``cutmix_prep + cutmix_fwd`` (one box per batch and a
       box per sample, box extents of lambda = 0.5), each pair captured into one HIP graph.
       ``*_fwd`` rows time the mixing kernel alone, ``*_prep`` rows the one-workgroup draw.
       ``cutmix_fwd`` reads one source per pixel where ``mixup_fwd`` reads two.
loss:  ``mixup_ce_fwd`` against ``mixup_ce_smooth_fwd`` (eps 0.1) at (1024, 10) and (1024, 100),
       bf16 logits, per-sample lambda, fused meter on.

The variants ALTERNATE inside one process: each round times every variant once (device events
over ``--iters`` graph replays after ``--warmup``); the figure of a variant is the median over
``--rounds`` rounds and its spread the (max - min) / median of those rounds.  One JSON line per
comparison."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

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
    return {"median_us": round(1e3 * med, 3), "spread": round((max(samples) - min(samples)) / med, 4),
            "rounds_us": [round(1e3 * s, 3) for s in samples]}


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


def bench_mix(dev, a, B=1024, H=32, W=32, cp=8):
    from faster_distributed_training_amd.ops import _native
    nat = _native.native()
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.zeros(B, H, W, cp, device=dev, dtype=BF)
    x[..., :3] = torch.randn(B, H, W, 3, device=dev, generator=gen).to(BF)
    out = torch.empty_like(x)
    y = torch.randint(0, 100, (B,), device=dev, generator=gen)
    # (valid before any prep has run: the mixing kernels index x with perm)
    perm = torch.arange(B, device=dev, dtype=torch.int32)
    yb = torch.zeros(B, device=dev, dtype=torch.int64)
    lv = torch.full((B,), 0.5, device=dev, dtype=torch.float32)
    box = torch.zeros(B, 4, device=dev, dtype=torch.int32)
    inner, seed = H * W * cp, 1234567
    bh, bw = int(H * 0.5 ** 0.5), int(W * 0.5 ** 0.5)  # lambda = 0.5

    def mixup_fwd():
        nat.mixup_fwd(x.data_ptr(), perm.data_ptr(), lv.data_ptr(), out.data_ptr(), B, inner, 1, _native.stream_ptr())

    def cutmix_fwd():
        nat.cutmix_fwd(x.data_ptr(), perm.data_ptr(), box.data_ptr(), out.data_ptr(), B, inner, H, W, cp, 1,
                       _native.stream_ptr())

    def mixup_prep():
        nat.mixup_prep(y.data_ptr(), B, 0.5, seed, perm.data_ptr(), yb.data_ptr(), lv.data_ptr(), _native.stream_ptr())

    def cutmix_prep(per_sample=1):
        nat.cutmix_prep(y.data_ptr(), B, H, W, bh, bw, per_sample, seed, perm.data_ptr(), yb.data_ptr(),
                        box.data_ptr(), lv.data_ptr(), _native.stream_ptr())

    def mixup():
        mixup_prep()
        mixup_fwd()

    def cutmix(per_sample):
        def run():
            cutmix_prep(per_sample)
            cutmix_fwd()
        return run

    fns = {"mixup": captured(mixup), "cutmix_batch_box": captured(cutmix(0)), "cutmix_sample_box": captured(cutmix(1))}
    # the mixing kernels alone, on the permutation / boxes the last prep left (a box per sample)
    fns["mixup_fwd"] = captured(mixup_fwd)
    fns["cutmix_fwd"] = captured(cutmix_fwd)
    # and the two one-workgroup draws alone
    fns["mixup_prep"] = captured(mixup_prep)
    fns["cutmix_prep"] = captured(cutmix_prep)
    alternate(fns, a, {"bench": "mix_prep_fwd_graph_replay", "B": B, "H": H, "W": W, "cp": cp, "dtype": "bf16",
                       "box": [bh, bw], "bytes_out": x.numel() * 2, "iters": a.iters, "rounds": a.rounds})


def bench_loss(dev, a, B, C, eps=0.1):
    from faster_distributed_training_amd.ops import _native
    nat = _native.native()
    gen = torch.Generator(device=dev).manual_seed(1)
    logits = torch.randn(B, C, device=dev, generator=gen).to(BF)
    ya = torch.randint(0, C, (B,), device=dev, generator=gen)
    yb = torch.randint(0, C, (B,), device=dev, generator=gen)
    lv = torch.rand(B, device=dev, generator=gen)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    glog = torch.empty_like(logits)
    dlam = torch.empty(B, device=dev, dtype=torch.float32)
    meter = torch.zeros(3, device=dev, dtype=torch.float32)
    args = (logits.data_ptr(), ya.data_ptr(), yb.data_ptr(), lv.data_ptr(), 0.0, loss.data_ptr(), glog.data_ptr(),
            dlam.data_ptr(), meter.data_ptr(), B, C, 1, 1)

    def plain():
        nat.mixup_ce_fwd(*args, _native.stream_ptr())

    def smooth():
        nat.mixup_ce_smooth_fwd(*args, eps, _native.stream_ptr())

    alternate({"unsmoothed": captured(plain), "smoothed": captured(smooth)}, a,
              {"bench": "mixup_ce_graph_replay", "B": B, "C": C, "eps": eps, "dtype": "bf16", "iters": a.iters,
               "rounds": a.rounds})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["mix", "loss"], default=None)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.only in (None, "mix"):
        bench_mix(dev, a)
    if a.only in (None, "loss"):
        for C in (10, 100):
            bench_loss(dev, a, 1024, C)


if __name__ == "__main__":
    main()

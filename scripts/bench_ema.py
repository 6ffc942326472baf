#!/usr/bin/env python3
"""Cost of the weight EMA (csrc/kernels/ema.hip) next to the flat SGD step, on the real ResNet-50
flat buffer, and what it adds to a training step.

Kernel level (default).  Graph-free eager launches, timed with device events over ``--iters``
consecutive launches after ``--warmup``, the variants alternating ``--rounds`` times in one
process (median and range over the rounds):

    sgd         one sgd_step launch (momentum 0.9): the flat optimizer kernel the EMA follows
    ema_update  one ema_update launch (warm-up schedule on, device skip flag passed)
    ema_swap    one ema_swap launch (an even number per window: the weights end where they were)

Bytes are counted from the rule, in fp32 words per flat element -- every buffer a launch reads or
writes once (the ResNet buffer has no bf16 shadow): sgd reads p g buf and writes p buf g (6),
ema_update reads p e and writes e (3), ema_swap reads and writes both (4).

``--step-ab``.  The ResNet trainer's step time with ``ema_decay`` 0.999 and 0 (ResNet-50, synthetic
data, MADGRAD, bf16, HIP graphs: the benchmark's configuration) at each ``--bs``: both trainers
live in one process, windows of ``--steps`` steps alternate off / on ``--rounds`` times, each
window between device synchronisations on the host clock.

    python scripts/bench_ema.py                         > profiles/ema/bench_ema_kernels.txt
    python scripts/bench_ema.py --step-ab --bs 1024 128 > profiles/ema/bench_ema_step.txt

Needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

WORDS = {"sgd": 6, "ema_update": 3, "ema_swap": 4}


def time_launches(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per launch


def kernels(a, dev):
    from faster_distributed_training_amd.models.resnet import resnet50
    from faster_distributed_training_amd.optim import flat_optim as O
    from faster_distributed_training_amd.optim.ema import FlatEMA
    from faster_distributed_training_amd.utils.flat import FlatParams
    torch.manual_seed(0)
    flat = FlatParams(resnet50(10).to(dev), device=dev)  # (as the trainer builds it: no bf16 shadow)
    flat.grad.normal_(generator=torch.Generator(device=dev).manual_seed(1))
    flat.grad.mul_(1e-3)
    sgd = O.SGD(flat, lr=1e-7, momentum=0.9, weight_decay=5e-4)  # (a step costs the same at any rate)
    ema = FlatEMA(flat, 0.999, warmup=True)
    found = torch.zeros(1, dtype=torch.int32, device=dev)
    fns = {"sgd": sgd.step, "ema_update": lambda: ema.update(found_inf=found), "ema_swap": ema.swap}
    assert ema._native and sgd._native, "the HIP kernels are what is measured"
    for fn in fns.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            times[k].append(time_launches(fn, a.iters))
    assert not ema.swapped and torch.isfinite(flat.data).all().item() and torch.isfinite(ema.e).all().item()
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = ["| kernel | elements | words/elem | MB/launch | us/launch (median, min-max) | TB/s | x sgd time | x sgd rate |",
             "|---|---|---|---|---|---|---|---|"]
    for k in fns:
        mb = WORDS[k] * 4 * flat.numel / 1e6
        rate, base = mb / med[k], WORDS["sgd"] * 4 * flat.numel / 1e6 / med["sgd"]
        print(json.dumps(dict(kernel=k, elements=flat.numel, words_per_elem=WORDS[k], mb_per_launch=mb,
                              us_median=med[k], us_min=min(times[k]), us_max=max(times[k]), tb_per_s=rate,
                              vs_sgd_time=med[k] / med["sgd"], vs_sgd_rate=rate / base, iters=a.iters,
                              rounds=a.rounds)), flush=True)
        lines.append(f"| {k} | {flat.numel} | {WORDS[k]} | {mb:.1f} | {med[k]:.1f} ({min(times[k]):.1f}-{max(times[k]):.1f}) "
                     f"| {rate:.2f} | {med[k] / med['sgd']:.2f} | {rate / base:.2f} |")
    print("\n".join(lines) + "\n", flush=True)


def step_ab(a, dev):
    from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig, ResNetTrainer
    lines = ["| batch | ema off ms/step (median, min-max) | ema on ms/step (median, min-max) | on - off us |", "|---|---|---|---|"]
    for bs in a.bs:
        runs = {}
        for name, decay in (("off", 0.0), ("on", 0.999)):
            tr = ResNetTrainer(ResNetConfig(arch="resnet50", bs=bs, synthetic=True, eval=False, plot=False, lr=2e-7,
                                            optimizer="madgrad", ema_decay=decay))
            assert (tr.ema is not None) == (decay > 0)

            def batches(tr=tr):
                while True:
                    for b in tr.train_loader:
                        yield b
            tr.model.train()
            runs[name] = (tr, batches())
        times = {k: [] for k in runs}
        for k, (tr, it) in runs.items():  # (the engine captures its graphs on the second step)
            for _ in range(max(a.warmup_steps, 3)):
                tr.train_step(*next(it))
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, (tr, it) in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    tr.train_step(*next(it))
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps(dict(batch=bs, steps=a.steps, rounds=a.rounds, off_ms=times["off"], on_ms=times["on"],
                              off_median_ms=med["off"], on_median_ms=med["on"],
                              delta_us=(med["on"] - med["off"]) * 1e3)), flush=True)
        lines.append(f"| {bs} | {med['off']:.3f} ({min(times['off']):.3f}-{max(times['off']):.3f}) | {med['on']:.3f} "
                     f"({min(times['on']):.3f}-{max(times['on']):.3f}) | {(med['on'] - med['off']) * 1e3:+.0f} |")
        del runs
        torch.cuda.empty_cache()
    print("\n".join(lines) + "\n", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100, help="launches per timed window (even: swaps pair up)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-ab", action="store_true", help="the trainer's step time with the EMA on and off instead")
    ap.add_argument("--bs", type=int, nargs="+", default=[1024, 128])
    ap.add_argument("--steps", type=int, default=30, help="--step-ab: steps per timed window")
    ap.add_argument("--warmup-steps", type=int, default=8)
    a = ap.parse_args()
    if a.iters < 50 or a.iters % 2 or a.warmup % 2:
        ap.error("--iters must be even and >= 50, --warmup even")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    (step_ab if a.step_ab else kernels)(a, dev)


if __name__ == "__main__":
    main()

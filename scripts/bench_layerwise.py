#!/usr/bin/env python3
"""Cost of the layer-wise optimizers (LARS / LAMB, csrc/kernels/optim_layerwise.hip) next to the
flat steps they extend, on the real ResNet-50 and transformer flat layouts.

Per layout, timed with device events over ``--iters`` steps after ``--warmup``, the variants
alternating ``--rounds`` times in one process (median and range over the rounds reported):

    sgd     one sgd_step launch (momentum 0.9)
    lars    slot_sumsq + slot_finalize + lars_apply
    adamw   one adam_step launch
    lamb    lamb_moments + slot_finalize + lamb_apply
    torch   the per-tensor PyTorch formulation of LARS: torch._foreach_norm of the parameters and
            of the gradients, then a foreach update (no host sync; what the flat design avoids)

Bytes are counted from the rule, in fp32 words per flat element (the bf16 shadow, where the
layout has one, is half a word): every buffer a launch reads or writes once.  Needs a GPU.
The steps zero the gradient, and it is refreshed once per timed window, outside it: all but the
first step of a window run on an all-zero gradient (LARS then takes q = 1).  The kernels' memory
traffic does not depend on the values.

    python scripts/bench_layerwise.py > profiles/lars/bench_layerwise.txt   # JSON lines, then the table
    python scripts/bench_layerwise.py --out table.md                        # the table alone, too
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from faster_distributed_training_amd.optim import flat_optim as O  # noqa: E402
from faster_distributed_training_amd.utils.flat import FlatParams  # noqa: E402


def layouts(device):
    from faster_distributed_training_amd.models.resnet import resnet50
    from faster_distributed_training_amd.models.transformer import Transformer
    torch.manual_seed(0)
    # (as the trainers build them: the ResNet buffer has no bf16 shadow, the transformer's has)
    yield "resnet50", FlatParams(resnet50(10).to(device), device=device), False
    tr = Transformer(4, 30522, n_layers=6, h=8, d_model=512, d_ff=1024, d_hidden=1024, maxlen=512)
    yield "transformer", FlatParams(tr.to(device), device=device, with_shadow=True), True


def words(kind, shadow):
    """fp32 words per element read + written by one step (g is zeroed by the step)."""
    sh = 0.5 if shadow else 0.0
    return {
        "sgd": 3 + 3 + sh,                 # read p g buf; write p buf g
        "lars": 2 + 3 + 3 + sh,            # + the reduction's read of p and g
        "adamw": 4 + 4 + sh,               # read p g m v; write p m v g
        "lamb": (4 + 2) + (3 + 2 + sh),    # pass A: read p g m v, write m v; apply: read p m v, write p g
        # norms 2; g *= q 2; g += wd q p 3; buf *= mom 2; buf += g 3; p -= lr buf 3; shadow cast 1 + sh
        "torch": 2 + 2 + 3 + 2 + 3 + 3 + ((1 + sh) if shadow else 0),
    }[kind]


def foreach_lars(flat, bufs, lr=1e-7, momentum=0.9, wd=5e-4, eta=1e-3, eps=1e-8):
    ps = [s.param.data for s in flat.slots]
    gs = [s.param.grad for s in flat.slots]
    adapted = torch.tensor([float(len(s.shape) > 1) for s in flat.slots], device=flat.device)

    def step():
        wn = torch.stack(torch._foreach_norm(ps))
        gn = torch.stack(torch._foreach_norm(gs))
        q = torch.where((adapted > 0) & (wn > 0) & (gn > 0), eta * wn / (gn + wd * wn + eps), torch.ones_like(wn))
        qs = list(q.unbind())
        torch._foreach_mul_(gs, qs)
        torch._foreach_addcmul_(gs, ps, list((q * wd * adapted).unbind()))
        torch._foreach_mul_(bufs, momentum)
        torch._foreach_add_(bufs, gs)
        torch._foreach_add_(ps, bufs, alpha=-lr)
        if flat.shadow is not None:
            flat.shadow.copy_(flat.data)
    return step


def variants(flat):
    lr = 1e-7  # (a step costs the same at any rate; the weights stay where they are)
    sgd = O.SGD(flat, lr=lr, momentum=0.9, weight_decay=5e-4)
    lars = O.LARS(flat, lr=lr, momentum=0.9, weight_decay=5e-4)
    adamw = O.Adam(flat, lr=lr, weight_decay=0.01, adamw=True)
    lamb = O.LAMB(flat, lr=lr, weight_decay=0.01)
    bufs = [torch.zeros_like(s.param.data) for s in flat.slots]
    return {"sgd": sgd.step, "lars": lars.step, "adamw": adamw.step, "lamb": lamb.step,
            "torch": foreach_lars(flat, bufs, lr=lr)}


def time_steps(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the markdown table here")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error("--iters must be >= 50")
    if not torch.cuda.is_available():
        raise SystemExit("bench_layerwise.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    lines = ["| layout | elements | variant | launches | words/elem | MB/step | us/step (median, min-max) | TB/s | x base |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, flat, shadow in layouts(dev):
        flat.grad.normal_(generator=torch.Generator(device=dev).manual_seed(1))
        flat.grad.mul_(1e-3)
        steps = variants(flat)
        times = {k: [] for k in steps}
        for k, st in steps.items():
            for _ in range(a.warmup):
                flat.grad.add_(1e-6)  # (the steps zero the gradient: keep it alive, outside the window)
                st()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, st in steps.items():
                flat.grad.add_(1e-6)
                torch.cuda.synchronize()
                times[k].append(time_steps(st, a.iters))
        assert torch.isfinite(flat.data).all().item()
        med = {k: statistics.median(v) for k, v in times.items()}
        nl = {"sgd": 1, "lars": 3, "adamw": 1, "lamb": 3, "torch": "~%d" % (7 * len(flat.slots))}
        for k in steps:
            w = words(k, shadow)
            mb = w * 4 * flat.numel / 1e6
            base = med["adamw"] if k == "lamb" else med["sgd"]
            rec = dict(layout=name, elements=flat.numel, slots=len(flat.slots), variant=k, words_per_elem=w,
                       mb_per_step=mb, us_median=med[k], us_min=min(times[k]), us_max=max(times[k]),
                       tb_per_s=mb / med[k], vs_base=med[k] / base, iters=a.iters, rounds=a.rounds)
            print(json.dumps(rec), flush=True)
            lines.append(f"| {name} | {flat.numel} | {k} | {nl[k]} | {w:g} | {mb:.1f} | {med[k]:.1f} "
                         f"({min(times[k]):.1f}-{max(times[k]):.1f}) | {mb / med[k]:.2f} | {med[k] / base:.2f} |")
    table = "\n".join(lines) + "\n"
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table)


if __name__ == "__main__":
    main()

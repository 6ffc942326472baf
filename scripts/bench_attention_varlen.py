#!/usr/bin/env python3
"""Padded against packed attention on AG-News-shaped lengths (MI355X).

Arms, alternated trip by trip inside one process, times from device events:
  * kernels: dense ``attention_packed`` on (B, 128, 3, 8, 64) with the trailing key mask against
    ``attention_varlen_packed`` on the same tokens packed, forward + backward, p = 0.1,
    at B = 256 and B = 32;
  * model: one eager training forward + backward of the 6-layer Transformer under bf16
    autocast, padded (B, 128) with mask against ``pack_tokens`` + the packed forward, B = 256.
Prints a Markdown table (median, min, max over the trips) and writes it to --out.

    python scripts/bench_attention_varlen.py --out /tmp/attention_varlen.md
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from faster_distributed_training_amd.data.agnews import VOCAB_SIZE, synthetic_agnews  # noqa: E402
from faster_distributed_training_amd.models.transformer import Transformer, pack_tokens  # noqa: E402
from faster_distributed_training_amd.ops import attention_native as an  # noqa: E402

L, H, P = 128, 8, 0.1


def time_arms(arms, trips, inner):
    """{name: [ms per call]}: ``trips`` rounds, each timing ``inner`` calls of every arm in turn."""
    out = {k: [] for k in arms}
    for k, f in arms.items():  # warm-up of every shape
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(trips):
        for k, f in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / inner)
    return out


def row(label, ts):
    return f"| {label} | {statistics.median(ts):.3f} | {min(ts):.3f} | {max(ts):.3f} |"


def kernel_arms(B, dev):
    lens = torch.from_numpy(synthetic_agnews(B, seed=1, max_len=L).lengths).clamp(max=L)
    g = torch.Generator().manual_seed(0)
    dense = torch.randn(B, L, 3, H, 64, generator=g).to(dev, torch.bfloat16).requires_grad_()
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(dev, torch.uint8)
    keep = mask.bool()
    packed = dense.detach()[keep].clone().requires_grad_()  # (T, 3, H, 64)
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = lens.cumsum(0)
    cu = cu.to(dev)
    go_d = torch.randn(B, L, H, 64, generator=g).to(dev, torch.bfloat16)
    go_p = go_d[keep].clone()
    max_len = int(lens.max())

    def run_dense():
        an.attention_packed(dense, mask, P).backward(go_d)
        dense.grad = None

    def run_packed():
        an.attention_varlen_packed(packed, cu, max_len, P).backward(go_p)
        packed.grad = None

    note = f"B = {B}: {int(lens.sum())} real of {B * L} padded tokens, longest {max_len}"
    return {f"dense attention_packed B={B}": run_dense, f"attention_varlen_packed B={B}": run_packed}, note


def model_arms(B, dev):
    store = synthetic_agnews(B, seed=1, max_len=L)
    lens = torch.from_numpy(store.lengths).clamp(max=L)
    torch.manual_seed(0)
    model = Transformer(4, VOCAB_SIZE, maxlen=512).to(dev).train()
    ids = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        n = int(lens[b])
        ids[b, :n] = torch.from_numpy(store.tokens[store.offsets[b]:store.offsets[b] + n].astype("int64"))
    ids = ids.to(dev)
    types = torch.zeros_like(ids)
    index = torch.arange(512, device=dev)
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(dev, torch.uint8).view(B, 1, 1, L)
    pids, ptypes, cu, max_len = pack_tokens(ids, types, lens, multiple=128)

    def step(*args, **kw):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits, _, _ = model(*args, **kw)
        logits.float().sum().backward()
        model.zero_grad(set_to_none=True)

    return {f"model padded B={B}": lambda: step(ids, types, index, mask),
            f"model packed B={B}": lambda: step(pids, ptypes, index, cu_seqlens=cu, max_len=max_len)}, \
        f"model: 6 layers, T = {pids.size(1)} packed rows against {B * L} padded"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trips", type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: a CPU timing says nothing about these kernels")
    dev = torch.device("cuda", 0)
    lines = ["| arm (forward + backward) | median ms | min ms | max ms |", "|---|---|---|---|"]
    notes = []
    for arms, note, inner in (kernel_arms(256, dev) + (20,), kernel_arms(32, dev) + (50,), model_arms(256, dev) + (3,)):
        notes.append(note)
        for k, ts in time_arms(arms, a.trips, inner).items():
            lines.append(row(k, ts))
    text = "\n".join(lines + [""] + [f"- {n}" for n in notes]) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

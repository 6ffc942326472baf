#!/usr/bin/env python3
"""Forward and data-gradient GEMM of the linear layers on MI355X, per call under graph replay:
csrc/kernels/linear_gemm.hip against the library call it replaces (F.linear with bias for nt,
g2 @ wc for nn), in alternating windows.

    python scripts/bench_linear_gemm.py [--tokens 4096 8192 32768 65536]

One line per (kind, M, N, K): median (min, max) us of each side and the verdict ("faster" / "slower":
the min-max ranges do not overlap).  The outputs are compared first (relative Frobenius difference).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        fn()
        with torch.cuda.graph(gr, stream=st):
            fn()
    torch.cuda.synchronize()
    return gr


def window(gr, replays):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        gr.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / replays * 1e3  # us


def alternating(fns, replays=200, repeats=7):
    """us per call of each fn: (median, min, max) over `repeats` windows taken in turns."""
    grs = [graph_of(f) for f in fns]
    for g in grs:
        window(g, replays)
    ts = [[] for _ in grs]
    for _ in range(repeats):
        for i, g in enumerate(grs):
            ts[i].append(window(g, replays))
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[4096, 8192, 32768, 65536])
    a = ap.parse_args()
    from faster_distributed_training_amd.ops import linear as L
    dev = torch.device("cuda")
    for M in a.tokens:
        for N, K in [(512, 512), (1536, 512), (1024, 512), (512, 1024)]:
            for kind in ("nt", "nn"):
                x = torch.randn(M, K, device=dev).to(torch.bfloat16)
                w = (torch.randn((N, K) if kind == "nt" else (K, N), device=dev) / K ** 0.5).to(torch.bfloat16)
                b = torch.randn(N, device=dev).to(torch.bfloat16) if kind == "nt" else None
                lib = (lambda: F.linear(x, w, b)) if kind == "nt" else (lambda: x @ w)
                hip = lambda: L.gemm(x, w, b, kind)
                ref = lib().double()
                diff = ((hip().double() - ref).norm() / ref.norm()).item()
                (tl, tl0, tl1), (th, th0, th1) = alternating([lib, hip])
                verdict = "faster" if th1 < tl0 else "slower" if th0 > tl1 else "inside the spread"
                print(json.dumps({"kind": kind, "M": M, "N": N, "K": K, "library_us": [round(v, 1) for v in (tl, tl0, tl1)],
                                  "hip_us": [round(v, 1) for v in (th, th0, th1)],
                                  "hip_tflops": round(2.0 * M * N * K / th / 1e6, 1), "rel_diff": float(f"{diff:.2e}"),
                                  "verdict": verdict}), flush=True)


if __name__ == "__main__":
    main()

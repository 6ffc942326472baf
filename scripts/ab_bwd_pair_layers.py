#!/usr/bin/env python3
"""Per-layer A/B for the fused backward of the expanding 1x1 convolutions (conv_bwd_pair): the
two-launch path (conv_dgrad + conv_wgrad from the tuned table) against the fused launch, for the
ACTBWD + ReLU variant (conv3 of a bottleneck block) and the STORE variant (the expanding shortcut),
HIP-graph replay (roofline_layers.timeit).  One-pass byte bound: g + y + x read, dX written, at
6.3 TB/s.  python scripts/ab_bwd_pair_layers.py BATCH [OUT.json] [WGS ...]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch
from roofline_layers import timeit
from faster_distributed_training_amd.ops import conv_igemm as ci

dev = torch.device("cuda")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
out_path = sys.argv[2] if len(sys.argv) > 2 else f"ab_bwd_pair_layers_{N}.json"
WGS = [int(v) for v in sys.argv[3:]] or [ci.BWD_PAIR_WGS]
LAYERS = [(32, 64, 256)]
HBM_TBS = 6.3
rows = []

for (H, cin, cout) in LAYERS:
    shp = ci.ConvShape(cin, cout, 1, 1, 0)
    torch.manual_seed(0)
    w = torch.randn(cout, cin, 1, 1, device=dev) / cin ** 0.5
    _, wd = ci.alloc_packed(shp, dev, fwd=False)
    ci.pack_weights([(w, None, wd, shp)])
    mk = lambda c: torch.randn(N, H, H, c, device=dev).to(torch.bfloat16)
    g, y, x = mk(cout), mk(cout), mk(cin)
    al, be = torch.randn(cout, device=dev) * 0.1, torch.randn(cout, device=dev) * 0.1
    gs = torch.rand(cout, device=dev) + 0.5
    s, t = torch.rand(cin, device=dev) + 0.5, torch.randn(cin, device=dev) * 0.3
    dx = torch.empty_like(x)
    dw = torch.zeros(cout, cin, 1, 1, device=dev)
    M = N * H * H
    part = ci.stat_slots(2, cin, dev, M)
    bound = (2 * M * cout * 2 + 2 * M * cin * 2) / (HBM_TBS * 1e12) * 1e6
    for name, epi, act, xs, xt in (("actbwd", ci.EPI_ACTBWD, 1, s, t), ("store", ci.EPI_STORE, 0, None, None)):
        kw = dict(ex=x, es=s, et=t, act=1, part=part) if epi == ci.EPI_ACTBWD else {}

        def dgrad():
            ci.conv_dgrad(g, y, al, be, wd, shp, tuple(x.shape), epi=epi, out=dx, gs=gs, **kw)

        def wgrad():
            ci.conv_wgrad(g, y, al, be, x, shp, dw, xs, xt, act, accumulate=True, gs=gs)

        def pair():
            dgrad()
            wgrad()

        def fused_of(wgs):
            return lambda: ci.conv_bwd_pair(g, y, al, be, wd, x, shp, dw, epi=epi, xs=xs, xt=xt, es=xs, et=xt,
                                            act=act, part=part if epi == ci.EPI_ACTBWD else None, gs=gs,
                                            accumulate=True, wgs=wgs, out=dx)

        us = lambda fn: min(timeit(fn) for _ in range(2)) * 1e3
        r = dict(layer=f"{N} {H}x{H} {cin}->{cout} {name}", dgrad_us=round(us(dgrad), 1), wgrad_us=round(us(wgrad), 1),
                 pair_us=round(us(pair), 1), bound_us=round(bound, 1),
                 fused_us={str(v): round(us(fused_of(v)), 1) for v in WGS})
        best = min(r["fused_us"].values())
        r["fused_share_of_bound"] = round(bound / best, 3)
        rows.append(r)
        print(f"{r['layer']:30s} dgrad {r['dgrad_us']:7.1f} wgrad {r['wgrad_us']:7.1f} pair {r['pair_us']:7.1f}  "
              f"fused {r['fused_us']}  bound {bound:6.1f} ({100 * bound / best:4.1f} % of bound)", flush=True)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(rows, open(out_path, "w"), indent=1)

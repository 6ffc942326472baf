#!/usr/bin/env python3
"""Per-layer A/B of the join-backward epilogue's operand prefetch (FDT_EPI_PREFETCH, conv_epilogue's
PF): every reducing 1x1 data gradient with the join-backward epilogue as the tuned table launches it,
switch off against on in one process, HIP-graph replay (roofline_layers.timeit), identity and conv
shortcut (the K = 512 layers, which the table leaves on the implicit-GEMM kernel, also with an
explicit kg 10).  Also the share of the one-pass byte bound (g + y, incoming gradient + residual branch
[+ shortcut branch] + mask read, gradient written, at 6.3 TB/s).
python scripts/ab_epi_prefetch_layers.py BATCH [OUT.json]"""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else f"ab_epi_prefetch_{N}.json"
# (H, cin, cout) of the forward convolution; the data gradient is the GEMM K = cout, Nout = cin
DG = [(32, 256, 64), (32, 256, 128), (16, 512, 128), (16, 512, 256), (8, 1024, 256), (8, 1024, 512), (4, 2048, 512)]
X1_EXPLICIT = (512,)  # K whose table entries keep the implicit-GEMM kernel: also timed with an explicit kg 10, xn 2
HBM = 6.3e12
rows = []

for (H, cin, cout) in DG:
    shp = ci.ConvShape(cin, cout, 1, 1, 0)
    torch.manual_seed(0)
    w = torch.randn(cout, cin, 1, 1, device=dev) / cin ** 0.5
    wf, wd = ci.alloc_packed(shp, dev)
    ci.pack_weights([(w, wf, wd, shp)])
    g = torch.randn(N, H, H, cout, device=dev).to(torch.bfloat16)
    yy = torch.randn(N, H, H, cout, device=dev).to(torch.bfloat16)
    al, be = torch.zeros(cout, device=dev), torch.zeros(cout, device=dev)
    xs = (N, H, H, cin)
    out = torch.zeros(xs, device=dev, dtype=torch.bfloat16)
    ex = torch.randn(xs, device=dev).to(torch.bfloat16)
    jyb = torch.randn(xs, device=dev).to(torch.bfloat16)
    mask = torch.randint(0, 256, (out.numel() // 8,), device=dev, dtype=torch.uint8)
    part = ci.stat_slots(3, cin, dev, N * H * H)
    M = N * H * H
    for sc, x1 in ((False, None), (True, None)) + ((((False, 2), (True, 2))) if cout in X1_EXPLICIT else ()):
        def fn():
            kw = dict(tile=(ci.X1_BM_OF_K[cout], 128, 32), nsplit=1, kg=10, xn=x1) if x1 else {}
            ci.conv_dgrad(g, yy, al, be, wd, shp, xs, epi=ci.EPI_JOINBWD, out=out, ex=ex, part=part, act=1,
                          jmask=mask, jyb=jyb if sc else None, **kw)
        ci.LAUNCH_LOG = []
        fn()
        kg = ci.LAUNCH_LOG[-1][5]
        ci.LAUNCH_LOG = None
        t = {}
        for on in (False, True, False, True):  # two interleaved measurements of each side
            ci.EPI_PREFETCH = on
            t.setdefault(on, []).append(timeit(fn) * 1e3)
        ci.EPI_PREFETCH = ci.epi_prefetch_default()
        bound = (2 * M * cout * 2 + (4 if sc else 3) * M * cin * 2 + M * cin // 8) / HBM * 1e6
        off, onv = min(t[False]), min(t[True])
        row = dict(layer=f"{N} {H}x{H} {cin}->{cout} dgrad join{'+sc' if sc else ''}{' (explicit kg 10)' if x1 else ''}", kg=kg, off_us=[round(v, 1) for v in t[False]],
                   on_us=[round(v, 1) for v in t[True]], bound_us=round(bound, 1), share_off=round(bound / off, 3),
                   share_on=round(bound / onv, 3), faster_both=all(b < a for a, b in zip(t[False], t[True])))
        rows.append(row)
        print(f"{row['layer']:54s} kg {kg:2d}  off {row['off_us']}  on {row['on_us']}  ({100 * (onv / off - 1):+5.1f} %)  "
              f"bound {bound:6.1f} us  share {row['share_off']:.2f} -> {row['share_on']:.2f}", flush=True)
    del g, yy, out, ex, jyb, mask

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(rows, open(out_path, "w"), indent=1)

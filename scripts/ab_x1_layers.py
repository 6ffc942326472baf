#!/usr/bin/env python3
"""Per-layer A/B for the activation-stationary 1x1 kernel (kg 10): the tuned table's launch against
kg 10 at every xn, for the in-scope forward layers (fwd1 / fwd0) and data gradients (store / add /
join-backward), HIP-graph replay (roofline_layers.timeit).  python scripts/ab_x1_layers.py BATCH [OUT.json]"""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else f"ab_x1_layers_{N}.json"
FWD = [(32, 64, 256), (16, 128, 512), (8, 256, 1024), (4, 512, 2048)]
DG = [(32, 256, 64), (16, 512, 128), (8, 1024, 256), (4, 2048, 512), (32, 256, 128), (16, 512, 256), (8, 1024, 512)]
rows = []


def cands(K, nout):
    nbn = nout // 128
    bm = ci.X1_BM_OF_K[K]
    return [(bm, xn) for xn in (1, 2, 4, 8, 16) if nbn % xn == 0]


def run(name, key, fn_of):
    base = min(timeit(fn_of(None, None, None)) for _ in range(2)) * 1e3
    res = {}
    for bm, xn in cands(*key):
        res[f"{bm}/{xn}"] = round(min(timeit(fn_of((bm, 128, 32), 10, xn)) for _ in range(2)) * 1e3, 1)
    best = min(res, key=res.get)
    rows.append(dict(layer=name, table_us=round(base, 1), x1=res, best=best, best_us=res[best]))
    print(f"{name:34s} table {base:7.1f}  best {best:7s} {res[best]:7.1f}  ({100 * (res[best] / base - 1):+5.1f} %)  {res}", flush=True)


for (H, cin, cout) in FWD:
    shp = ci.ConvShape(cin, cout, 1, 1, 0)
    torch.manual_seed(0)
    x = torch.randn(N, H, H, cin, device=dev).to(torch.bfloat16)
    w = torch.randn(cout, cin, 1, 1, device=dev) / cin ** 0.5
    wf, wd = ci.alloc_packed(shp, dev)
    ci.pack_weights([(w, wf, wd, shp)])
    sv, tv = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
    part = ci.stat_slots(2, cout, dev, N * H * H)
    for op in ("fwd1", "fwd0"):
        def fn_of(tile, kg, xn, op=op):
            if op == "fwd1":
                return lambda: ci.conv_fwd(x, wf, shp, sv, tv, 1, 1.0, tile=tile, kg=kg, xn=xn, part=part,
                                           nsplit=1 if tile else None)
            return lambda: ci.conv_fwd(x, wf, shp, tile=tile, kg=kg, xn=xn, part=part, nsplit=1 if tile else None)
        run(f"{N} {H}x{H} {cin}->{cout} {op}", (cin, cout), fn_of)
    del x, w, wf, wd

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
    mask = torch.randint(0, 256, (out.numel() // 8,), device=dev, dtype=torch.uint8)
    part = ci.stat_slots(3, cin, dev, N * H * H)
    for op, epi in (("store", ci.EPI_STORE), ("add", ci.EPI_ADD), ("join", ci.EPI_JOINBWD)):
        def fn_of(tile, kg, xn, epi=epi):
            kw = dict(ex=ex, part=part, act=1, jmask=mask) if epi == ci.EPI_JOINBWD else {}
            return lambda: ci.conv_dgrad(g, yy, al, be, wd, shp, xs, epi=epi, out=out, tile=tile, kg=kg, xn=xn,
                                         nsplit=1 if tile else None, **kw)
        run(f"{N} {H}x{H} {cin}->{cout} dgrad {op}", (cout, cin), fn_of)
    del g, yy, out, ex, mask

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(rows, open(out_path, "w"), indent=1)

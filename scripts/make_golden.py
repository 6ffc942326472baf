#!/usr/bin/env python3
"""Record what the reference implementation computes on the tests' fixed inputs.

    python scripts/make_golden.py /path/to/Faster-Distributed-Training

writes ``tests/golden/*.npz`` and ``state_dict_schema.json`` (read by tests/reference_oracle.py).
Only the reference's pure-torch modules are imported (resnet.py, transformer.py,
ngd_optimizer.py); nothing is written into its directory.  CPU, fp64, a few seconds.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reference_oracle as G  # noqa: E402


def load(ref_dir, name):
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location(f"_fdt_ref_{name}", os.path.join(ref_dir, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def save(name, **arrays):
    np.savez(os.path.join(G.GOLDEN, name + ".npz"), **{k: v.detach().numpy() for k, v in arrays.items()})


def main():
    ref_dir = sys.argv[1]
    os.makedirs(G.GOLDEN, exist_ok=True)
    resnet, transformer, ngd = (load(ref_dir, n) for n in ("resnet", "transformer", "ngd_optimizer"))

    # parameter schema (checkpoint compatibility)
    torch.manual_seed(0)
    schemas = {a: G.schema(getattr(resnet, a)(10).state_dict()) for a in ("resnet18", "resnet50")}
    schemas["transformer_4_1000"] = G.schema(transformer.Transformer(4, 1000).state_dict())
    with open(os.path.join(G.GOLDEN, "state_dict_schema.json"), "w") as f:
        json.dump(schemas, f, indent=0)
        f.write("\n")

    # fused conv + batch-norm autograd function
    torch.manual_seed(0)
    X = torch.randn(4, 8, 6, 6, dtype=torch.float64, requires_grad=True)
    W = torch.randn(6, 8, 3, 3, dtype=torch.float64, requires_grad=True)
    g = torch.randn(4, 6, 6, 6, dtype=torch.float64)
    out = resnet.FusedConvBN2DFunction.apply(X, W, 1, 1, 1e-3)
    gx, gw = torch.autograd.grad(out, (X, W), g)
    save("fused_conv_bn", X=X, W=W, g=g, out=out, gx=gx, gw=gw)

    # whole-model forward + backward on seeded weights
    for arch in ("resnet18", "resnet50"):
        m = getattr(resnet, arch)(10).double()
        G.fill_state(m.state_dict(), seed=7)
        x, y = G.resnet_batch()
        loss = F.cross_entropy(m(x), y)
        loss.backward()
        save(f"{arch}_fwd_bwd", loss=loss, **G.grad_record([p.grad.reshape(-1) for p in m.parameters()]))

    # transformer pieces
    torch.manual_seed(0)
    x = torch.randn(2, 7, 64, dtype=torch.float64)
    ln = transformer.LayerNorm(64).double()
    with torch.no_grad():
        ln.a_2.uniform_()
    emb = transformer.Embeddings(64, 50, 16).double()
    ids = torch.randint(0, 50, (2, 7))
    types = torch.randint(0, 3, (2, 7))
    save("transformer_pieces", x=x, ln_a_2=ln.a_2, ln_out=ln(x), ids=ids, types=types,
         emb_out=emb(ids, types, torch.arange(16)), **{"emb." + k: v for k, v in emb.state_dict().items()})

    # online natural gradient: 20 steps per (shape, axis)
    for shape, axis in [((12, 7), 0), ((12, 7), 1), ((6, 5, 3), 1), ((40,), 0)]:
        torch.manual_seed(0)
        ong = ngd.OnlineNaturalGradient(torch.zeros(shape, dtype=torch.float64), axis, alpha=4.0, update_period=4,
                                        eta=0.1)
        gs = [torch.randn(shape, dtype=torch.float64) * (1 + step % 3) for step in range(20)]
        outs = [ong.precondition_directions(g.clone()) for g in gs]
        save("ong_" + "x".join(map(str, shape)) + f"_axis{axis}", g=torch.stack(gs), out=torch.stack(outs))

    # the NGD optimizer: weight decay -> per-axis preconditioning -> momentum, 12 steps
    torch.manual_seed(0)
    mb = nn.Sequential(nn.Linear(8, 6, bias=False), nn.Linear(6, 3, bias=False)).double()
    init = [p.detach().clone() for p in mb.parameters()]
    opt = ngd.NGD(mb.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    grads = ([], [])
    for s in range(12):
        gen = torch.Generator().manual_seed(100 + s)
        for p, keep in zip(mb.parameters(), grads):
            p.grad = torch.randn(p.shape, generator=gen, dtype=torch.float64)
            keep.append(p.grad.clone())
        opt.step()
    final = list(mb.parameters())
    save("ngd_optimizer", init0=init[0], init1=init[1], grad0=torch.stack(grads[0]), grad1=torch.stack(grads[1]),
         final0=final[0], final1=final[1])


if __name__ == "__main__":
    main()

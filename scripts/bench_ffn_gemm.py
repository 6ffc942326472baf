#!/usr/bin/env python3
"""The FFN's two GELU-dropout GEMMs on MI355X, per call under graph replay in alternating windows:

  forward   (a) library GEMM x W_1^T + b_1, then gelu_dropout_fwd   (the default path)
            (b) the implicit-GEMM kernel's epilogue                (FDT_FFN_FUSED=1)
            (c) linear_gemm.hip's epilogue                         (FDT_FFN_FUSED=gemm)
  backward  (a) library g @ W_2, then gelu_dropout_bwd_colsum
            (b) the implicit-GEMM kernel on a transposed copy of W_2 (the copy is part of every call)
            (c) linear_gemm.hip on W_2 as stored, then linear_bias_fold

    python scripts/bench_ffn_gemm.py [--tokens 32768 4096] [--dff 2048 1024]

One JSON line per (side, M, d_ff): median (min, max) us of each variant, the relative Frobenius difference
of (b) and (c) from (a), and the verdict of (c) against (a) ("faster" / "slower": the min-max ranges do
not overlap).  Every variant allocates its outputs inside the call, as ops/ffn.py does; p = 0.1.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from bench_linear_gemm import alternating


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[32768, 4096])
    ap.add_argument("--dff", type=int, nargs="+", default=[2048, 1024])
    ap.add_argument("--dmodel", type=int, default=512)
    args = ap.parse_args()
    from faster_distributed_training_amd.ops import _native, ffn
    from faster_distributed_training_amd.ops.linear import bias_fold_into
    nat = _native.native()
    dev = torch.device("cuda")
    bf, p, seed, D = torch.bfloat16, 0.1, 0x5DEECE66D, args.dmodel
    for M in args.tokens:
        for dff in args.dff:
            x = torch.randn(M, D, device=dev).to(bf)
            w1 = (torch.randn(dff, D, device=dev) / D ** 0.5).to(bf)
            b1 = (torch.randn(dff, device=dev) * 0.1).to(bf)
            b1f = b1.float()
            g = torch.randn(M, D, device=dev).to(bf)
            w2 = (torch.randn(D, dff, device=dev) / dff ** 0.5).to(bf)
            act = F.linear(x, w1, b1)
            gb = torch.zeros(dff, device=dev)  # accumulated into by every call: never compared

            def fwd_lib():
                a = F.linear(x, w1, b1)
                h = torch.empty_like(a)
                nat.gelu_dropout_fwd(a.data_ptr(), h.data_ptr(), a.numel(), p, seed, 0, _native.stream_ptr())
                return h

            def fwd_igemm():
                a, h = torch.empty(M, dff, device=dev, dtype=bf), torch.empty(M, dff, device=dev, dtype=bf)
                ffn._gemm(x, w1, a, ffn.EPI_GELU_FWD, bias=b1f, out2=h, p=p, seed=seed, tile=ffn.TILE_FWD)
                return h

            def fwd_gemm():
                a, h = torch.empty(M, dff, device=dev, dtype=bf), torch.empty(M, dff, device=dev, dtype=bf)
                ffn._gemm_gelu(x, w1, 0, a, h, bias=b1, p=p, seed=seed)
                return h

            def bwd_lib():
                gh = g @ w2
                ga = torch.empty_like(gh)
                nat.gelu_dropout_bwd_colsum(gh.data_ptr(), act.data_ptr(), ga.data_ptr(), gb.data_ptr(), M, dff, p,
                                            seed, 0, _native.stream_ptr())
                return ga

            def bwd_igemm():
                ga = torch.empty(M, dff, device=dev, dtype=bf)
                ffn._gemm(g, w2.t().contiguous(), ga, ffn.EPI_GELU_BWD, a_in=act, gb=gb, p=p, seed=seed,
                          tile=ffn.TILE_BWD)
                return ga

            def bwd_gemm():
                ga = torch.empty(M, dff, device=dev, dtype=bf)
                slab = torch.empty((M + 127) // 128, dff, device=dev)
                ffn._gemm_gelu(g, w2, 1, act, ga, gbslab=slab, p=p, seed=seed)
                bias_fold_into(slab, gb)
                return ga

            for side, fns in (("forward", (fwd_lib, fwd_igemm, fwd_gemm)), ("backward", (bwd_lib, bwd_igemm, bwd_gemm))):
                ref = fns[0]().double()
                diffs = [float(f"{((f().double() - ref).norm() / ref.norm()).item():.2e}") for f in fns[1:]]
                ts = alternating(list(fns))
                (_, l0, l1), _, (_, n0, n1) = ts
                verdict = "faster" if n1 < l0 else "slower" if n0 > l1 else "inside the spread"
                row = {"side": side, "M": M, "d_model": D, "d_ff": dff}
                for name, t in zip(("library_us", "igemm_us", "gemm_us"), ts):
                    row[name] = [round(v, 1) for v in t]
                row.update(rel_diff_igemm=diffs[0], rel_diff_gemm=diffs[1], gemm_vs_library=verdict)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

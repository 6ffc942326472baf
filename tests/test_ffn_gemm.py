"""csrc/kernels/linear_gemm.hip linear_gemm_gelu: the dense MFMA GEMM finished through the FFN's
GELU-dropout epilogues, and ops/ffn.py on it (``FDT_FFN_FUSED=gemm``).

Oracles: pointwise_oracle (fp64 GELU, the host replica of the dropout hash).  Forward: a must EQUAL the
plain kernel's output; h is one bf16 rounding (2^-8 with slack) of keep * gelu(a) / (1 - p) at the
kernel's own a, plus 2^-20 for fp32 erff in the cancelling negative tail.  Backward: with dh the fp64
product, gamma = K 2^-23 (|gy| @ |w2|) the fp32 accumulation bound of test_linear_gemm.py and
f = |gelu'(a)| / (1 - p), e = f gamma + 2^-16 |dh| / (1 - p) (the second term caps fp32 erff / __expf in
gelu'), ga is within e + 2^-8 (|ref| + e) and the folded column sums within the summed e plus sum_bound.
"""
import pytest
import torch

import pointwise_oracle as po
from faster_distributed_training_amd.ops import linear as L

BF16 = torch.bfloat16
CASES = [(128, 128, 128, 0),                    # one tile, two K steps (the ring depth)
         (1003, 384, 128, 0x123456789ABCDEF0),  # partial last panel, three N tiles; a device seed word
         (300, 128, 640, 0)]                    # ten K steps
PAD = 200                                       # NaN rows past M, to the end of the last panel and beyond
SEED = 0x5DEECE66D


def bound_bwd(gy, w2, a, p):
    """(ref without the mask, e) of the backward epilogue; see the module docstring."""
    dh = po.f64(gy) @ po.f64(w2)
    gamma = gy.shape[1] * 2.0 ** -23 * (po.f64(gy).abs() @ po.f64(w2).abs())
    s = po.drop_scale(p)
    return s * po.gelu_grad(a) * dh, s * po.gelu_grad(a).abs() * gamma + 2.0 ** -16 * s * dh.abs()


def call(kind, x, w, act, out, M, bias=None, slab=None, p=0.0, word=None):
    from faster_distributed_training_amd.ops import _native
    N = out.shape[1]
    _native.native().linear_gemm_gelu(x.data_ptr(), w.data_ptr(), _native.ptr(bias), act.data_ptr(), out.data_ptr(),
                                      _native.ptr(slab), M, N, x.shape[1], kind, p, SEED, _native.ptr(word),
                                      _native.stream_ptr())


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M,N,K,word", CASES)
def test_forward_epilogue(cuda, M, N, K, word, p):
    g = torch.Generator(device=cuda).manual_seed(M)
    x = torch.randn(M, K, device=cuda, generator=g).to(BF16)
    w1 = torch.randn(N, K, device=cuda, generator=g).to(BF16)
    b1 = torch.randn(N, device=cuda, generator=g).to(BF16)
    wt = torch.tensor([word], dtype=torch.int64, device=cuda) if word else None
    outs = []
    for _ in range(2):
        a = torch.full((M + PAD, N), float("nan"), device=cuda, dtype=BF16)
        h = torch.full_like(a, float("nan"))
        call(0, x, w1, a, h, M, bias=b1, p=p, word=wt)
        outs.append((a, h))
    (a, h), (a2, h2) = outs
    assert torch.equal(a[:M], L.gemm(x, w1, b1, "nt"))
    keep = po.keep_mask_t((M, N), SEED, p, cuda, word)
    ref = keep * po.gelu(a[:M]) * po.drop_scale(p)
    err = (po.f64(h[:M]) - ref).abs() - (2.0 ** -8 * ref.abs() + 2.0 ** -20)
    print(f"forward M={M} N={N} K={K} p={p}: max excess {err.max().item():.3e}")
    assert bool((err <= 0).all())
    assert bool((h[:M][~keep] == 0).all())
    assert bool(a[M:].isnan().all()) and bool(h[M:].isnan().all())
    assert torch.equal(a2[:M], a[:M]) and torch.equal(h2[:M], h[:M])


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M,N,K,word", CASES)
def test_backward_epilogue(cuda, M, N, K, word, p):
    from faster_distributed_training_amd.ops import _native
    g = torch.Generator(device=cuda).manual_seed(M + 1)
    gy = torch.randn(M, K, device=cuda, generator=g).to(BF16)
    w2 = torch.randn(K, N, device=cuda, generator=g).to(BF16)
    a = torch.full((M + PAD, N), float("nan"), device=cuda, dtype=BF16)
    a[:M] = torch.randn(M, N, device=cuda, generator=g).to(BF16)
    wt = torch.tensor([word], dtype=torch.int64, device=cuda) if word else None
    panels = (M + 127) // 128

    def run(fill):
        ga = torch.full((M + PAD, N), float("nan"), device=cuda, dtype=BF16)
        slab = torch.full((panels, N), float("nan"), device=cuda)
        call(1, gy, w2, a, ga, M, slab=slab, p=p, word=wt)
        gb = torch.full((N,), fill, device=cuda)
        _native.native().linear_bias_fold(slab.data_ptr(), gb.data_ptr(), panels, N, N, _native.stream_ptr())
        return ga, gb

    ga, gb = run(0.0)
    keep = po.keep_mask_t((M, N), SEED, p, cuda, word)
    ref, e = bound_bwd(gy, w2, a[:M], p)
    ref = keep * ref
    err = (po.f64(ga[:M]) - ref).abs() - (e + 2.0 ** -8 * (ref.abs() + e))
    print(f"backward M={M} N={N} K={K} p={p}: max excess {err.max().item():.3e}")
    assert bool((err <= 0).all())
    assert bool((ga[:M][~keep] == 0).all())
    assert bool(ga[M:].isnan().all())
    assert bool(gb.isfinite().all())
    errb = (po.f64(gb) - ref.sum(0)).abs() - (e.sum(0) + po.sum_bound(M, ref.abs().sum(0)))
    print(f"column sums: max excess {errb.max().item():.3e}")
    assert bool((errb <= 0).all())
    ga2, gb2 = run(0.0)
    assert torch.equal(ga2[:M], ga[:M]) and torch.equal(gb2, gb)
    assert torch.equal(run(0.5)[1], 0.5 + gb)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("direct", [False, True])
def test_module_on_gemm_kernel(cuda, monkeypatch, p, direct):
    """PositionalWiseFFN at 4100 tokens (a partial panel) on the gemm kernel against the unfused path on
    the same dropout draw, and two runs of the new path bit for bit, b_1's gradient included."""
    from faster_distributed_training_amd.models import transformer as T
    from faster_distributed_training_amd.ops import ffn
    from faster_distributed_training_amd.ops.linear import enable_direct_grads
    torch.manual_seed(0)
    m = T.PositionalWiseFFN(512, 1024, p).to(cuda)
    x = torch.randn(4, 1025, 512, device=cuda).to(BF16).requires_grad_(True)
    g = torch.randn(4, 1025, 512, device=cuda)
    monkeypatch.setattr(ffn, "KERNEL", "gemm")
    monkeypatch.setattr(ffn, "FUSED", True)
    assert ffn.fusable(x, 512, 1024)

    def run(fused):
        monkeypatch.setattr(ffn, "FUSED", fused)
        x.grad = None
        for q in m.parameters():
            q.grad = torch.full_like(q, 0.5) if direct else None
        enable_direct_grads(m.parameters(), direct)
        torch.manual_seed(5)
        with torch.autocast("cuda", dtype=BF16):
            y = m(x)
        y.float().backward(g)
        torch.cuda.synchronize()
        return [y.detach().float(), x.grad.float().clone()] + [q.grad.clone() for q in m.parameters()]

    try:
        r0, r1, r2 = run(False), run(True), run(True)
    finally:
        enable_direct_grads(m.parameters(), False)
    for a_, b_, name, tol in zip(r1, r0, ["y", "x", "w1", "b1", "w2", "b2"], [1e-2] + [2e-2] * 5):
        rel = ((a_ - b_).norm() / b_.norm()).item()
        assert rel < tol, (name, rel)
    for a_, b_, name in zip(r1, r2, ["y", "x", "w1", "b1", "w2", "b2"]):
        assert torch.equal(a_, b_), name


def test_fusable_gates(monkeypatch):
    from faster_distributed_training_amd.ops import ffn
    monkeypatch.setattr(ffn, "KERNEL", "gemm")
    monkeypatch.setattr(ffn, "FUSED", True)
    assert not ffn.fusable(torch.zeros(4096, 512, dtype=BF16), 512, 1024)
    assert not ffn.fusable(torch.zeros(4096, 64, dtype=BF16), 64, 1024)

"""csrc/kernels/linear_gemm.hip: the dense MFMA GEMM of the linears' forward (nt) and data gradient (nn).

Exact oracle: operands and bias are integers in [-4, 4] (exact in bf16), so every fp32 partial sum is
an integer below 16 * 640 + 4 < 2**24, exact in any order: the output must EQUAL the fp64 result
rounded to bf16.  Normal data: with ref the fp64 product of the bf16 operands and
gamma = K * 2**-23 * (|a| @ |b|) (fp32 accumulation), |out - ref| <= gamma + 2**-8 * (|ref| + gamma)
(one bf16 RNE rounding is at most 2**-9 of the value).
"""
import pytest
import torch
import torch.nn.functional as F

from faster_distributed_training_amd.ops import linear as L

CASES = [(128, 128, 128),    # one tile, two K steps (the ring depth)
         (1003, 384, 128),   # odd M: a partial last panel whose rows must not be stored; several N tiles
         (300, 128, 640),    # ten K steps: the ring wraps many times
         (4120, 256, 512)]   # 33 panels x 2 tiles = 66 workgroups, no multiple of the 8 XCDs
PAD = 200                    # NaN rows past M, to the end of the last panel and beyond


def within(out, ref, gamma):
    return bool(((out.double() - ref).abs() <= gamma + 2.0 ** -8 * (ref.abs() + gamma)).all())


def run(a, w, bias, kind):
    """The kernel into a NaN-filled output over-allocated by PAD rows."""
    from faster_distributed_training_amd.ops import _native
    M, K = a.shape
    N = w.shape[0] if kind == "nt" else w.shape[1]
    out = torch.full((M + PAD, N), float("nan"), device=a.device, dtype=torch.bfloat16)
    _native.native().linear_gemm(a.data_ptr(), w.data_ptr(), _native.ptr(bias), out.data_ptr(), M, N, K,
                                 L._KINDS[kind], _native.stream_ptr())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nt", "nn"])
@pytest.mark.parametrize("M,N,K", CASES)
def test_kernel_against_fp64(cuda, kind, M, N, K):
    g = torch.Generator(device=cuda).manual_seed(M + (kind == "nn"))
    wshape = (N, K) if kind == "nt" else (K, N)
    a = torch.randint(-4, 5, (M, K), device=cuda, generator=g).to(torch.bfloat16)
    w = torch.randint(-4, 5, wshape, device=cuda, generator=g).to(torch.bfloat16)
    bias = torch.randint(-4, 5, (N,), device=cuda, generator=g).to(torch.bfloat16) if kind == "nt" else None
    mat = (lambda t: t.double().t()) if kind == "nt" else (lambda t: t.double())
    ref = a.double() @ mat(w) + (bias.double() if bias is not None else 0)
    out = run(a, w, bias, kind)
    assert torch.equal(out[:M], ref.to(torch.bfloat16))
    assert bool(out[M:].isnan().all())
    assert torch.equal(run(a, w, bias, kind)[:M], out[:M])
    if M in (1003, 4120):  # rounding: standard-normal operands
        a = torch.randn(M, K, device=cuda, generator=g).to(torch.bfloat16)
        w = torch.randn(wshape, device=cuda, generator=g).to(torch.bfloat16)
        out = run(a, w, None, kind)
        gamma = K * 2.0 ** -23 * (a.double().abs() @ mat(w).abs())
        assert within(out[:M], a.double() @ mat(w), gamma)
        assert bool(out[M:].isnan().all())


@pytest.mark.gpu
@pytest.mark.parametrize("cat", [False, True])
def test_linear_through_hip(cuda, monkeypatch, cat):
    """linear() / linear_cat() at 32 x 128 tokens, 512 -> 1536: the HIP path is taken for both kinds,
    y and x.grad agree with F.linear in fp32 on the bf16-rounded operands, two passes are bitwise
    equal, and FDT_LINEAR_GEMM=0 gives the library result bit for bit."""
    torch.manual_seed(7)
    nw = 3 if cat else 1
    ws = [(torch.randn(1536 // nw, 512, device=cuda) / 512 ** 0.5).requires_grad_() for _ in range(nw)]
    bs = [(torch.randn(1536 // nw, device=cuda) * 0.1).requires_grad_() for _ in range(nw)]
    x = torch.randn(32, 128, 512, device=cuda).requires_grad_()
    g = torch.randn(32, 128, 1536, device=cuda).to(torch.bfloat16)

    def step():
        x.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = L.linear_cat(x, ws, bs) if cat else L.linear(x, ws[0], bs[0])
        y.backward(g)
        return y.detach(), x.grad.clone()

    monkeypatch.setenv("FDT_LINEAR_GEMM", "1")
    assert L.gemm_backend("nt", 4096, 1536, 512, torch.bfloat16, cuda) == "hip"
    assert L.gemm_backend("nn", 4096, 512, 1536, torch.bfloat16, cuda) == "hip"
    (y, dx), (y2, dx2) = step(), step()
    assert y.dtype == torch.bfloat16 and torch.equal(y, y2) and torch.equal(dx, dx2)
    xb, gb = x.detach().to(torch.bfloat16), g.view(-1, 1536)
    wb, bb = torch.cat(ws).detach().to(torch.bfloat16), torch.cat(bs).detach().to(torch.bfloat16)
    xr = xb.float().requires_grad_()
    yr = F.linear(xr, wb.float(), bb.float())
    yr.backward(g.float())
    gam_y = 512 * 2.0 ** -23 * (xb.view(-1, 512).double().abs() @ wb.double().abs().t())
    gam_x = 1536 * 2.0 ** -23 * (gb.double().abs() @ wb.double().abs())
    assert within(y.view(-1, 1536), yr.detach().view(-1, 1536).double(), gam_y)
    assert within(dx.view(-1, 512), xr.grad.view(-1, 512).double(), gam_x)
    monkeypatch.setenv("FDT_LINEAR_GEMM", "0")
    y0, dx0 = step()
    assert torch.equal(y0, F.linear(xb, wb, bb))
    assert torch.equal(dx0, (gb @ wb).view(x.shape).float())


def test_backend_library_cases(monkeypatch):
    bf = torch.bfloat16
    monkeypatch.setenv("FDT_LINEAR_GEMM", "1")
    assert L.gemm_backend("nt", 4096, 512, 512, bf, torch.zeros(1).device) == "library"
    assert L.gemm_backend("nt", 4096, 512, 512, torch.float16) == "library"
    assert L.gemm_backend("nt", 4096, 520, 512, bf) == "library"
    assert L.gemm_backend("nn", 4096, 512, 64, bf) == "library"
    monkeypatch.setenv("FDT_LINEAR_GEMM", "0")
    assert L.gemm_backend("nt", 4096, 512, 512, bf) == "library"
    monkeypatch.setenv("FDT_LINEAR_GEMM", "auto")
    assert ("nn", 4000, 512, 512) not in L._AUTO_GEMM
    assert L.gemm_backend("nn", 4000, 512, 512, bf) == "library"
    monkeypatch.setenv("FDT_LINEAR_GEMM", "yes")
    with pytest.raises(ValueError):
        L.gemm_backend("nt", 4096, 512, 512, bf)

"""csrc/kernels/linear_wgrad.hip: the split-K MFMA weight gradient dW = gy^T x of the linear layers.

Exact oracle: operands are integers in [-4, 4] (exact in bf16), so every product and partial
sum is an integer below 16 * 4120 < 2**17 < 2**24 and the fp32 result is exact in any summation
order -- the fold of the slabs must EQUAL the fp64 product.  Normal data: relative Frobenius
error below 1e-4 against the fp64 product of the same bf16 operands (tests/test_linear.py's bound).
"""
import pytest
import torch
import torch.nn.functional as F

from faster_distributed_training_amd.ops import linear as L

T = 128  # the kernel's tile edge
CASES = [(256, T, T, 1),          # one tile, one split, whole chunks
         (1003, T, 3 * T, 4),     # odd M, partial last 16-token step, several in-tiles
         (4120, 2 * T, T, 3),     # uneven splits, tail chunk, several out-tiles
         (520, 1536, 512, 16),    # more splits than chunks: empty splits write zeros
         (4096, 512, 1024, 0)]    # the launcher's own split choice


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def run(gy, x, nsplit):
    """The kernel into NaN-filled slabs."""
    from faster_distributed_training_amd.ops import _native
    nat = _native.native()
    (M, out), in_ = gy.shape, x.shape[1]
    s = nsplit or nat.linear_wgrad_splits(M, out, in_)
    slab = torch.full((s, out, in_), float("nan"), device=gy.device)
    bslab = torch.full((s, out), float("nan"), device=gy.device)
    nat.linear_wgrad(gy.data_ptr(), x.data_ptr(), slab.data_ptr(), bslab.data_ptr(), M, out, in_, nsplit,
                     _native.stream_ptr())
    return slab, bslab


@pytest.mark.gpu
@pytest.mark.parametrize("M,out,in_,nsplit", CASES)
def test_slabs_against_fp64(cuda, monkeypatch, M, out, in_, nsplit):
    g = torch.Generator(device=cuda).manual_seed(M)
    gy = torch.randint(-4, 5, (M, out), device=cuda, generator=g).to(torch.bfloat16)
    x = torch.randint(-4, 5, (M, in_), device=cuda, generator=g).to(torch.bfloat16)
    ref = (gy.double().t() @ x.double()).float()
    slab, bslab = run(gy, x, nsplit)
    assert torch.equal(slab.sum(0), ref)
    assert torch.equal(bslab.sum(0), gy.double().sum(0).float())
    slab2, bslab2 = run(gy, x, nsplit)
    assert torch.equal(slab2, slab) and torch.equal(bslab2, bslab)
    if M == 1003:  # the fold into a loaded destination, through the public entry
        monkeypatch.setenv("FDT_LINEAR_WGRAD", "1")
        assert L.wgrad_backend(M, out, in_, gy.dtype, gy.device) == "hip"
        dst0 = torch.randint(-1000, 1001, (out, in_), device=cuda, generator=g).float()
        dst = dst0.clone()
        L.wgrad_into(gy, x, dst)
        assert torch.equal(dst, dst0 + ref)
    if M in (4120, 4096):  # rounding: standard-normal operands
        gy = torch.randn(M, out, device=cuda, generator=g).to(torch.bfloat16)
        x = torch.randn(M, in_, device=cuda, generator=g).to(torch.bfloat16)
        slab, bslab = run(gy, x, nsplit)
        assert rel(slab.sum(0), gy.double().t() @ x.double()) < 1e-4
        assert rel(bslab.sum(0), gy.double().sum(0)) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("cat", [False, True])
def test_linear_backward_through_hip(cuda, monkeypatch, cat):
    """linear() / linear_cat() at M = 4096, 512 -> 1536 with direct fp32 gradient targets: the
    HIP path is taken, agrees with the fp32 reference on the bf16-rounded operands, and two
    backward passes give bitwise-equal weight and bias gradients."""
    monkeypatch.setenv("FDT_LINEAR_WGRAD", "1")
    assert L.wgrad_backend(4096, 1536, 512, torch.bfloat16, cuda) == "hip"
    torch.manual_seed(5)
    nw = 3 if cat else 1
    ws = [(torch.randn(1536 // nw, 512, device=cuda) / 512 ** 0.5).requires_grad_() for _ in range(nw)]
    bs = [(torch.randn(1536 // nw, device=cuda) * 0.1).requires_grad_() for _ in range(nw)]
    L.enable_direct_grads(ws + bs)
    x = torch.randn(32, 128, 512, device=cuda)
    g = torch.randn(32, 128, 1536, device=cuda).to(torch.bfloat16)
    grads = []
    for _ in range(2):
        for p in ws + bs:
            p.grad = torch.zeros_like(p)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = L.linear_cat(x, ws, bs) if cat else L.linear(x, ws[0], bs[0])
        y.backward(g)
        grads.append([p.grad.clone() for p in ws + bs])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    wr = torch.cat([w.detach().to(torch.bfloat16).float() for w in ws]).requires_grad_()
    br = torch.cat([b.detach().to(torch.bfloat16).float() for b in bs]).requires_grad_()
    F.linear(x.to(torch.bfloat16).float(), wr, br).backward(g.float())
    assert rel(torch.cat(grads[0][:nw]), wr.grad) < 1e-4
    assert rel(torch.cat(grads[0][nw:]), br.grad) < 1e-4


def test_backend_library_cases(monkeypatch):
    monkeypatch.setenv("FDT_LINEAR_WGRAD", "1")
    assert L.wgrad_backend(4096, 512, 512, torch.bfloat16, torch.zeros(1).device) == "library"
    assert L.wgrad_backend(4096, 512, 512, torch.float16) == "library"
    assert L.wgrad_backend(4096, 520, 512, torch.bfloat16) == "library"

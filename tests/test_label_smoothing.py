"""Label smoothing in the mixup cross entropy: the torch path and ``mixup_criterion``'s handling
of ``nn.CrossEntropyLoss`` (CPU), the smoothed instantiation of the fused kernel (GPU)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from faster_distributed_training_amd.ops import mixup as M


def _ref(logits, ya, yb, lam, eps):
    """lam * CE_eps(a) + (1 - lam) * CE_eps(b), batch mean; lam a float or a (B,) vector."""
    ce_a = F.cross_entropy(logits, ya, reduction="none", label_smoothing=eps)
    ce_b = F.cross_entropy(logits, yb, reduction="none", label_smoothing=eps)
    return (lam * ce_a + (1 - lam) * ce_b).mean()


# ------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("eps", [0.1, 0.5])
def test_smoothed_loss_cpu(eps):
    torch.manual_seed(0)
    logits = torch.randn(5, 10, requires_grad=True)
    ya, yb = torch.randint(0, 10, (5,)), torch.randint(0, 10, (5,))
    lam = 0.3
    ref = lam * F.cross_entropy(logits, ya, label_smoothing=eps) + (1 - lam) * F.cross_entropy(logits, yb, label_smoothing=eps)
    assert torch.allclose(M.mixup_cross_entropy(logits, ya, yb, lam, label_smoothing=eps), ref, atol=1e-6)
    assert torch.allclose(M.mixup_criterion(None, logits, ya, yb, lam, label_smoothing=eps), ref, atol=1e-6)
    lv = torch.rand(5)
    assert torch.allclose(M.mixup_cross_entropy(logits, ya, yb, lv, label_smoothing=eps), _ref(logits, ya, yb, lv, eps),
                          atol=1e-6)
    assert torch.allclose(M.mixup_criterion_meta(None, logits, ya, yb, lv.view(5, 1, 1, 1), label_smoothing=eps),
                          _ref(logits, ya, yb, lv, eps), atol=1e-6)
    # the keyword at 0 is the unsmoothed loss
    assert torch.equal(M.mixup_cross_entropy(logits, ya, yb, lv, label_smoothing=0.0),
                       M.mixup_cross_entropy(logits, ya, yb, lv))


def test_criterion_smoothing_is_honoured_cpu():
    """``nn.CrossEntropyLoss(label_smoothing=...)`` used to be computed without its smoothing."""
    torch.manual_seed(1)
    logits = torch.randn(6, 10)
    ya, yb = torch.randint(0, 10, (6,)), torch.randint(0, 10, (6,))
    lam = 0.3
    crit = nn.CrossEntropyLoss(label_smoothing=0.1)
    got = M.mixup_criterion(crit, logits, ya, yb, lam)
    assert torch.allclose(got, lam * crit(logits, ya) + (1 - lam) * crit(logits, yb), atol=1e-6)
    plain = M.mixup_criterion(nn.CrossEntropyLoss(), logits, ya, yb, lam)
    assert torch.allclose(plain, M.mixup_criterion(None, logits, ya, yb, lam), atol=0)
    assert abs(float(got) - float(plain)) > 1e-3  # the silent drop


@pytest.mark.parametrize("kw", [dict(weight=torch.linspace(0.5, 2.0, 10)), dict(ignore_index=3),
                                dict(reduction="sum")])
def test_criterion_generic_path_cpu(kw):
    """Class weights, an ignore_index and another reduction are not what the fused kernel computes:
    such a criterion is applied to both targets and blended."""
    torch.manual_seed(2)
    logits = torch.randn(6, 10)
    ya, yb = torch.randint(0, 10, (6,)), torch.randint(0, 10, (6,))
    ya[0] = 3
    lam = 0.3
    crit = nn.CrossEntropyLoss(**kw)
    got = M.mixup_criterion(crit, logits, ya, yb, lam)
    assert torch.equal(got, lam * crit(logits, ya) + (1 - lam) * crit(logits, yb))
    assert not torch.allclose(got, M.mixup_criterion(None, logits, ya, yb, lam), atol=1e-4)


def test_smoothing_range_is_checked():
    logits, y = torch.randn(4, 10), torch.zeros(4, dtype=torch.int64)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="label_smoothing"):
            M.mixup_cross_entropy(logits, y, y, 0.5, label_smoothing=bad)


# ------------------------------------------------------------------------------ GPU
def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.gpu
@pytest.mark.parametrize("vector", [True, False])
@pytest.mark.parametrize("eps", [0.1, 0.5])
@pytest.mark.parametrize("C", [10, 100, 256])
def test_smoothed_ce_kernel(cuda, C, eps, vector):
    """fp32 logits, B = 64; C = 10 runs a row per thread, 100 and 256 a row per wave.  Tolerances:
    those of the unsmoothed check (test_gpu_kernels.py test_mixup_kernels)."""
    torch.manual_seed(C)
    B = 64
    base = torch.randn(B, C, device=cuda)
    ya, yb = torch.randint(0, C, (B,), device=cuda), torch.randint(0, C, (B,), device=cuda)
    lam = torch.rand(B, device=cuda).requires_grad_() if vector else 0.3
    logits = base.clone().requires_grad_()
    loss = M.mixup_cross_entropy(logits, ya, yb, lam, label_smoothing=eps)
    loss.backward()
    l2 = base.clone().requires_grad_()
    lam2 = lam.detach().clone().requires_grad_() if vector else lam
    ref = _ref(l2, ya, yb, lam2, eps)
    ref.backward()
    print(f"C={C} eps={eps} vector={vector}: |loss-ref| {abs(loss.item() - ref.item()):.3e} "
          f"rel dlogits {rel(logits.grad, l2.grad):.3e}")
    assert abs(loss.item() - ref.item()) < 1e-5
    assert rel(logits.grad, l2.grad) < 1e-5
    if vector:
        print(f"  rel dlam {rel(lam.grad, lam2.grad):.3e}")
        assert rel(lam.grad, lam2.grad) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("C", [10, 100])
def test_smoothing_zero_is_the_unsmoothed_kernel(cuda, C):
    torch.manual_seed(4)
    base = torch.randn(64, C, device=cuda)
    ya, yb = torch.randint(0, C, (64,), device=cuda), torch.randint(0, C, (64,), device=cuda)
    lv = torch.rand(64, device=cuda)
    for lam in (lv, 0.3):
        a, b = base.clone().requires_grad_(), base.clone().requires_grad_()
        la = M.mixup_cross_entropy(a, ya, yb, lam, label_smoothing=0.0)
        lb = M.mixup_cross_entropy(b, ya, yb, lam)
        la.backward()
        lb.backward()
        assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [10, 100])
def test_smoothed_ce_fused_meter(cuda, C):
    """The fused meter accumulates the smoothed loss; the accuracy terms are those of
    ``DeviceMeter.update``.  Two steps."""
    from faster_distributed_training_amd.train.metrics import DeviceMeter
    torch.manual_seed(5)
    fused, plain = DeviceMeter(cuda), DeviceMeter(cuda)
    for step in range(2):
        logits = torch.randn(96, C, device=cuda).to(torch.bfloat16)
        logits[:8] = 0.0  # ties: argmax must pick the first index
        ya, yb = torch.randint(0, C, (96,), device=cuda), torch.randint(0, C, (96,), device=cuda)
        lv = torch.rand(96, device=cuda)
        loss = M.mixup_cross_entropy(logits, ya, yb, lv, meter=fused, label_smoothing=0.1)
        assert fused.fused
        assert abs(loss.item() - _ref(logits.float(), ya, yb, lv, 0.1).item()) < 1e-4
        fused.update(loss, logits, ya, yb, lv)
        plain.update(loss, logits, ya, yb, lv)
    assert fused.steps == plain.steps == 2
    assert rel(fused.acc, plain.acc) < 1e-5, (fused.acc, plain.acc)


@pytest.mark.gpu
def test_criterion_smoothing_is_honoured_gpu(cuda):
    torch.manual_seed(6)
    logits = torch.randn(64, 100, device=cuda)
    ya, yb = torch.randint(0, 100, (64,), device=cuda), torch.randint(0, 100, (64,), device=cuda)
    crit = nn.CrossEntropyLoss(label_smoothing=0.1)
    got = M.mixup_criterion(crit, logits, ya, yb, 0.3)
    ref = 0.3 * crit(logits, ya) + 0.7 * crit(logits, yb)
    assert abs(got.item() - ref.item()) < 1e-5
    assert abs(got.item() - M.mixup_criterion(None, logits, ya, yb, 0.3).item()) > 1e-3

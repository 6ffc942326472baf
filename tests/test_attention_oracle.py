"""CPU tests of the helpers in ``attention_oracle.py`` that ``test_attention_edges.py`` judges
the HIP attention kernels with: the oracle against autograd, the dropout read-out against a
known mask, and the per-row error against the corruptions a global norm lets through."""
import pytest
import torch

import attention_oracle as ao


def _inputs(B, L, H, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, L, H, 64, generator=g).bfloat16() for _ in range(4)]


def _close(a, b, tol=1e-12):
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("kind", ["none", "trailing", "fill"])
def test_oracle_matches_reference_fp64(kind, monkeypatch):
    """oracle == attention_reference in fp64, forward and autograd gradients (no fully masked row:
    there the two differ by definition).  attention_reference casts its scores to fp32 for the
    softmax whatever the input type, which alone costs 1e-7: for the 1e-12 comparison that one
    cast is made a no-op, so the reference really runs in fp64; as it stands it must agree to
    what an fp32 softmax allows."""
    from faster_distributed_training_amd.ops.attention import attention_reference
    B, L, H = 2, 70, 3
    q, k, v, go = _inputs(B, L, H, 1)
    mask, fill = None, None
    if kind != "none":
        mask = (torch.arange(L)[None, :] < torch.tensor([L, 9])[:, None]).long()
        fill = -1e-9 if kind == "fill" else None
    got = ao.oracle(q, k, v, mask, fill, go=go)

    def reference():
        ts = [t.double().requires_grad_() for t in (q, k, v)]
        ref = attention_reference(*ts, mask, 0.0, fill)
        ref.backward(go.double())
        return [ref.detach()] + [t.grad for t in ts]

    for a, b in zip(got, reference()):
        _close(a, b, 1e-6)
    monkeypatch.setattr(torch.Tensor, "float", lambda self: self)
    for a, b in zip(got, reference()):
        _close(a, b, 1e-12)


def test_oracle_with_keep_matches_autograd():
    B, L, H, p = 2, 70, 2, 0.3
    q, k, v, go = _inputs(B, L, H, 2)
    mask = (torch.arange(L)[None, :] < torch.tensor([L, 40])[:, None]).long()
    keep = torch.rand(B, H, L, L, generator=torch.Generator().manual_seed(3)) >= p
    ts = [t.double().requires_grad_() for t in (q, k, v)]
    Q, K, V = (t.transpose(1, 2) for t in ts)
    S = (Q @ K.transpose(-1, -2) / 8.0).masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    O = ((torch.softmax(S, -1) * keep / (1 - p)) @ V).transpose(1, 2)
    O.backward(go.double())
    got = ao.oracle(q, k, v, mask, None, keep=keep, p=p, go=go)
    for a, b in zip(got, [O.detach()] + [t.grad for t in ts]):
        _close(a, b)


def test_oracle_fully_masked_row_is_zero():
    q, k, v, go = _inputs(2, 5, 1, 4)
    mask = torch.tensor([[1, 1, 0, 1, 1], [0, 0, 0, 0, 0]])
    O, dQ, dK, dV = ao.oracle(q, k, v, mask, None, go=go)
    for t in (O, dQ, dK, dV):
        assert torch.isfinite(t).all() and (t[1] == 0).all() and (t[0] != 0).any()


def test_recover_pdrop_returns_the_mask():
    """A torch stand-in for the forward with a known keep mask: the read-out returns exactly the
    dropped probabilities, so exactly that mask, also where L is no multiple of 64."""
    B, L, H, p = 2, 150, 2, 0.4
    q, k, _, _ = _inputs(B, L, H, 5)
    keep = torch.rand(B, H, L, L, generator=torch.Generator().manual_seed(6)) >= p
    calls = []

    def fwd(q, k, v):
        calls.append(torch.initial_seed())
        return ao.oracle(q, k, v, None, None, keep=keep, p=p)

    Pd = ao.recover_pdrop(fwd, q.double(), k.double(), L, seed=17)
    assert Pd.shape == (B, H, L, L) and calls == [17, 17, 17]
    assert torch.equal(Pd != 0, keep)
    P = torch.softmax(q.double().transpose(1, 2) @ k.double().transpose(1, 2).transpose(-1, -2) / 8.0, -1)
    _close(Pd, P * keep / (1 - p))


def _global_rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def test_row_err_sees_what_a_global_norm_misses():
    """One row replaced by its neighbour, or one element of one row negated, at B=1, L=512, H=8:
    the per-row budget (2 x the bf16 arm's own error) fails, the global relative norm of the
    same tensor stays under the 2e-2 the older test allows.  The corrupted row and its neighbour
    (next position, same head) are the smallest such pair of the tensor, the kind either measure
    sees least: a row of average size swapped for its neighbour moves the global norm by
    sqrt(2 / 4096) = 2.2e-2, on top of the arm's own 4.5e-3, and would sit right at that bound."""
    B, L, H = 1, 512, 8
    q, k, v, go = _inputs(B, L, H, 7)
    ref = ao.oracle(q, k, v, None, None, go=go)
    arm = ao.bf16_arm(q, k, v, None, None, go=go)
    for name, a, r in zip("O dQ dK dV".split(), arm, ref):
        budget = ao.BUDGET * ao.row_err(a, r)
        assert 0 < budget < 0.1, (name, budget)
        n = r[0].norm(dim=-1)                                   # (L, H) row norms
        pair = torch.maximum(n[:-1], n[1:])
        i, h = (int(t) for t in (pair == pair.min()).nonzero()[0])
        swapped = a.clone()
        swapped[0, i, h] = a[0, i + 1, h]
        negated = a.clone()
        j = r[0, i, h].abs().argmax()
        negated[0, i, h, j] = -a[0, i, h, j]
        for bad in (swapped, negated):
            assert ao.row_err(bad, r) > budget, name
            assert _global_rel(bad, r) < 2e-2, name
            ok, _ = ao.budget_report(name, bad, a, r)
            assert not ok


def test_budget_report_zero_reference():
    """dQ, dK at L = 1 are exactly zero: the check falls back to an absolute bound from dV."""
    q, k, v, go = _inputs(2, 1, 3, 8)
    O, dQ, dK, dV = ao.oracle(q, k, v, None, None, go=go)
    assert not (dQ != 0).any() and not (dK != 0).any()
    lim = 1e-3 * ao.rms_row_norm(dV)
    small = torch.full_like(dQ, 0.5 * lim / 8.0)
    assert ao.budget_report("dQ", small, dQ, dQ, dV)[0]
    assert not ao.budget_report("dQ", small * 4, dQ, dQ, dV)[0]
    assert not ao.budget_report("dQ", torch.full_like(dQ, float("nan")), dQ, dQ, dV)[0]
    assert ao.row_err(torch.full_like(O, float("nan")), O) == float("inf")

"""fp64 oracle, bf16 yardstick and per-row error for the attention tests.

Nothing here touches a project kernel: ``oracle`` is the explicit fp64 arithmetic of
softmax(q k^T / 8, key mask) -> keep mask -> @ v and its gradients, ``bf16_arm`` is the same
composition in plain bf16 torch ops through autograd (what PyTorch itself would lose to
rounding), and ``row_err`` compares one (b, position, head) row of 64 at a time, so one
wrong row cannot hide in a global norm.

Layouts: q, k, v, go and every result are (B, L, H, 64); mask is (B, L) with nonzero = keep;
``keep`` (the dropout keep mask) is (B, H, Lq, Lk).
"""
from __future__ import annotations

import torch

D = 64
BUDGET = 2.0  # kernel row error <= BUDGET x the bf16 arm's row error (README round 3 item 9)


def _bhld(t, dtype):
    return t.detach().to(torch.bfloat16).to(dtype).transpose(1, 2)


def oracle(q, k, v, mask, fill, keep=None, p=0.0, go=None):
    """fp64 attention on the bf16-rounded inputs.  ``fill`` None = true masking (-inf); a
    fully masked row is defined as P = 0 (output 0).  A masked key passes no gradient to its
    score, whatever the fill.  Returns O, or (O, dQ, dK, dV) when ``go`` is given."""
    Q, K, V = (_bhld(t, torch.float64) for t in (q, k, v))
    S = Q @ K.transpose(-1, -2) / 8.0
    live = None
    if mask is not None:
        live = (mask != 0)[:, None, None, :]
        S = S.masked_fill(~live, float("-inf") if fill is None else float(fill))
    m = S.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    P = E / torch.where(l > 0, l, torch.ones_like(l))
    z = None if keep is None else keep.to(torch.float64) / (1.0 - p)
    Pd = P if z is None else P * z
    O = Pd @ V
    if go is None:
        return O.transpose(1, 2)
    dO = _bhld(go, torch.float64)
    dV = Pd.transpose(-1, -2) @ dO
    dPd = dO @ V.transpose(-1, -2)
    delta = (dO * O).sum(-1, keepdim=True)
    dS = P * ((dPd if z is None else dPd * z) - delta)
    if live is not None:
        dS = dS * live
    dQ = dS @ K / 8.0
    dK = dS.transpose(-1, -2) @ Q / 8.0
    return tuple(t.transpose(1, 2) for t in (O, dQ, dK, dV))


def bf16_arm(q, k, v, mask, fill, keep=None, p=0.0, go=None):
    """The same operation in plain bf16 torch ops through autograd, on the inputs' device:
    bf16 matmul, masked_fill, fp32 softmax cast back to bf16, the given keep mask, bf16
    matmul.  Returns O, or (O, dQ, dK, dV) when ``go`` is given."""
    ts = [t.detach().to(torch.bfloat16).clone().requires_grad_(go is not None) for t in (q, k, v)]
    Q, K, V = (t.transpose(1, 2) for t in ts)
    S = torch.matmul(Q, K.transpose(-1, -2)) / 8.0
    if mask is not None:
        S = S.masked_fill(mask[:, None, None, :] == 0, torch.finfo(S.dtype).min if fill is None else float(fill))
    P = torch.softmax(S.float(), dim=-1).to(torch.bfloat16)
    if keep is not None:
        P = P * keep.to(torch.bfloat16) * (1.0 / (1.0 - p))
    O = torch.matmul(P, V).transpose(1, 2)
    if go is None:
        return O.detach()
    O.backward(go.detach().to(torch.bfloat16))
    return (O.detach(),) + tuple(t.grad for t in ts)


def _rows(t):
    return t.detach().to(torch.float64).reshape(-1, t.shape[-1])


def rms_row_norm(ref) -> float:
    return _rows(ref).pow(2).sum(-1).mean().sqrt().item()


def row_err(x, ref) -> float:
    """max over rows of ||x - ref|| / (||ref|| + 1e-3 rms_row_norm(ref)); a row is the last
    axis (64 values of one (b, position, head)).  Non-finite x gives inf."""
    x, ref = _rows(x), _rows(ref)
    if not torch.isfinite(x).all():
        return float("inf")
    den = ref.norm(dim=-1) + 1e-3 * ref.pow(2).sum(-1).mean().sqrt()
    return ((x - ref).norm(dim=-1) / den).max().item()


def max_row_norm(x) -> float:
    x = _rows(x)
    return float("inf") if not torch.isfinite(x).all() else x.norm(dim=-1).max().item()


def budget_report(name, got, arm, ref, dv_ref=None):
    """(ok, text) of the budget: row_err(got, ref) <= BUDGET * row_err(arm, ref).  Where ``ref``
    is all zero (dQ, dK at L = 1) the check is max row ||got|| <= 1e-3 rms_row_norm(dv_ref)."""
    if not bool((ref != 0).any()):
        n, lim = max_row_norm(got), 1e-3 * rms_row_norm(dv_ref)
        return n <= lim, f"{name}: zero reference, max row norm {n:.3e} (limit {lim:.3e})"
    e, a = row_err(got, ref), row_err(arm, ref)
    ratio = e / a if a > 0 else (0.0 if e == 0 else float("inf"))
    return e <= BUDGET * a, f"{name}: kernel {e:.3e} arm {a:.3e} ratio {ratio:.3f}"


def recover_pdrop(fwd, q, k, L, seed):
    """The dropped probabilities P_drop (B, H, L, L) of ``fwd(q, k, v) -> (B, L, H, 64)``, read
    out 64 keys at a time with V_c[key] = e_{key - 64c} (zero outside chunk c).  The CPU default
    generator is re-seeded before every call: a forward that draws its dropout seed from it
    (the native wrapper does) then repeats the same mask in every chunk."""
    B, _, H, _ = q.shape
    cols = []
    for c in range((L + D - 1) // D):
        n = min(D, L - D * c)
        v = torch.zeros(B, L, H, D, device=q.device, dtype=q.dtype)
        v[:, D * c:D * c + n] = torch.eye(D, device=q.device, dtype=q.dtype)[:n, None, :]
        torch.manual_seed(seed)
        cols.append(fwd(q, k, v).detach()[..., :n])
    return torch.cat(cols, -1).permute(0, 2, 1, 3)

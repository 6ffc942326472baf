"""fp64 oracles and a host replica of the dropout hash for the transformer's pointwise kernels
(layernorm.hip, dropout.hip, embedding.hip, mlp.hip).

Nothing here touches a project kernel.  Every oracle is the explicit fp64 arithmetic of the
operation (no autograd) on the inputs as the kernel receives them, already rounded to their
dtype; ``keep_mask`` recomputes ``dropout_math.h`` (drop_hash, keep8, the threshold) in numpy
uint64 with wrap-around, so a dropout test knows every kept position without reading it back
from the kernel's output.  The per-row error is attention_oracle's.

Summation bounds: a kernel that adds k fp32 terms into a destination is held to
``sum_bound(k, mag)`` = (k + 8) 2^-24 mag, where mag is the sum of the magnitudes of everything
that enters the sum (the destination's earlier content is one of the terms: the last add rounds
relative to it too).  The oracles return those magnitudes next to the sums.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from attention_oracle import BUDGET, rms_row_norm, row_err  # noqa: F401  (re-exported)

EPS24 = 2.0 ** -24


def f64(t):
    return t.detach().to(torch.float64)


def sum_bound(k, mag):
    """|fp32 sum of k terms - exact| <= (k + 8) 2^-24 sum|terms| (8: the roundings of a term's own
    arithmetic and of the partial-sum folds)."""
    return (k + 8) * EPS24 * mag


# ---------------------------------------------------------------- LayerNorm
def ln_oracle(x, a, b, eps, gy=None, gres=None):
    """y = a (x - mean) / (std_unbiased + eps) + b over the last axis of x [rows, d], in fp64.
    Returns a namespace with y, mean [rows], rstd = 1 / (std + eps) [rows]; with ``gy`` also dx
    (plus ``gres`` when given), dgamma, dbeta [d] and their term magnitudes mag_gamma, mag_beta.

    mag_gamma: a term of dgamma is gy r (x - mean), and the kernel's x - mean carries the
    rounding of an fp32 mean of the row (relative to the row's mean |x|, not to x - mean), so the
    magnitude of a term is |gy| r (|x - mean| + mean_row |x|).  With |gy z| alone no fp32
    evaluation meets the summation bound in a column where x is close to the row's mean (the fp32
    torch reference does not: test_pointwise_oracle.py::test_ln_dgamma_magnitude)."""
    X, A, B = f64(x), f64(a), f64(b)
    d = X.shape[-1]
    mean = X.mean(-1, keepdim=True)
    xc = X - mean
    std = (xc.pow(2).sum(-1, keepdim=True) / (d - 1)).sqrt()
    r = 1.0 / (std + eps)
    z = xc * r
    out = SimpleNamespace(y=A * z + B, mean=mean.squeeze(-1), rstd=r.squeeze(-1))
    if gy is None:
        return out
    G = f64(gy)
    ga = A * G
    s1 = ga.sum(-1, keepdim=True)
    s2 = (ga * xc).sum(-1, keepdim=True)
    dx = r * (ga - s1 / d) - r * r * s2 * xc / ((d - 1) * std)
    out.dx = dx if gres is None else dx + f64(gres)
    out.dgamma = (G * z).sum(0)
    out.dbeta = G.sum(0)
    out.mag_gamma = (G.abs() * r * (xc.abs() + X.abs().mean(-1, keepdim=True))).sum(0)
    out.mag_beta = G.abs().sum(0)
    return out


# ---------------------------------------------------------------- dropout hash
_M1 = np.uint64(0xFF51AFD7ED558CCD)
_M2 = np.uint64(0xC4CEB9FE1A85EC53)
_S33 = np.uint64(33)
_MASK64 = (1 << 64) - 1


def drop_hash(i, seed):
    """dropout_math.h drop_hash on a uint64 array of counters."""
    with np.errstate(over="ignore"):
        x = np.asarray(i, dtype=np.uint64) ^ np.uint64(seed & _MASK64)
        x = x ^ (x >> _S33)
        x = x * _M1
        x = x ^ (x >> _S33)
        x = x * _M2
        x = x ^ (x >> _S33)
    return x


def threshold(p) -> int:
    """dropout.hip threshold(): p arrives as a float, the product is taken in double."""
    p32 = float(np.float32(p))
    assert 0.0 <= p32 < 1.0
    return int(min(p32 * 4294967296.0, 4294967295.0))


def drop_scale(p) -> float:
    """1.f / (1.f - p) as the launchers compute it, in fp32."""
    one = np.float32(1.0)
    return float(one / (one - np.float32(p)))


def keep_mask(n, seed, p, device_word=0):
    """Boolean numpy array [n]: element e is kept.  keep8: element 8c + 2j takes the low half of
    hash 4c + j and element 8c + 2j + 1 the high half, so element e takes half e % 2 of hash
    e // 2; kept iff that half >= threshold(p).  The live seed is seed ^ device_word."""
    s = (int(seed) ^ int(device_word)) & _MASK64
    h = drop_hash(np.arange((n + 1) // 2, dtype=np.uint64), s)
    halves = np.stack([h & np.uint64(0xFFFFFFFF), h >> np.uint64(32)], axis=1).reshape(-1)[:n]
    return halves >= np.uint64(threshold(p))


def keep_mask_t(shape, seed, p, device, device_word=0):
    n = int(np.prod(shape))
    return torch.from_numpy(keep_mask(n, seed, p, device_word)).view(*shape).to(device)


# ---------------------------------------------------------------- GELU
_INV_SQRT2 = 1.0 / math.sqrt(2.0)
_INV_SQRT2PI = 1.0 / math.sqrt(2.0 * math.pi)


def gelu(a):
    A = f64(a)
    return 0.5 * A * (1.0 + torch.erf(A * _INV_SQRT2))


def gelu_grad(a):
    A = f64(a)
    return 0.5 * (1.0 + torch.erf(A * _INV_SQRT2)) + A * _INV_SQRT2PI * torch.exp(-0.5 * A * A)


def bf16_ulp(v):
    """Spacing of bf16 at |v| (fp64 tensor): 2^(floor(log2 |v|) - 7), the subnormal spacing below
    2^-126."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


# ---------------------------------------------------------------- embedding
def emb_oracle(ids, types, pos_ids, tok, pos, seg, scale, g=None):
    """out[b, l] = (tok[ids[b, l]] + pos[pos_ids[l]] + seg[types[b, l]]) * scale in fp64, and
    mag = (|t| + |p| + |s|) * scale.  With ``g`` [B, L, d] also, for each table, the index_add_
    gradient, the per-element sum |g * scale| and the per-row contribution count."""
    B, L = ids.shape
    T, P, S = f64(tok), f64(pos), f64(seg)
    ii, tt = ids.long().reshape(-1), types[:, :L].long().reshape(-1)
    pp = pos_ids[:L].long().repeat(B)
    t, p, s = T[ii], P[pp], S[tt]
    d = T.shape[1]
    res = SimpleNamespace(out=((t + p + s) * scale).view(B, L, d),
                          mag=((t.abs() + p.abs() + s.abs()) * scale).view(B, L, d))
    if g is None:
        return res
    gs = f64(g).reshape(B * L, d) * scale
    for name, table, idx in (("tok", T, ii), ("pos", P, pp), ("seg", S, tt)):
        grad = torch.zeros_like(table).index_add_(0, idx, gs)
        mag = torch.zeros_like(table).index_add_(0, idx, gs.abs())
        cnt = torch.zeros(table.shape[0], dtype=torch.float64, device=table.device)
        cnt.index_add_(0, idx, torch.ones_like(idx, dtype=torch.float64))
        setattr(res, name, SimpleNamespace(grad=grad, mag=mag, count=cnt))
    return res


# ---------------------------------------------------------------- column and slab sums
def colsum_oracle(x):
    """(sum over rows, sum over rows of |x|) of x [rows, cols] in fp64."""
    X = f64(x)
    return X.sum(0), X.abs().sum(0)


def slabsum_oracle(src, n):
    """(sum_j src[j, :n], sum_j |src[j, :n]|) of src [s, ld] in fp64."""
    X = f64(src)[:, :n]
    return X.sum(0), X.abs().sum(0)


# ---------------------------------------------------------------- MLP
def mlp_oracle(X, W1, b1, W2, b2, g=None, bias_grad_mean=False):
    """Linear -> ReLU -> Linear in fp64 on the given (dtype-rounded) tensors; with ``g`` the
    gradients (gX, gW1, gb1, gW2, gb2) too, the bias gradients divided by the row count when
    ``bias_grad_mean``.  gpre is 0 wherever pre <= 0."""
    x, w1, w2 = f64(X), f64(W1), f64(W2)
    pre = x @ w1.t()
    if b1 is not None:
        pre = pre + f64(b1).reshape(1, -1)
    act = pre.clamp_min(0.0)
    out = act @ w2.t()
    if b2 is not None:
        out = out + f64(b2).reshape(1, -1)
    res = SimpleNamespace(out=out, pre=pre)
    if g is None:
        return res
    G = f64(g)
    k = 1.0 / x.shape[0] if bias_grad_mean else 1.0
    gpre = (G @ w2) * (pre > 0)
    res.gW2 = G.t() @ act
    res.gb2 = None if b2 is None else G.sum(0) * k
    res.gW1 = gpre.t() @ x
    res.gb1 = None if b1 is None else gpre.sum(0) * k
    res.gX = gpre @ w1
    res.gpre = gpre
    return res

"""CPU tests of the helpers in ``pointwise_oracle.py`` that ``test_pointwise_edges.py`` judges the
LayerNorm, dropout, embedding and MLP kernels with: each explicit fp64 oracle against fp64
autograd of the project's reference composition, and the dropout hash replica against the
properties of ``dropout_math.h`` that a wrong replica (or a wrong kernel) would break."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_oracle as po


def _close(a, b, tol=1e-10):
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("rows,d", [(1, 64), (5, 192), (9, 512)])
@pytest.mark.parametrize("with_res", [False, True])
def test_ln_oracle_matches_autograd_fp64(rows, d, with_res):
    from faster_distributed_training_amd.ops.layernorm import layer_norm_reference
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g) * 2 + 0.5
    x[0, 3] = 1e4
    a, b = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    gy, gres = torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g)
    o = po.ln_oracle(x, a, b, 1e-6, gy, gres if with_res else None)
    xs, as_, bs = (t.double().requires_grad_() for t in (x, a, b))
    ref = layer_norm_reference(xs, as_, bs, 1e-6)
    ref.backward(gy.double())
    _close(o.y, ref.detach())
    _close(o.mean, x.double().mean(-1))
    _close(o.rstd, 1.0 / (x.double().std(-1) + 1e-6))
    _close(o.dx, xs.grad + (gres.double() if with_res else 0.0))
    _close(o.dgamma, as_.grad)
    _close(o.dbeta, bs.grad)
    assert (o.mag_beta >= o.dbeta.abs()).all() and (o.mag_gamma >= o.dgamma.abs()).all()


def test_ln_dgamma_magnitude():
    """Why mag_gamma carries the row's mean |x|: with sum |gy z| alone the fp32 torch reference
    itself misses the summation bound at one row (a column where x is close to the row mean has a
    tiny term but the full rounding of the mean); with mag_gamma it meets it, and a dgamma that
    lost one row's contribution still does not."""
    from faster_distributed_training_amd.ops.layernorm import layer_norm_reference
    g = torch.Generator().manual_seed(0)
    worst_naive, worst = 0.0, 0.0
    for rows, d in ((1, 64), (1, 512), (1, 2048), (9, 512)):
        x = torch.randn(rows, d, generator=g) * 2 + 0.5
        a, b = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
        gy = torch.randn(rows, d, generator=g)
        o = po.ln_oracle(x, a, b, 1e-6, gy)
        a32 = a.clone().requires_grad_()
        layer_norm_reference(x, a32, b, 1e-6).backward(gy)
        err = (a32.grad.double() - o.dgamma).abs()
        naive = po.sum_bound(rows, (gy.double() * (x.double() - o.mean[:, None]) * o.rstd[:, None]).abs().sum(0))
        worst_naive = max(worst_naive, (err / naive).max().item())
        worst = max(worst, (err / po.sum_bound(rows, o.mag_gamma)).max().item())
        if rows > 1:  # one row's contribution dropped: far outside
            lost = o.dgamma - (gy.double() * (x.double() - o.mean[:, None]) * o.rstd[:, None])[3]
            assert ((lost - o.dgamma).abs() > po.sum_bound(rows, o.mag_gamma)).float().mean() > 0.99
    print(f"fp32 reference dgamma error / bound: naive {worst_naive:.2f}, with mean|x| {worst:.3f}")
    assert worst_naive > 1.0
    assert worst <= 1.0


@pytest.mark.parametrize("repeat_pos", [False, True])
def test_emb_oracle_matches_autograd_fp64(repeat_pos, monkeypatch):
    """embedding_sum_reference casts a token table that is not fp32 to fp32, which would cost the
    fp64 run 1e-7 in the token gradient: for this comparison that cast is made a no-op."""
    from faster_distributed_training_amd.ops.embedding import embedding_sum_reference
    monkeypatch.setattr(torch.Tensor, "float", lambda self: self)
    g = torch.Generator().manual_seed(3)
    B, L, d, vt, vp, vs = 3, 7, 16, 11, 20, 3
    tok, pos, seg = (torch.randn(v, d, generator=g) for v in (vt, vp, vs))
    ids = torch.randint(0, vt, (B, L), generator=g)
    types = torch.randint(0, vs, (B, L), generator=g)
    pos_ids = torch.arange(vp) // 2 if repeat_pos else torch.arange(vp)
    go = torch.randn(B, L, d, generator=g)
    go[1, 2] = 0.0
    o = po.emb_oracle(ids, types, pos_ids, tok, pos, seg, 4.0, go)
    ws = [t.double().requires_grad_() for t in (tok, pos, seg)]
    ref = embedding_sum_reference(ids, types, pos_ids, *ws, 4.0)
    ref.backward(go.double())
    _close(o.out, ref.detach())
    for part, w in zip((o.tok, o.pos, o.seg), ws):
        _close(part.grad, w.grad)
        assert (part.mag >= part.grad.abs() - 1e-12).all()
    assert o.tok.count.sum().item() == o.pos.count.sum().item() == o.seg.count.sum().item() == B * L
    assert o.pos.count[0].item() == (2 * B if repeat_pos else B)


def test_gelu_and_sums():
    a = torch.linspace(-6, 6, 241)
    ad = a.double().requires_grad_()
    ref = F.gelu(ad)
    ref.sum().backward()
    _close(po.gelu(a), ref.detach(), 1e-14)
    _close(po.gelu_grad(a), ad.grad, 1e-14)
    assert po.gelu_grad(torch.tensor([-40.0, -3e38])).tolist() == [0.0, 0.0]
    v = torch.tensor([1.0, 1.5, 2.0, 255.0, -0.75, 2.0 ** -127]).double()
    assert po.bf16_ulp(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0 ** -8, 2.0 ** -133]
    x = torch.randn(5, 8)
    s, m = po.colsum_oracle(x)
    _close(s, x.double().sum(0), 1e-15)
    _close(m, x.double().abs().sum(0), 1e-15)
    s, m = po.slabsum_oracle(x, 4)
    assert s.shape == (4,)
    _close(s, x.double()[:, :4].sum(0), 1e-15)


def test_mlp_oracle_matches_autograd_fp64():
    g = torch.Generator().manual_seed(5)
    X, W1, b1 = torch.randn(9, 6, generator=g), torch.randn(8, 6, generator=g), torch.randn(8, generator=g)
    W2, b2, go = torch.randn(4, 8, generator=g), torch.randn(4, generator=g), torch.randn(9, 4, generator=g)
    W1[2], b1[2] = 0.0, 0.0  # pre == 0 exactly: no gradient through it
    ts = [t.double().requires_grad_() for t in (X, W1, b1, W2, b2)]
    ref = F.linear(torch.relu(F.linear(ts[0], ts[1], ts[2])), ts[3], ts[4])
    ref.backward(go.double())
    o = po.mlp_oracle(X, W1, b1, W2, b2, go)
    _close(o.out, ref.detach())
    for got, t in zip((o.gX, o.gW1, o.gb1, o.gW2, o.gb2), ts):
        _close(got, t.grad)
    assert (o.gpre[:, 2] == 0).all() and (o.gW1[2] == 0).all()
    om = po.mlp_oracle(X, W1, b1, W2, b2, go, bias_grad_mean=True)
    _close(om.gb1 * 9, o.gb1)
    _close(om.gb2 * 9, o.gb2)


# ---------------------------------------------------------------- dropout hash replica
def _hash_scalar(i, seed):
    """drop_hash with Python integers (independent of the numpy code path)."""
    m = (1 << 64) - 1
    x = (i ^ seed) & m
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & m
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & m
    x ^= x >> 33
    return x


def test_keep_mask_follows_the_hash():
    seed, n = (0xABCDEF << 40) | 12345, 64
    h = po.drop_hash(np.arange(n // 2, dtype=np.uint64), seed)
    assert [int(v) for v in h] == [_hash_scalar(i, seed) for i in range(n // 2)]
    assert po.threshold(0.0) == 0 and po.threshold(0.5) == 1 << 31
    assert po.threshold(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32)
    assert po.drop_scale(0.5) == 2.0 and po.drop_scale(0.0) == 1.0
    assert po.drop_scale(0.999) == float(np.float32(1) / (np.float32(1) - np.float32(0.999)))
    for p in (0.1, 0.5):
        thr = po.threshold(p)
        m = po.keep_mask(n, seed, p)
        for c in range(n // 8):  # keep8 of chunk c
            for j in range(4):
                hv = _hash_scalar(4 * c + j, seed)
                assert m[8 * c + 2 * j] == ((hv & 0xFFFFFFFF) >= thr)      # low half
                assert m[8 * c + 2 * j + 1] == ((hv >> 32) >= thr)         # high half, the adjacent element
    # an odd length is a prefix of the next even one
    assert np.array_equal(po.keep_mask(13, seed, 0.5), po.keep_mask(16, seed, 0.5)[:13])


def test_keep_mask_seed_bits():
    n = 4096
    assert po.keep_mask(n, 99, 0.0).all()
    assert po.keep_mask(n, 1 << 63, 0.0).all()
    base = po.keep_mask(n, 7, 0.5)
    for bit in (32, 45, 63):  # seed bits at or above 2^32 change the mask
        assert not np.array_equal(po.keep_mask(n, 7 | (1 << bit), 0.5), base)
    word = 0x123456789ABCDEF0
    assert np.array_equal(po.keep_mask(n, 7, 0.5, device_word=word), po.keep_mask(n, 7 ^ word, 0.5))
    assert not np.array_equal(po.keep_mask(n, 7, 0.5, device_word=word), base)
    assert np.array_equal(po.keep_mask(n, word, 0.5, device_word=word), po.keep_mask(n, 0, 0.5))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", [20240229, 0x9E3779B9 << 32])
def test_keep_mask_fraction(p, seed):
    n = 1 << 20
    m = po.keep_mask(n, seed, p)
    sigma = math.sqrt(p * (1 - p) / n)
    for name, part in (("all", m), ("low halves", m[0::2]), ("high halves", m[1::2])):
        s = sigma * math.sqrt(n / part.size)
        assert abs(part.mean() - (1 - p)) <= 5 * s, (name, part.mean(), 1 - p, s)

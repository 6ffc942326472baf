"""The transformer's pointwise HIP kernels (layernorm.hip, dropout.hip, embedding.hip, mlp.hip)
against fp64 oracles and an exact host replica of the dropout mask, at the edges of their
partitions: every instantiated LayerNorm width and dtype triple, row counts around the
wave-per-row grid and the 8-row backward blocks, the grid-stride wrap and partial column blocks
of the dropout kernels, the global-atomics segment path of the embedding backward, strided
column sums and slab sums.  Helpers: pointwise_oracle.py (tested on the CPU in
test_pointwise_oracle.py).

Conventions: kernels are called as the ops/ wrappers call them, on the current stream; every
buffer a kernel writes is longer than needed and ends in a canary of NaN bit patterns that must
come back untouched; no index is out of range; no element is left out of a comparison.

Budgets.  Per row, row_err(kernel, oracle) <= 2 x row_err(arm, oracle); the arm of a bf16 / fp16
result is the oracle rounded once to that dtype, the arm of an fp32 result is the plain fp32
torch composition on the same device, with the floor the older tests use (1e-5 forward, 1e-4
gradients) applied per row.  Sums of k fp32 terms: pointwise_oracle.sum_bound.  Dropout masks:
exact.  Every test prints the worst fraction of its limit (``WORST ...``) before it asserts.

Worst fraction of the limit measured on an MI355X over all cases of this file (0.5 = the kernel's
row error equals the arm's):
    LayerNorm  y 0.51 (fp32 in, bf16 out, 3 x 2048), dx 0.50, mean 0.006, rstd 0.02,
               dgamma 0.33 (1 x 1536 bf16), dbeta 0.20 (5 x 384, slab fold)
    dropout    dropout_add 0.97 (8388632 elements, p = 0.1), dropout_bwd 0.50, GELU 0.49,
               GELU backward 0.50; fused column sums 0.11 (1 x 256)
    embedding  forward 0.88 (d = 3072, 1 x 64), token 0.65, position 0.53, segment 0.47
    mlp.hip    fused_mlp 0.52 (gb1, 33 x 8 bf16), colsum_bf16 0.11, slab_sum_acc 0.23

Before the LayerNorm forward took its row sum in fp64, rows with mean 100 and standard deviation
0.01 failed y in fp32 at every width (row error 4e-4 .. 8e-4 against 2e-5 .. 2e-4 of the fp32
PyTorch formula, up to 28 x at 9 x 64) and dx at 9 x 64 (1.5e-4 against 2.3e-5).  Before
fused_mlp passed its biases to the GEMMs, out failed in bf16 and fp16 (2.1 x the arm at 32 x 8
bf16, 4.4 x at 1 x 8 fp16).  Widths 192, 320, ... raised in layer_norm_unbiased.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import pointwise_oracle as po

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT = {F32: 0, BF16: 1, F16: 2}
PAT = {4: (torch.int32, 0x7FA5A5A5), 2: (torch.int16, 0x7FA5)}  # NaN in fp32 / bf16 / fp16
TAIL = 512


def _nat():
    from faster_distributed_training_amd.ops import _native
    return _native.native(), _native.stream_ptr()


class _Buf:
    """A tensor of ``shape`` at the head of a longer buffer whose every element starts as a NaN
    bit pattern; ``init`` (a tensor) overwrites the head.  ``tail_ok()``: the canary behind the
    head is bitwise untouched; ``written()``: no element of the head still has the pattern."""

    def __init__(self, shape, dtype, device, init=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.n = math.prod(shape)
        self.idt, self.pat = PAT[torch.empty(0, dtype=dtype).element_size()]
        self.raw = torch.full((self.n + TAIL,), self.pat, dtype=self.idt, device=device)
        self.t = self.raw[:self.n].view(dtype).view(*shape)
        if init is not None:
            self.t.copy_(init)

    def ptr(self):
        return self.t.data_ptr()

    def tail_ok(self):
        return bool((self.raw[self.n:] == self.pat).all())

    def written(self):
        return bool((self.raw[:self.n] != self.pat).all())

    def bits(self):
        return self.raw[:self.n]


class _Worst:
    """Largest fraction of a limit seen per family, with the case it came from."""

    def __init__(self):
        self.w = {}

    def note(self, fam, frac, tag):
        if fam not in self.w or frac > self.w[fam][0]:
            self.w[fam] = (frac, tag)

    def report(self, head):
        for fam, (frac, tag) in sorted(self.w.items()):
            print(f"WORST {head} {fam}: {frac:.3f} of the limit at {tag}")


def _budget(worst, bad, fam, tag, got, arm, ref, floor=0.0):
    """row_err(got) <= max(2 x row_err(arm), floor)."""
    e, a = po.row_err(got, ref), po.row_err(arm, ref)
    lim = max(po.BUDGET * a, floor)
    frac = e / lim if lim > 0 else (0.0 if e == 0 else float("inf"))
    worst.note(fam, frac, f"{tag} (kernel {e:.3e} arm {a:.3e})")
    if not e <= lim:
        bad.append(f"{fam} {tag}: kernel {e:.3e} arm {a:.3e} limit {lim:.3e}")


def _within(worst, bad, fam, tag, got, ref, bound):
    """|got - ref| <= bound elementwise (fp64 tensors); where bound is 0 the match is exact."""
    err = (po.f64(got) - ref).abs()
    inf = torch.full_like(err, float("inf"))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(po.f64(got)), ratio, inf).reshape(-1)
    frac = ratio.max().item()
    worst.note(fam, frac, tag)
    if not frac <= 1.0:
        i = int(ratio.argmax())
        bad.append(f"{fam} {tag}: {frac:.3f} of the bound at flat index {i} of {ratio.numel()} "
                   f"(got {po.f64(got).reshape(-1)[i].item():.9e} want {ref.reshape(-1)[i].item():.9e})")


# ================================================================= LayerNorm
from faster_distributed_training_amd.ops.layernorm import NATIVE_WIDTHS  # noqa: E402

LN_ROWS = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33)
LN_TRIPLES = ((F32, F32, F32), (F32, BF16, BF16), (BF16, BF16, BF16), (F16, F16, F16))  # x, y, gy
EPS = 1e-6


def _ln_inputs(rows, d, tx, tg, seed, device):
    """x = randn * 2 + 0.5 with one outlier of 1e4 in the last row; for fp32 x and >= 3 rows, row
    1 has mean 100 and standard deviation 0.01 (a one-pass variance loses it)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, generator=g) * 2 + 0.5
    if tx == F32 and rows >= 3:
        x[1] = 100.0 + 0.01 * torch.randn(d, generator=g)
    x[rows - 1, (7 * rows) % d] = 1e4
    a = torch.rand(d, generator=g) + 0.5
    b = torch.randn(d, generator=g)
    gy = torch.randn(rows, d, generator=g)
    gres = torch.randn(rows, d, generator=g)
    return (x.to(device, tx), a.to(device), b.to(device), gy.to(device, tg), gres.to(device, tx))


def _ln_nblk(rows):
    return max(1, min(2048, (rows + 7) // 8))  # ops/layernorm.py _LayerNormNative.backward


def _ln_fp32_arm(x, a, b, gy, gres):
    """layer_norm_reference and its autograd in fp32 on the device."""
    from faster_distributed_training_amd.ops.layernorm import layer_norm_reference
    xs, as_, bs = (t.detach().float().clone().requires_grad_() for t in (x, a, b))
    y = layer_norm_reference(xs, as_, bs, EPS)
    y.backward(gy.float())
    xf = x.detach().float()
    return dict(y=y.detach(), dx=xs.grad, dx_res=xs.grad + gres.float(), mean=xf.mean(-1),
                rstd=1.0 / (xf.std(-1) + EPS))


def _ln_check(worst, bad, tag, x, a, b, gy, gres, ty, got):
    """Budgets of one LayerNorm case.  ``got``: y, mean, rstd, dx, dx_res, dgamma / dbeta pairs."""
    o = po.ln_oracle(x, a, b, EPS, gy)
    arm = _ln_fp32_arm(x, a, b, gy, gres)
    rows = x.shape[0]
    yarm, yfloor = (arm["y"], 1e-5) if ty == F32 else (o.y.to(ty), 0.0)
    _budget(worst, bad, f"y[{ty}]", tag, got["y"], yarm, o.y, yfloor)
    _budget(worst, bad, "mean", tag, got["mean"][:, None], arm["mean"][:, None], o.mean[:, None], 1e-5)
    _budget(worst, bad, "rstd", tag, got["rstd"][:, None], arm["rstd"][:, None], o.rstd[:, None], 1e-5)
    for key, ref in (("dx", o.dx), ("dx_res", o.dx + po.f64(gres))):
        if key in got:
            darm, dfloor = (arm[key], 1e-4) if x.dtype == F32 else (ref.to(x.dtype), 0.0)
            _budget(worst, bad, f"{key}[{x.dtype}]", tag, got[key], darm, ref, dfloor)
    for name, dg, db, extra in got["grads"]:  # extra: magnitude of what the destination held
        _within(worst, bad, f"dgamma {name}", tag, dg, o.dgamma, po.sum_bound(rows, o.mag_gamma + extra[0]))
        _within(worst, bad, f"dbeta {name}", tag, db, o.dbeta, po.sum_bound(rows, o.mag_beta + extra[1]))


def _ln_direct(x, a, b, gy, gres, ty):
    """Forward, backward without and with gres, and the three folds of the partials, as
    _LayerNormNative calls them; all outputs in canary buffers."""
    nat, sp = _nat()
    rows, d = x.shape
    dev = x.device
    y, mean, rstd = _Buf((rows, d), ty, dev), _Buf(rows, F32, dev), _Buf(rows, F32, dev)
    nat.layernorm_fwd(x.data_ptr(), a.data_ptr(), b.data_ptr(), y.ptr(), mean.ptr(), rstd.ptr(), rows, d, EPS,
                      DT[x.dtype], DT[ty], DT[a.dtype], sp)
    nblk = _ln_nblk(rows)
    bufs = [y, mean, rstd]
    out = {}
    for key, res in (("dx", None), ("dx_res", gres)):
        gx, part = _Buf((rows, d), x.dtype, dev), _Buf((nblk, 2, d), F32, dev)
        nat.layernorm_bwd(gy.data_ptr(), x.data_ptr(), a.data_ptr(), mean.ptr(), rstd.ptr(), gx.ptr(),
                          0 if res is None else res.data_ptr(), part.ptr(), rows, d, nblk, DT[gy.dtype],
                          DT[x.dtype], DT[a.dtype], EPS, sp)
        out[key] = gx.t
        bufs += [gx, part]
    # the direct-gradient folds into destinations that already hold values
    gen = torch.Generator().manual_seed(rows * 4096 + d)
    pre = torch.randn(2, d, generator=gen).to(dev)
    adj = _Buf((2, d), F32, dev, pre)  # beta's view directly behind gamma's: one call
    nat.slab_sum_acc(part.ptr(), adj.ptr(), nblk, 2 * d, 2 * d, sp)
    ta, tb = _Buf(d, F32, dev, pre[0]), _Buf(d, F32, dev, pre[1])  # apart: one call each
    nat.slab_sum_acc(part.ptr(), ta.ptr(), nblk, 2 * d, d, sp)
    nat.slab_sum_acc(part.ptr() + d * 4, tb.ptr(), nblk, 2 * d, d, sp)
    bufs += [adj, ta, tb]
    p64, zero = po.f64(pre), torch.zeros(d, dtype=torch.float64, device=dev)
    sums = part.t.sum(0)
    out.update(y=y.t, mean=mean.t, rstd=rstd.t, grads=[
        ("part.sum", sums[0], sums[1], (zero, zero)),
        ("slab adjacent", po.f64(adj.t[0]) - p64[0], po.f64(adj.t[1]) - p64[1], p64.abs()),
        ("slab apart", po.f64(ta.t) - p64[0], po.f64(tb.t) - p64[1], p64.abs())])
    torch.cuda.synchronize()
    for i, buf in enumerate(bufs):
        assert buf.tail_ok(), f"buffer {i}: canary overwritten"
        assert buf.written(), f"buffer {i}: elements never written"
    return out, part.t


def _ln_wrapper(x, a, b, gy, gres, ty):
    """The same through _LayerNormNative and autograd (gres handed over as dropout_add does)."""
    from faster_distributed_training_amd.ops.layernorm import ResidualGrad, _LayerNormNative
    xs, as_, bs = (t.detach().clone().requires_grad_() for t in (x, a, b))
    res = ResidualGrad()
    y = _LayerNormNative.apply(xs, as_, bs, EPS, ty, res)
    assert res.armed
    res.g = gres
    y.backward(gy)
    return y.detach(), xs.grad, as_.grad, bs.grad


def _ln_case(worst, bad, rows, d, triple, device):
    tx, ty, tg = triple
    x, a, b, gy, gres = _ln_inputs(rows, d, tx, tg, 1000 * d + rows, device)
    tag = f"rows={rows} d={d} x={tx} y={ty} gy={tg}".replace("torch.", "")
    got, part = _ln_direct(x, a, b, gy, gres, ty)
    _ln_check(worst, bad, tag, x, a, b, gy, gres, ty, got)
    wy, wdx, wda, wdb = _ln_wrapper(x, a, b, gy, gres, ty)
    sums = part.sum(0)
    for name, p, q in (("y", wy, got["y"]), ("dx", wdx, got["dx_res"]), ("dgamma", wda, sums[0]), ("dbeta", wdb, sums[1])):
        if not torch.equal(p, q):
            bad.append(f"{tag}: _LayerNormNative's {name} is not the direct call's")
    return part


@pytest.mark.parametrize("d", NATIVE_WIDTHS)
def test_layernorm_rows_and_dtypes(cuda, d):
    """Every dtype triple and row count at one instantiated width: y, mean, rstd, dx (with and
    without the residual gradient) per row, dgamma / dbeta per column through all three folds."""
    worst, bad = _Worst(), []
    for triple in LN_TRIPLES:
        for rows in LN_ROWS:
            _ln_case(worst, bad, rows, d, triple, cuda)
    worst.report(f"layernorm d={d}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("triple", LN_TRIPLES, ids=["f32", "train", "bf16", "f16"])
def test_layernorm_capped_partition(cuda, triple):
    """16385 rows at d = 64: nblk is capped at 2048, 9 rows per block, and the last 227 blocks
    have no rows; their partials must be written as zeros (the folds read all 2048)."""
    rows, d = 16385, 64
    assert _ln_nblk(rows) == 2048 and -(-rows // 2048) == 9
    worst, bad = _Worst(), []
    part = _ln_case(worst, bad, rows, d, triple, cuda)
    first_empty = -(-rows // 9)
    assert first_empty < 2048 and (part[first_empty:] == 0).all()
    worst.report("layernorm capped")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("d", range(64, 2049, 64))
def test_layernorm_width_gate(cuda, d):
    """layer_norm_unbiased serves every multiple of 64 up to 2048 (the kernel for NATIVE_WIDTHS,
    the PyTorch formula otherwise), forward and backward, within the budgets."""
    from faster_distributed_training_amd.ops.layernorm import layer_norm_unbiased
    rows = 5
    x, a, b, gy, gres = _ln_inputs(rows, d, F32, F32, 77 + d, cuda)
    xs, as_, bs = (t.detach().clone().requires_grad_() for t in (x, a, b))
    y = layer_norm_unbiased(xs, as_, bs, EPS)
    y.backward(gy)
    o = po.ln_oracle(x, a, b, EPS, gy)
    arm = _ln_fp32_arm(x, a, b, gy, gres)
    worst, bad = _Worst(), []
    tag = f"d={d}"
    _budget(worst, bad, "y", tag, y.detach(), arm["y"], o.y, 1e-5)
    _budget(worst, bad, "dx", tag, xs.grad, arm["dx"], o.dx, 1e-4)
    _within(worst, bad, "dgamma", tag, as_.grad, o.dgamma, po.sum_bound(rows, o.mag_gamma))
    _within(worst, bad, "dbeta", tag, bs.grad, o.dbeta, po.sum_bound(rows, o.mag_beta))
    worst.report("layernorm gate")
    assert not bad, "\n".join(bad)


# ================================================================= dropout
SEEDS = ((20240229, 0), (0x9E3779B9 << 32, 0), (0x5DEECE66D, 0x123456789ABCDEF0))  # (host seed, device word)
PS = (0.0, 0.1, 0.5, 0.999)
COLS = (8, 248, 256, 264, 520, 1032)
ROWS2D = (1, 7, 8, 9, 31, 32, 33, 65)


def _word(word, device):
    """The device seed word as the runner keeps it: one int64 on the device (0 = no pointer)."""
    return None if word == 0 else torch.tensor([word], dtype=torch.int64, device=device)


def _nonzero(shape, gen, device, dtype, lo=0.25):
    """randn pushed away from zero by ``lo``: no product with it vanishes or hides in a sum."""
    v = torch.randn(shape, generator=gen, device=device)
    return (v + torch.where(v >= 0, lo, -lo)).to(dtype)


def _gelu_input(shape, gen, device):
    """bf16 in +-[2^-6, 5]: neither gelu nor gelu' of it, times any scale here, rounds to zero
    (below -5.5 erff is -1 in fp32 and gelu a true zero, which no read-back tells from a drop)."""
    v = (torch.randn(shape, generator=gen, device=device) * 1.5).clamp(-5.0, 5.0)
    return torch.where(v.abs() < 2.0 ** -6, torch.full_like(v, 0.5), v).to(BF16)


def _drop_expect(kind, mask, scale, g=None, a=None, x=None, y=None):
    """(fp64 expectation, elementwise bound) of the four operations.  ``scale`` is the launcher's
    fp32 1 / (1 - p); the bounds are those of an fp32 evaluation followed by the one rounding of
    the stored type (the GELU terms 2^-23 |a| and 2^-20 |g| max(1, |a|) cover erff / __expf)."""
    m = mask.double()
    if kind == "add":  # one fp32 rounding of the product, one of the sum
        ys = po.f64(y) * scale * m
        return po.f64(x) + ys, 2.0 ** -23 * (po.f64(x).abs() + ys.abs())
    if kind == "bwd":  # one bf16 rounding of g * scale (itself rounded to fp32): one ulp
        e = po.f64(g) * scale * m
        return e, po.bf16_ulp(e) * m
    if kind == "gelu":  # fp32 evaluation (erff cancels in the negative tail), one bf16 rounding
        e = po.gelu(a) * scale * m
        return e, (2.0 ** -7 * e.abs() + 2.0 ** -23 * po.f64(a).abs() * scale) * m
    gs = po.f64(g) * scale * m
    e = gs * po.gelu_grad(a)
    return e, 2.0 ** -7 * e.abs() + 2.0 ** -20 * gs.abs() * po.f64(a).abs().clamp_min(1.0)


def _mask_equal(bad, tag, kept, mask):
    if not torch.equal(kept, mask):
        diff = (kept != mask).reshape(-1)
        bad.append(f"{tag}: {int(diff.sum())} of {diff.numel()} positions differ from the replica, first "
                   f"at {int(diff.nonzero()[0])}")


def _run_1d(worst, bad, n, seed, word, p, y, x, g32, a, g16):
    """The four grid-stride kernels at one (seed, device word, p); returns (gy, ga) bits."""
    nat, sp = _nat()
    dev = x.device
    wt = _word(word, dev)
    wp = 0 if wt is None else wt.data_ptr()
    mask = po.keep_mask_t((n,), seed, p, dev, word)
    scale = po.drop_scale(p)
    tag = f"n={n} seed={seed:#x} word={word:#x} p={p}"
    out, gy, h, ga = _Buf(n, F32, dev), _Buf(n, BF16, dev), _Buf(n, BF16, dev), _Buf(n, BF16, dev)
    nat.dropout_add_fwd(y.data_ptr(), x.data_ptr(), out.ptr(), n, p, seed, wp, sp)
    nat.dropout_bwd(g32.data_ptr(), gy.ptr(), n, p, seed, wp, sp)
    nat.gelu_dropout_fwd(a.data_ptr(), h.ptr(), n, p, seed, wp, sp)
    nat.gelu_dropout_bwd(g16.data_ptr(), a.data_ptr(), ga.ptr(), n, p, seed, wp, sp)
    torch.cuda.synchronize()
    for name, buf in (("dropout_add", out), ("dropout_bwd", gy), ("gelu_dropout", h), ("gelu_dropout_bwd", ga)):
        assert buf.tail_ok(), f"{name} {tag}: canary overwritten"
        assert buf.written(), f"{name} {tag}: elements never written"
    _mask_equal(bad, f"dropout_add {tag}", out.t != x, mask)
    _mask_equal(bad, f"dropout_bwd {tag}", gy.t != 0, mask)
    _mask_equal(bad, f"gelu_dropout {tag}", h.t != 0, mask)
    _mask_equal(bad, f"gelu_dropout_bwd {tag}", ga.t != 0, mask)
    for kind, got, kw in (("add", out.t, dict(x=x, y=y)), ("bwd", gy.t, dict(g=g32)), ("gelu", h.t, dict(a=a)),
                          ("gelu_bwd", ga.t, dict(g=g16, a=a))):
        ref, bound = _drop_expect(kind, mask, scale, **kw)
        _within(worst, bad, kind, tag, got, ref, bound)
    return gy, ga


@pytest.mark.parametrize("n", [8, 8 * 255, 8 * 257, 8 * (4096 * 256 + 3)])
def test_dropout_1d_masks_and_values(cuda, n):
    """dropout_add_fwd, dropout_bwd, gelu_dropout_fwd, gelu_dropout_bwd: the kept positions are
    the replica's, exactly, for seeds below 2^32, with only high bits, and XORed with a device
    word; the values are within the fp32 / bf16 rounding bounds.  The largest n wraps the
    grid-stride loop (the grid is capped at 4096 blocks of 256 lanes of 8)."""
    gen = torch.Generator(device=cuda).manual_seed(n)
    y = _nonzero(n, gen, cuda, BF16)
    x = torch.randn(n, generator=gen, device=cuda)
    g32 = _nonzero(n, gen, cuda, F32)
    g16 = _nonzero(n, gen, cuda, BF16)
    a = _gelu_input(n, gen, cuda)
    worst, bad = _Worst(), []
    for seed, word in SEEDS:
        for p in PS:
            _run_1d(worst, bad, n, seed, word, p, y, x, g32, a, g16)
    worst.report(f"dropout n={n}")
    assert not bad, "\n".join(bad)


def test_dropout_seed_bits_reach_the_kernel(cuda):
    """Masks of seeds that differ only above bit 32, or only by the device word, differ."""
    nat, sp = _nat()
    n, p = 8 * 257, 0.5
    g = torch.ones(n, device=cuda)
    masks = []
    for seed, word in ((5, 0), (5 | (1 << 40), 0), (5, 1 << 40), (5, 1)):
        wt = _word(word, cuda)
        gy = _Buf(n, BF16, cuda)
        nat.dropout_bwd(g.data_ptr(), gy.ptr(), n, p, seed, 0 if wt is None else wt.data_ptr(), sp)
        torch.cuda.synchronize()
        assert gy.tail_ok()
        masks.append(gy.t != 0)
        assert torch.equal(masks[-1], po.keep_mask_t((n,), seed, p, cuda, word))
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[0], masks[3])
    assert torch.equal(masks[1], masks[2])  # seed ^ word is all the kernel sees


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gelu_dropout_special_values(cuda, p):
    """+-0, +-2^-126, +-0.5, +-3, +-10, +-40, +-3e38 through both GELU kernels: finite results,
    gelu'(-40) = gelu'(-3e38) = 0 exactly (not NaN), the mask from the replica (read-back is
    impossible here: gelu(+-0) = 0), the value bounds plus 2^-126 for results below the smallest
    normal fp32 (the hardware may flush them)."""
    nat, sp = _nat()
    mags = [0.0, 2.0 ** -126, 0.5, 3.0, 10.0, 40.0, 3e38]
    a = torch.tensor([s * m for m in mags for s in (1.0, -1.0)] + [1.0, -1.0], device=cuda).to(BF16)
    n = a.numel()
    assert n == 16 and torch.isfinite(a).all()
    g = torch.ones(n, device=cuda, dtype=BF16)
    worst, bad = _Worst(), []
    for seed, word in SEEDS:
        wt = _word(word, cuda)
        wp = 0 if wt is None else wt.data_ptr()
        mask = po.keep_mask_t((n,), seed, p, cuda, word)
        scale = po.drop_scale(p)
        h, ga = _Buf(n, BF16, cuda), _Buf(n, BF16, cuda)
        nat.gelu_dropout_fwd(a.data_ptr(), h.ptr(), n, p, seed, wp, sp)
        nat.gelu_dropout_bwd(g.data_ptr(), a.data_ptr(), ga.ptr(), n, p, seed, wp, sp)
        torch.cuda.synchronize()
        assert h.tail_ok() and ga.tail_ok()
        tag = f"seed={seed:#x} word={word:#x} p={p}"
        assert torch.isfinite(h.t).all() and torch.isfinite(ga.t).all(), (tag, h.t, ga.t)
        assert (h.t[~mask] == 0).all() and (ga.t[~mask] == 0).all(), tag
        for i in (11, 13):  # a = -40, -3e38
            assert a[i].item() < -39 and ga.t[i].item() == 0.0, (tag, i, ga.t[i])
        for kind, got, kw in (("gelu", h.t, dict(a=a)), ("gelu_bwd", ga.t, dict(g=g, a=a))):
            ref, bound = _drop_expect(kind, mask, scale, **kw)
            _within(worst, bad, kind, tag, got, ref, bound + 2.0 ** -126 * mask.double())
    worst.report(f"gelu specials p={p}")
    assert not bad, "\n".join(bad)


def _run_2d(worst, bad, rows, cols, seed, word, p, gen, device):
    """Both *_bwd_colsum kernels against the plain backward kernels and the fp64 column sum."""
    nat, sp = _nat()
    n = rows * cols
    wt = _word(word, device)
    wp = 0 if wt is None else wt.data_ptr()
    g32 = _nonzero((rows, cols), gen, device, F32)
    g16 = _nonzero((rows, cols), gen, device, BF16)
    a = _gelu_input((rows, cols), gen, device)
    gb0 = torch.randn(2, cols, generator=gen, device=device)
    gb0 = gb0 + torch.where(gb0 >= 0, 0.5, -0.5)
    mask = po.keep_mask_t((rows, cols), seed, p, device, word)
    tag = f"rows={rows} cols={cols} seed={seed:#x} word={word:#x} p={p}"
    gy, ga = _Buf((rows, cols), BF16, device), _Buf((rows, cols), BF16, device)
    nat.dropout_bwd(g32.data_ptr(), gy.ptr(), n, p, seed, wp, sp)
    nat.gelu_dropout_bwd(g16.data_ptr(), a.data_ptr(), ga.ptr(), n, p, seed, wp, sp)
    gy2, ga2 = _Buf((rows, cols), BF16, device), _Buf((rows, cols), BF16, device)
    gb, gc = _Buf(cols, F32, device, gb0[0]), _Buf(cols, F32, device, gb0[1])
    nat.dropout_bwd_colsum(g32.data_ptr(), gy2.ptr(), gb.ptr(), rows, cols, p, seed, wp, sp)
    nat.gelu_dropout_bwd_colsum(g16.data_ptr(), a.data_ptr(), ga2.ptr(), gc.ptr(), rows, cols, p, seed, wp, sp)
    torch.cuda.synchronize()
    for name, buf in (("gy", gy), ("ga", ga), ("gy2", gy2), ("ga2", ga2), ("gb", gb), ("gc", gc)):
        assert buf.tail_ok(), f"{name} {tag}: canary overwritten"
        assert buf.written(), f"{name} {tag}: elements never written"
    _mask_equal(bad, f"dropout_bwd_colsum {tag}", gy2.t != 0, mask)
    _mask_equal(bad, f"gelu_dropout_bwd_colsum {tag}", ga2.t != 0, mask)
    for name, plain, fused, dst, dst0 in (("dropout", gy, gy2, gb, gb0[0]), ("gelu", ga, ga2, gc, gb0[1])):
        if not torch.equal(plain.bits(), fused.bits()):
            bad.append(f"{name}_bwd_colsum {tag}: stored tensor is not the plain backward's")
        s, mag = po.colsum_oracle(fused.t)
        _within(worst, bad, f"{name} colsum", tag, po.f64(dst.t) - po.f64(dst0), s,
                po.sum_bound(rows, mag + po.f64(dst0).abs()))


@pytest.mark.parametrize("cols", COLS)
def test_dropout_colsum_2d(cuda, cols):
    """dropout_bwd_colsum / gelu_dropout_bwd_colsum store bitwise what the plain backward stores
    (so the replica's mask), and add the fp64 column sum of the stored values to a pre-filled
    bias gradient; partial last column block (cols / 8 % 32 != 0), row counts around the 8 row
    lanes and the 4-row unroll, several row chunks (65 rows; 8200 rows at 8 columns, where the
    rows per block grow past 32)."""
    gen = torch.Generator(device=cuda).manual_seed(cols)
    worst, bad = _Worst(), []
    k = 0
    for rows in ROWS2D + ((8200,) if cols == 8 else ()):
        for p in PS:
            seed, word = SEEDS[k % 3]
            k += 1
            _run_2d(worst, bad, rows, cols, seed, word, p, gen, cuda)
    worst.report(f"dropout 2d cols={cols}")
    assert not bad, "\n".join(bad)


def test_dropout_wrappers_draw_the_seed_from_torch(cuda):
    """After torch.manual_seed(s) the wrappers draw the seed a test can re-draw with the same
    randint call; forward and backward masks are the replica's."""
    from faster_distributed_training_amd.ops import attention_native as AN
    from faster_distributed_training_amd.ops.dropout import dropout_add, gelu_dropout
    assert AN.DEVICE_SEED is None
    rows, cols, p = 33, 264, 0.1
    gen = torch.Generator(device=cuda).manual_seed(5)
    y = _nonzero((rows, cols), gen, cuda, BF16).requires_grad_()
    x = torch.randn(rows, cols, generator=gen, device=cuda)
    a = _gelu_input((rows, cols), gen, cuda).requires_grad_()
    g = _nonzero((rows, cols), gen, cuda, F32)
    for s, op in ((11, "add"), (12, "gelu")):
        torch.manual_seed(s)
        out = dropout_add(y, x, p) if op == "add" else gelu_dropout(a, p)
        torch.manual_seed(s)
        seed = int(torch.randint(0, 2**62, (1,)).item())
        assert seed >= 2 ** 32  # (these two draws do exercise the high bits)
        mask = po.keep_mask_t((rows, cols), seed, p, cuda)
        assert torch.equal((out.detach() != x) if op == "add" else (out.detach() != 0), mask), op
        out.backward(g.to(out.dtype))
        assert torch.equal((y.grad if op == "add" else a.grad) != 0, mask), op


# ================================================================= embedding
EMB_BL = ((1, 1), (1, 3), (1, 4), (1, 5), (3, 21), (1, 64), (5, 13), (3, 43))  # rows 1 .. 129


@pytest.mark.parametrize("d", [256, 512, 768, 3072])
def test_embedding_rows_ids_and_tables(cuda, d):
    """Forward per element and the three table gradients per element against the fp64 sum, at
    row counts around the wave-per-row grid and the 64-row backward blocks; random and all-equal
    token ids, arange and repeated position ids; gradient rows that are zero, -0.0, or nonzero in
    their last element only.  d = 3072 with 3 segment rows takes the global-atomics segment
    path (3 * 3072 floats exceed the LDS accumulator)."""
    from faster_distributed_training_amd.ops.embedding import _EmbeddingNative
    nat, sp = _nat()
    vt, vp, vs = 37, 80, 3
    scale = torch.tensor(math.sqrt(d)).float().item()  # as the kernel receives it: a float
    gen = torch.Generator().manual_seed(d)
    tok, pos, seg = (torch.randn(v, d, generator=gen).to(cuda) for v in (vt, vp, vs))
    worst, bad = _Worst(), []
    for B, L in EMB_BL:
        rows = B * L
        for id_kind in ("random", "equal"):
            for pos_kind in ("arange", "repeats"):
                tag = f"d={d} B={B} L={L} ids={id_kind} pos={pos_kind}"
                ids = (torch.randint(0, vt, (B, L), generator=gen) if id_kind == "random"
                       else torch.full((B, L), 5)).to(cuda)
                types = (torch.arange(rows).view(B, L) % vs).to(cuda)
                pos_ids = (torch.arange(vp) if pos_kind == "arange" else torch.arange(vp) // 2).to(cuda)
                assert int(ids.max()) < vt and int(pos_ids[:L].max()) < vp and int(types.max()) < vs
                g = torch.randn(B, L, d, generator=gen)
                gf = g.view(rows, d)
                gf[0] = 0.0
                gf[0, d - 1] = 1.0          # the only nonzero is the last element
                if rows > 1:
                    gf[1] = 0.0             # a whole zero row
                if rows > 2:
                    gf[2] = -0.0            # and one of negative zeros
                g = g.to(cuda)
                o = po.emb_oracle(ids, types, pos_ids, tok, pos, seg, scale, g)
                ids32, ty32, pos32 = (t.to(torch.int32).contiguous() for t in (ids, types, pos_ids[:L]))
                out = _Buf((B, L, d), F32, cuda)
                nat.embedding_fwd(ids32.data_ptr(), ty32.data_ptr(), pos32.data_ptr(), tok.data_ptr(), pos.data_ptr(),
                                  seg.data_ptr(), out.ptr(), B, L, d, scale, vt, vp, vs, sp)
                pre = [torch.randn(v, d, generator=gen).to(cuda) for v in (vt, vp, vs)]
                dst = [_Buf((v, d), F32, cuda, q) for v, q in zip((vt, vp, vs), pre)]
                nat.embedding_bwd(g.data_ptr(), ids32.data_ptr(), ty32.data_ptr(), pos32.data_ptr(), dst[0].ptr(),
                                  dst[1].ptr(), dst[2].ptr(), B, L, d, scale, vt, vp, vs, sp)
                torch.cuda.synchronize()
                assert out.tail_ok() and out.written(), tag
                assert all(b.tail_ok() for b in dst), tag
                _within(worst, bad, "forward", tag, out.t, o.out, 3 * po.EPS24 * o.mag)
                # the autograd wrapper: the same forward, gradients returned in fresh tensors
                ws = [t.detach().clone().requires_grad_() for t in (tok, pos, seg)]
                wout = _EmbeddingNative.apply(ids, types, pos_ids, *ws, scale)
                wout.backward(g)
                if not torch.equal(wout.detach(), out.t):
                    bad.append(f"{tag}: _EmbeddingNative's forward is not the direct call's")
                for name, part, w, q, buf in zip(("tok", "pos", "seg"), (o.tok, o.pos, o.seg), ws, pre, dst):
                    k = (part.count + 2)[:, None]
                    _within(worst, bad, f"d{name} returned", tag, w.grad, part.grad, k * po.EPS24 * part.mag)
                    q64 = po.f64(q)
                    _within(worst, bad, f"d{name} accumulated", tag, po.f64(buf.t) - q64, part.grad,
                            k * po.EPS24 * (part.mag + q64.abs()))
                    idle = part.count == 0  # rows nothing maps to keep their content bitwise
                    if not torch.equal(buf.t[idle], q[idle]):
                        bad.append(f"{tag}: d{name} rows without contributions changed")
    worst.report(f"embedding d={d}")
    assert not bad, "\n".join(bad)


# ================================================================= mlp.hip
MLP_ROWS = (1, 31, 32, 33, 65)


def _mlp_run(fn, ts, g, dt):
    ps = [None if t is None else t.detach().clone().requires_grad_() for t in ts]
    if dt == F32:
        out = fn(*ps)
    else:
        with torch.autocast("cuda", dtype=dt):
            out = fn(*ps)
    out.backward(g.to(out.dtype))
    return [out.detach()] + [None if p is None else p.grad for p in ps]


def _dyadic(shape, gen, step, lim):
    """Random multiples of ``step`` in [-lim, lim]."""
    k = int(round(lim / step))
    return torch.randint(-k, k + 1, shape, generator=gen).float() * step


def _mlp_inputs(rows, hidden, din, ncls, exact, gen, device, dt):
    """``exact``: X and W1 are multiples of 1/2 in [-1, 1] and b1 odd multiples of 1/8 in
    [-2, 2], so X W1^T (multiples of 1/4, at most 16 in size) and pre (multiples of 1/8 below
    18.125) are exact in bf16, fp16 and fp32: the ReLU mask of the kernel and of the fp64 oracle
    are the same set, and pre == 0 exactly is common when there is no b1.  Otherwise randn."""
    if exact:
        X, W1 = _dyadic((rows, din), gen, 0.5, 1.0), _dyadic((hidden, din), gen, 0.5, 1.0)
        b1 = _dyadic((hidden,), gen, 0.25, 1.75) + 0.125
    else:
        X, W1 = torch.randn(rows, din, generator=gen), torch.randn(hidden, din, generator=gen) * 0.3
        b1 = torch.randn(hidden, generator=gen)
    W2 = torch.randn(ncls, hidden, generator=gen) * 0.3
    b2 = torch.randn(ncls, generator=gen)
    g = torch.randn(rows, ncls, generator=gen)
    dead = [1, hidden - 2]
    W1[dead], b1[dead] = 0.0, 0.0
    return [t.to(device) for t in (X, W1, b1, W2, b2)], g.to(device).to(dt), dead


@pytest.mark.parametrize("exact", [True, False], ids=["exact-pre", "randn"])
@pytest.mark.parametrize("hidden", [8, 1000])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_fused_mlp_rows_and_dtypes(cuda, dt, hidden, exact):
    """fused_mlp (bias_relu_fwd, relu_bwd_colsum) per row against the fp64 oracle on the
    dtype-rounded inputs, the arm being F.linear / relu / F.linear in the same dtype; with and
    without biases, bias_grad_mean on and off; hidden columns 1 and hidden - 2 have zero weights
    and bias, so pre == 0 there and nothing may flow back through them.

    Gradients are judged on inputs whose pre is exact in every dtype (_mlp_inputs): with randn
    inputs a pre within a rounding of zero has one ReLU mask in fp64 and another in bf16, for the
    arm as for the kernel, and its whole gradient term is then "wrong" by definition, not by
    rounding.  The randn inputs judge the forward, which has no such jump."""
    from faster_distributed_training_amd.ops.mlp import fused_mlp
    din, ncls = 16, 4
    gen = torch.Generator().manual_seed(hidden + exact)
    worst, bad = _Worst(), []
    for rows in MLP_ROWS:
        (X, W1, b1, W2, b2), g, dead = _mlp_inputs(rows, hidden, din, ncls, exact, gen, cuda, dt)
        for has_b1, has_b2, mean in ((True, True, False), (True, True, True), (False, True, False),
                                     (True, False, True), (False, False, False)):
            tag = f"rows={rows} hidden={hidden} {dt} b1={has_b1} b2={has_b2} mean={mean}".replace("torch.", "")
            ts = [X, W1, b1 if has_b1 else None, W2, b2 if has_b2 else None]
            got = _mlp_run(lambda *a: fused_mlp(*a, mean), ts, g, dt)
            arm = _mlp_run(lambda x, w1, c1, w2, c2: F.linear(torch.relu(F.linear(x, w1, c1)), w2, c2), ts, g, dt)
            k = 1.0 / rows if mean else 1.0
            # the biases enter their GEMMs rounded to dt
            o = po.mlp_oracle(X.to(dt), W1.to(dt), b1.to(dt) if has_b1 else None, W2.to(dt),
                              b2.to(dt) if has_b2 else None, g, mean)
            if exact:
                lo = o.pre.abs()[:, [j for j in range(hidden) if j not in dead]]
                assert (o.pre[:, dead] == 0).all() and ((lo == 0) | (lo >= 0.125)).all()
            refs = [o.out, o.gX, o.gW1, o.gb1, o.gW2, o.gb2]
            for name, gt, am, rf, floor in zip(("out", "gX", "gW1", "gb1", "gW2", "gb2"), got, arm, refs,
                                               (1e-5, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4)):
                if rf is None:
                    assert gt is None, (tag, name)
                    continue
                if not exact and name != "out":
                    continue
                if name in ("gb1", "gb2"):
                    gt, am, rf = gt.reshape(1, -1), am.reshape(1, -1) * k, rf.reshape(1, -1)
                _budget(worst, bad, name, tag, gt, am, rf, floor if dt == F32 else 0.0)
            if not bool((got[2][dead] == 0).all()):
                bad.append(f"{tag}: gW1 of a hidden unit with pre == 0 is not zero")
            if has_b1 and not bool((got[3].reshape(-1)[dead] == 0).all()):
                bad.append(f"{tag}: gb1 of a hidden unit with pre == 0 is not zero")
    worst.report(f"fused_mlp {dt} hidden={hidden} exact={exact}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_bias_relu_fwd_with_bias(cuda, dt):
    """bias_relu_fwd called directly with a bias (fused_mlp passes none: its biases ride in the
    GEMMs): pre becomes pre + b[column] rounded once, in place, and act is relu of exactly that."""
    nat, sp = _nat()
    gen = torch.Generator(device=cuda).manual_seed(3)
    worst, bad = _Worst(), []
    for rows in MLP_ROWS:
        for cols in (8, 1000):
            pre0 = torch.randn(rows, cols, generator=gen, device=cuda).to(dt)
            b = torch.randn(cols, generator=gen, device=cuda)
            b[1], pre0[:, 1] = 0.0, 0.0
            pre, act = _Buf((rows, cols), dt, cuda, pre0), _Buf((rows, cols), dt, cuda)
            nat.bias_relu_fwd(pre.ptr(), b.data_ptr(), act.ptr(), rows, cols, DT[dt], sp)
            torch.cuda.synchronize()
            tag = f"rows={rows} cols={cols} {dt}"
            assert pre.tail_ok() and act.tail_ok() and act.written(), tag
            ref = po.f64(pre0) + po.f64(b)
            _budget(worst, bad, "pre", tag, pre.t, ref.to(dt), ref, 1e-6 if dt == F32 else 0.0)
            assert torch.equal(act.t, torch.relu(pre.t)), tag
            assert (act.t[:, 1] == 0).all(), tag
    worst.report(f"bias_relu_fwd {dt}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cols", COLS)
def test_bias_grad_into_strided(cuda, cols):
    """colsum_bf16 through bias_grad_into: a contiguous gradient and the middle third of a packed
    [rows, 3 cols] one (ld > cols; the other two thirds hold NaN), added to a pre-filled
    destination; row counts around the 8 row lanes and the 64-row blocks."""
    from faster_distributed_training_amd.ops.linear import bias_grad_into
    gen = torch.Generator(device=cuda).manual_seed(cols)
    worst, bad = _Worst(), []
    for rows in ROWS2D + (63, 64) + ((8200,) if cols == 8 else ()):
        gy = torch.randn(rows, cols, generator=gen, device=cuda).to(BF16)
        wide = torch.full((rows, 3 * cols), float("nan"), device=cuda, dtype=BF16)
        wide[:, cols:2 * cols] = gy
        s, mag = po.colsum_oracle(gy)
        for name, src in (("contiguous", gy), ("packed slice", wide[:, cols:2 * cols])):
            assert src.dtype == BF16 and src.stride(1) == 1 and src.stride(0) % 8 == 0 and src.data_ptr() % 16 == 0
            dst0 = torch.randn(cols, generator=gen, device=cuda)
            dst = _Buf(cols, F32, cuda, dst0)
            bias_grad_into(src, dst.t)
            torch.cuda.synchronize()
            tag = f"rows={rows} cols={cols} {name}"
            assert dst.tail_ok(), tag
            _within(worst, bad, "colsum_bf16", tag, po.f64(dst.t) - po.f64(dst0), s,
                    po.sum_bound(rows, mag + po.f64(dst0).abs()))
    worst.report(f"colsum_bf16 cols={cols}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", [4, 252, 256, 260, 4 * 64 * 512])
def test_slab_sum_acc_strided(cuda, n):
    """slab_sum_acc called directly with ld = n and ld = 2 n (the LayerNorm partials' layout; the
    columns past n hold NaN), into a pre-filled destination.  n = 131072 gives 512 column blocks:
    the slab axis is not split and the result is stored without atomics (513 slabs are left out
    there: 0.5 GB that reaches no further path, every s keeps one block per column group)."""
    nat, sp = _nat()
    gen = torch.Generator(device=cuda).manual_seed(n)
    worst, bad = _Worst(), []
    for s in (1, 3, 4, 5, 16, 17) + ((513,) if n < 1000 else ()):
        for ld in (n, 2 * n):
            src = torch.full((s, ld), float("nan"), device=cuda)
            src[:, :n] = torch.randn(s, n, generator=gen, device=cuda)
            dst0 = torch.randn(n, generator=gen, device=cuda)
            dst = _Buf(n, F32, cuda, dst0)
            nat.slab_sum_acc(src.data_ptr(), dst.ptr(), s, ld, n, sp)
            torch.cuda.synchronize()
            tag = f"s={s} n={n} ld={ld}"
            assert dst.tail_ok(), tag
            ref, mag = po.slabsum_oracle(src, n)
            _within(worst, bad, "slab_sum_acc", tag, po.f64(dst.t) - po.f64(dst0), ref,
                    po.sum_bound(s, mag + po.f64(dst0).abs()))
    worst.report(f"slab_sum_acc n={n}")
    assert not bad, "\n".join(bad)

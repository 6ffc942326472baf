"""The fused data + weight gradient of the expanding 1x1 convolutions (ops.conv_igemm.conv_bwd_pair,
csrc/kernels/conv_bwd_pair.hip) against the fp32 PyTorch reference on the bf16-rounded operands
and against the two-launch path it replaces (conv_dgrad + conv_wgrad), with the budgets of
tests/test_conv_kernels.py: dX 1e-2, statistics rows 1e-2, dW 5e-3 (relative L2).  CPU tests: the
support predicate and the fall-back to the pair."""
import functools

import pytest
import torch

from faster_distributed_training_amd.ops import conv_igemm as ci

BF = torch.bfloat16
BF16_SENTINEL = 0x7FA5  # a NaN bit pattern no kernel result has
F32_SENTINEL = -7.25e30
GUARD = 4096

# (N, H, Cin, Cout), wgs: the grid is fixed so that each chunk distribution is hit
CASES = [
    ((3, 5, 64, 256), None),   # M = 75: one partial chunk
    ((5, 11, 64, 256), 2),     # M = 605: chunks 3 + 2, the last one partial (uneven split)
    ((2, 8, 64, 256), 4),      # M = 128: one chunk, three idle workgroups
]
VARIANTS = ["actbwd_gs", "actbwd", "store"]


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def nchw(x):
    return x.permute(0, 3, 1, 2).float()


def nhwc(x):
    return x.permute(0, 2, 3, 1)


class Guarded:
    """A tensor of ``shape`` in the middle of a sentinel-filled buffer (bf16 or fp32)."""

    def __init__(self, shape, dev, dtype=BF, init=None):
        n = 1
        for d in shape:
            n *= d
        self.n = n
        if dtype == BF:
            self.raw = torch.full((GUARD + n + GUARD,), BF16_SENTINEL, dtype=torch.int16, device=dev)
            self.t = self.raw[GUARD:GUARD + n].view(BF).view(*shape)
            self.sent = BF16_SENTINEL
        else:
            self.raw = torch.full((GUARD + n + GUARD,), F32_SENTINEL, dtype=torch.float32, device=dev)
            self.t = self.raw[GUARD:GUARD + n].view(*shape)
            self.sent = F32_SENTINEL
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        return bool((self.raw[:GUARD] == self.sent).all()) and bool((self.raw[GUARD + self.n:] == self.sent).all())


@functools.lru_cache(maxsize=None)
def _case(shape, variant, dev, alpha_scale=0.1):
    """Inputs and the fp32 reference of one case (computed once, shared, never modified)."""
    N, H, Cin, Cout = shape
    torch.manual_seed(11)
    shp = ci.ConvShape(Cin, Cout, 1, 1, 0)
    w = torch.randn(Cout, Cin, 1, 1, device=dev) / Cin ** 0.5
    _, wd = ci.alloc_packed(shp, dev, fwd=False)
    ci.pack_weights([(w, None, wd, shp)])
    mk = lambda *s: torch.randn(*s, device=dev).to(BF)
    g, y, x = mk(N, H, H, Cout), mk(N, H, H, Cout), mk(N, H, H, Cin)
    al = torch.randn(Cout, device=dev) * alpha_scale
    be = torch.randn(Cout, device=dev) * 0.1
    gs = torch.rand(Cout, device=dev) + 0.5 if variant == "actbwd_gs" else None
    gt = g.float() * (gs if gs is not None else 1.0) + al + be * y.float()
    gt = gt.to(BF).float()
    dx = nhwc(torch.nn.grad.conv2d_input((N, Cin, H, H), w.to(BF).float(), nchw(gt)))
    c = dict(shp=shp, wd=wd, g=g, y=y, x=x, al=al, be=be, gs=gs, M=N * H * H)
    if variant == "store":
        a = x.float()
        c.update(epi=ci.EPI_STORE, act=0, s=None, t=None, dx=dx, q=None)
    else:
        s = torch.randn(Cin, device=dev)  # BN scales of both signs
        s = torch.where(s.abs() < 0.1, torch.full_like(s, 0.5), s)
        t = torch.randn(Cin, device=dev) * 0.3
        z = x.float() * s + t
        a = torch.relu(z).to(BF).float()
        gp = dx * (z > 0).float()
        q = torch.stack([(gp * x.float()).reshape(-1, Cin).sum(0), gp.reshape(-1, Cin).sum(0)])
        c.update(epi=ci.EPI_ACTBWD, act=1, s=s, t=t, dx=gp * s, q=q)
    c["dw"] = torch.nn.grad.conv2d_weight(nchw(a), (Cout, Cin, 1, 1), nchw(gt))
    return c


def _start(c, dev, seed):
    """dX in guards, dW in guards and the slots pre-loaded with random values: the launch must
    add to them, not overwrite."""
    N, H = c["g"].shape[:2]
    Cin, Cout = c["shp"].cin, c["shp"].cout
    gen = torch.Generator(device="cpu").manual_seed(seed)
    dw0 = torch.randn(Cout, Cin, 1, 1, generator=gen).to(dev)
    gx = Guarded((N, H, H, Cin), dev)
    gw = Guarded((Cout, Cin, 1, 1), dev, torch.float32, dw0)
    part = p0 = None
    if c["epi"] == ci.EPI_ACTBWD:
        part = ci.stat_slots(2, Cin, dev, c["M"])
        part.copy_(torch.randn(part.shape, generator=gen).to(dev))
        p0 = part.clone()
    return gx, gw, dw0, part, p0


def _fused(c, gx, gw, part, wgs):
    return ci.conv_bwd_pair(c["g"], c["y"], c["al"], c["be"], c["wd"], c["x"], c["shp"], gw.t, epi=c["epi"],
                            xs=c["s"], xt=c["t"], es=c["s"], et=c["t"], act=c["act"], part=part, gs=c["gs"],
                            accumulate=True, wgs=wgs, out=gx.t)


def _pair(c, gx, gw, part):
    ci.conv_dgrad(c["g"], c["y"], c["al"], c["be"], c["wd"], c["shp"], tuple(c["x"].shape), epi=c["epi"],
                  out=gx.t, ex=c["x"] if part is not None else None, es=c["s"], et=c["t"], act=c["act"], part=part,
                  gs=c["gs"])
    ci.conv_wgrad(c["g"], c["y"], c["al"], c["be"], c["x"], c["shp"], gw.t, c["s"], c["t"], c["act"],
                  accumulate=True, gs=c["gs"])


def _check(c, gx, gw, dw0, part, p0, what, ref=None):
    """dX / statistics rows / dW of one launch against ``ref`` (default: the fp32 reference)."""
    rdx, rq, rdw = ref if ref is not None else (c["dx"], c["q"], c["dw"])
    e = rel(gx.t, rdx)
    print(what, "dX", e)
    assert e < 1e-2, (what, e)
    if part is not None:
        ps = (part - p0).sum(0)
        for i in range(2):
            e = rel(ps[i], rq[i])
            print(what, "slot row", i, e)
            assert e < 1e-2, (what, i, e)
    e = rel(gw.t - dw0, rdw)
    print(what, "dW", e)
    assert e < 5e-3, (what, e)
    assert gx.intact() and gw.intact(), what


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])))
@pytest.mark.parametrize("variant", VARIANTS)
def test_pair_matches_reference_and_two_launch_path(cuda, case, variant):
    shape, wgs = case
    c = _case(shape, variant, str(cuda))
    ci.LAUNCH_LOG = []
    try:
        gx, gw, dw0, part, p0 = _start(c, cuda, 5)
        _fused(c, gx, gw, part, wgs)
        log = list(ci.LAUNCH_LOG)
    finally:
        ci.LAUNCH_LOG = None
    assert [e[0] for e in log] == ["bwdpair"] and log[0][5] == 11
    chunks = -(-c["M"] // ci.BWD_PAIR_PX)
    assert log[0][4] == -(-chunks // -(-chunks // (wgs or ci.BWD_PAIR_WGS)))  # workgroups with work
    _check(c, gx, gw, dw0, part, p0, "fused vs reference")
    bx, bw, bw0, bpart, bp0 = _start(c, cuda, 5)
    _pair(c, bx, bw, bpart)
    _check(c, bx, bw, bw0, bpart, bp0, "pair vs reference")
    two = (bx.t.float(), (bpart - bp0).sum(0) if bpart is not None else None, bw.t - bw0)
    _check(c, gx, gw, dw0, part, p0, "fused vs pair", ref=two)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["actbwd", "store"])
def test_pair_masks_rows_past_m(cuda, variant):
    """M = 75 of a 128-pixel chunk with a LARGE alpha: the 53 padded rows fold to alpha (and, with
    the input transform, to relu(xt)), so a kernel that does not mask them misses dW and the
    statistics by far more than the budget."""
    c = _case((3, 5, 64, 256), variant, str(cuda), alpha_scale=4.0)
    gx, gw, dw0, part, p0 = _start(c, cuda, 6)
    _fused(c, gx, gw, part, None)
    _check(c, gx, gw, dw0, part, p0, "masking")


def _det_runs(c, dev, wgs, repeats):
    outs = []
    for _ in range(repeats):
        gx, gw, dw0, part, p0 = _start(c, dev, 9)
        _fused(c, gx, gw, part, wgs)
        torch.cuda.synchronize()
        outs.append((gx.t.view(torch.int16).clone(), None if part is None else part.view(torch.int32).clone(),
                     gw.t.view(torch.int32).clone()))
        assert gx.intact() and gw.intact()
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]), "dX"
        assert o[1] is None or torch.equal(o[1], outs[0][1]), "slots"
        assert torch.equal(o[2], outs[0][2]), "dW"
    return gx, gw, dw0, part, p0


@pytest.mark.gpu
def test_pair_deterministic_mode_bitwise(cuda):
    """Deterministic mode (slab + wgrad_reduce, one writer per slot): launches are bitwise equal
    -- at the small shapes, and at 64 images of 32x32 (512 chunks, every CU busy; three repeats)."""
    from faster_distributed_training_amd.ops import _native
    _native.set_deterministic(True)
    try:
        for shape, wgs in CASES:
            c = _case(shape, "actbwd_gs", str(cuda))
            st = _det_runs(c, cuda, wgs, 2)
            _check(c, *st, "deterministic small")
        big = _case((64, 32, 64, 256), "actbwd", str(cuda))
        st = _det_runs(big, cuda, None, 3)
        _check(big, *st, "deterministic 64x32x32")
        st = _det_runs(_case((64, 32, 64, 256), "store", str(cuda)), cuda, None, 3)
    finally:
        _native.set_deterministic(False)


@pytest.mark.gpu
def test_engine_step_with_fused_pair_matches_the_pair(cuda, monkeypatch):
    """One ResNet-50 training step at batch 8 with the "bwdpair" entry forced for the 32x32
    64 -> 256 layers against the same step with FDT_BWD_PAIR=0, with the budgets
    tests/test_resnet_engine.py holds the engine to: logits within max(2 e_ref, 3e-2), every
    gradient within max(2 e_b, 5e-3) (fc.bias 1.5e-2), e_ref / e_b = what the fp32 reference
    model loses on the logits / on that parameter under bf16 autocast.  The launch log shows the
    fused path.  (Printed beside each worst case: the distance of a second two-launch step.)"""
    import torch.nn.functional as F
    from faster_distributed_training_amd.models import resnet as R
    shp = ci.ConvShape(64, 256, 1, 1, 0)
    ci.tuned("bwdpair", 8, 32, shp)  # (loads the table)
    key = ci.tune_key(8, 32, shp)
    monkeypatch.setitem(ci._TUNED, key, dict(ci._TUNED.get(key, {}), bwdpair={"tile": [128, 64, 64], "wgs": 256}))
    torch.backends.cudnn.allow_tf32 = False
    torch.manual_seed(0)
    # fp32 reference, the same under bf16 autocast, engine with the pair (twice), engine fused
    models = [R.resnet50(10).to(cuda) for _ in range(5)]
    for m in models[1:]:
        m.load_state_dict(models[0].state_dict())
    torch.manual_seed(1)
    x = torch.randn(8, 3, 32, 32, device=cuda)
    y = torch.randint(0, 10, (8,), device=cuda)
    outs, logs = [], []
    for i, m in enumerate(models):
        m.fast_path = i >= 2
        monkeypatch.setattr(ci, "BWD_PAIR", i == 4)
        ci.LAUNCH_LOG = []
        try:
            if i == 1:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    out = m(x)
            else:
                out = m(x)
            F.cross_entropy(out.float(), y).backward()
            logs.append(list(ci.LAUNCH_LOG))
        finally:
            ci.LAUNCH_LOG = None
        outs.append(out)
    assert not any(e[0] == "bwdpair" for e in logs[2] + logs[3])
    # three conv3 layers (ACTBWD) and the expanding shortcut (STORE) of the first stage
    assert sum(e[0] == "bwdpair" for e in logs[4]) == 4, [e for e in logs[4] if e[0] == "bwdpair"]
    assert len(logs[2]) - len(logs[4]) == 4  # each fused launch replaces a dgrad and a wgrad
    e_ref, e = rel(outs[1], outs[0]), rel(outs[4], outs[2])
    assert e < max(2.0 * e_ref, 3e-2), (e, e_ref)
    worst = []
    named = [list(m.named_parameters()) for m in models]
    for (n, pr), (_, pb), (_, p0), (_, p0b), (_, p1) in zip(*named):
        assert p1.grad is not None, n
        e_b, e, noise = rel(pb.grad, pr.grad), rel(p1.grad, p0.grad), rel(p0b.grad, p0.grad)
        worst.append((e / max(e_b, 1e-6), n, e, e_b, noise))
    worst.sort(reverse=True)
    print("worst (fused vs pair) / autocast error ratios: (ratio, name, fused-pair, autocast-fp32, pair-pair)")
    for w in worst[:6]:
        print("  ", w)
    for _, n, e, e_b, _ in worst:
        assert e <= max(2.0 * e_b, 1.5e-2 if n == "fc.bias" else 5e-3), (n, e, e_b)


# ---------------------------------------------------------------------------------- CPU
def test_bwd_pair_predicate_support_set():
    ok = ci.bwd_pair_ok
    s = ci.ConvShape(64, 256, 1, 1, 0)
    assert ok(s, ci.EPI_ACTBWD, 1)
    assert ok(s, ci.EPI_STORE, 0)
    assert ok(s, ci.EPI_STORE, 0, True, False)
    assert not ok(s, ci.EPI_ACTBWD, 2)                     # CELU
    assert not ok(s, ci.EPI_ACTBWD, 0)                     # ACTBWD without an activation
    assert not ok(s, ci.EPI_ACTBWD, 1, True, False)        # ... or without the input transform
    assert not ok(s, ci.EPI_STORE, 0, True, True)          # STORE with an input transform
    assert not ok(s, ci.EPI_STORE, 0, False)               # no fold
    assert not ok(s, ci.EPI_ADD, 0) and not ok(s, ci.EPI_JOINBWD, 1)
    assert not ok(ci.ConvShape(128, 512, 1, 1, 0), ci.EPI_ACTBWD, 1)   # not instantiated
    assert not ok(ci.ConvShape(256, 1024, 1, 1, 0), ci.EPI_ACTBWD, 1)  # out of scope
    assert not ok(ci.ConvShape(256, 64, 1, 1, 0), ci.EPI_ACTBWD, 1)    # reducing
    assert not ok(ci.ConvShape(64, 128, 1, 1, 0), ci.EPI_STORE, 0)     # ratio 2
    assert not ok(ci.ConvShape(64, 256, 3, 1, 1), ci.EPI_ACTBWD, 1)    # 3x3
    assert not ok(ci.ConvShape(64, 256, 1, 2, 0), ci.EPI_STORE, 0)     # strided


def test_bwd_pair_falls_back_to_the_pair(monkeypatch):
    """A table entry alone does not select the fused launch: an unsupported launch, a CELU
    activation or FDT_BWD_PAIR=0 keep the two launches; no entry does too."""
    s = ci.ConvShape(64, 256, 1, 1, 0)
    big = ci.ConvShape(128, 512, 1, 1, 0)
    ent = {"bwdpair": {"tile": [128, 64, 64], "wgs": 256}}
    monkeypatch.setattr(ci, "_TUNED", {ci.tune_key(8, 32, s): ent, ci.tune_key(8, 16, big): ent})
    monkeypatch.setattr(ci, "BWD_PAIR", True)
    assert ci.bwd_pair_entry(8, 32, s, ci.EPI_ACTBWD, 1) == ent["bwdpair"]
    assert ci.bwd_pair_entry(8, 32, s, ci.EPI_STORE, 0, True, False) == ent["bwdpair"]
    assert ci.bwd_pair_entry(8, 16, big, ci.EPI_ACTBWD, 1) is None   # entry, unsupported launch
    assert ci.bwd_pair_entry(8, 32, s, ci.EPI_ACTBWD, 2) is None     # CELU
    assert ci.bwd_pair_entry(16, 32, s, ci.EPI_ACTBWD, 1) is None    # no entry for this batch
    monkeypatch.setattr(ci, "BWD_PAIR", False)
    assert ci.bwd_pair_entry(8, 32, s, ci.EPI_ACTBWD, 1) is None     # FDT_BWD_PAIR=0

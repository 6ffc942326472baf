"""The activation-stationary 1x1 convolution kernel (kg 10, csrc/kernels/conv_x1_impl.h) against the
implicit-GEMM kernel it replaces on some layers: same explicit tile, nsplit 1, once with kg 1 and
once with kg 10 -- outputs and statistics slots bit-identical, nothing written outside the output.
One case per prologue is also held to the fp32 PyTorch reference with the budgets of
tests/test_conv_kernels.py.  CPU tests: the Python support predicate and the table fallback."""
import pytest
import torch
import torch.nn.functional as F

from faster_distributed_training_amd.ops import conv_igemm as ci

BF = torch.bfloat16
BF16_SENTINEL = 0x7FA5  # a NaN bit pattern no kernel result has
GUARD = 4096            # sentinel elements on both sides of an output

# (N, H, K, Nout) of the GEMM out[N*H*H][Nout] = X[N*H*H][K] W[Nout][K]^T
SHAPES = [
    (3, 5, 64, 256),     # M = 75: one partial row block
    (5, 6, 128, 512),    # M = 180: one full and one partial block
    (2, 8, 256, 1024),   # M = 128 exact, 8 column tiles
    (2, 4, 512, 2048),   # K = 512: the BM = 64 instantiation, 16 column tiles
    (3, 5, 128, 256),    # ratio 2
    (4, 4, 64, 128),     # a single column tile
]
REF_SHAPE = (5, 6, 128, 512)  # the case also compared with the fp32 reference


def _tile(K):
    return (64, 128, 32) if K == 512 else (128, 128, 32)


def _xns(nout):
    nbn = nout // 128
    return sorted({x for x in (1, 2, nbn) if nbn % x == 0})


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def make(shape, dev, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(BF)


def nchw(x):
    return x.permute(0, 3, 1, 2).float()


def nhwc(x):
    return x.permute(0, 2, 3, 1)


class Guarded:
    """A bf16 tensor of ``shape`` in the middle of a sentinel-filled buffer."""

    def __init__(self, shape, dev, init=None):
        n = 1
        for d in shape:
            n *= d
        self.raw = torch.full((GUARD + n + GUARD,), BF16_SENTINEL, dtype=torch.int16, device=dev)
        self.n = n
        self.t = self.raw[GUARD:GUARD + n].view(BF).view(*shape)
        if init is not None:
            self.t.copy_(init)

    def bits(self):
        return self.raw[GUARD:GUARD + self.n]

    def intact(self):
        return bool((self.raw[:GUARD] == BF16_SENTINEL).all()) and bool((self.raw[GUARD + self.n:] == BF16_SENTINEL).all())


def _slots(nq, C, dev, M, seed):
    """Statistics slots that already hold something: a launch that re-zeroed a slot (or wrote one
    it does not own) would differ from the kg 1 launch on the same start values."""
    part = ci.stat_slots(nq, C, dev, M)
    g = torch.Generator(device="cpu").manual_seed(seed)
    part.copy_(torch.randn(part.shape, generator=g).to(dev))
    return part


def _bits32(t):
    return t.view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ["plain", "relu", "affine"])
def test_x1_forward_bit_identical(cuda, shape, mode):
    from faster_distributed_training_amd.ops import _native
    N, H, K, Nout = shape
    torch.manual_seed(0)
    shp = ci.ConvShape(K, Nout, 1, 1, 0)
    x = make((N, H, H, K), cuda)
    w = torch.randn(Nout, K, 1, 1, device=cuda) / K ** 0.5
    wf, _ = ci.alloc_packed(shp, cuda, dgrad=False)
    ci.pack_weights([(w, wf, None, shp)])
    if mode == "plain":
        s = t = None
        act = 0
    else:
        s = torch.randn(K, device=cuda)  # negative scales included
        s = torch.where(s.abs() < 0.1, torch.full_like(s, 0.5), s)
        t = torch.randn(K, device=cuda) * 0.3
        act = 1 if mode == "relu" else 0
    tile, M = _tile(K), N * H * H
    for det in (False, True):
        _native.set_deterministic(det)
        try:
            base = Guarded((N, H, H, Nout), cuda)
            p0 = _slots(2, Nout, cuda, M, 7)
            ci.conv_fwd(x, wf, shp, s, t, act, 1.0, tile=tile, nsplit=1, kg=1, part=p0, out=base.t)
            for xn in _xns(Nout):
                new = Guarded((N, H, H, Nout), cuda)
                p1 = _slots(2, Nout, cuda, M, 7)
                ci.conv_fwd(x, wf, shp, s, t, act, 1.0, tile=tile, nsplit=1, kg=10, xn=xn, part=p1, out=new.t)
                assert torch.equal(new.bits(), base.bits()), (det, xn)
                assert torch.equal(_bits32(p1), _bits32(p0)), (det, xn)
                assert new.intact() and base.intact(), (det, xn)
        finally:
            _native.set_deterministic(False)
    if shape == REF_SHAPE:
        # the budget of tests/test_conv_kernels.py::test_conv_fwd (positive scales, as there)
        if mode != "plain":
            s = torch.rand(K, device=cuda) + 0.5
        a = x.float() if mode == "plain" else (x.float() * s + t)
        if mode == "relu":
            a = torch.relu(a)
        a = a.to(BF).float()
        y, part = ci.conv_fwd(x, wf, shp, s, t, act, 1.0, tile=tile, nsplit=1, kg=10, xn=2)
        ref = nhwc(F.conv2d(nchw(a), w.to(BF).float()))
        assert rel(y, ref) < 1e-2, rel(y, ref)
        ps, yf = part.sum(0), ref.reshape(-1, Nout)
        assert rel(ps[0], yf.sum(0)) < 2e-3
        assert rel(ps[1], (yf * yf).sum(0)) < 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("epi", ["store", "add", "join", "join_shortcut"])
@pytest.mark.parametrize("scaled", [False, True])
def test_x1_dgrad_bit_identical(cuda, shape, epi, scaled):
    """The data gradient of the reducing 1x1 convolution Nout -> K (as a GEMM: K deep, Nout wide)
    with the fold prologue (with and without gs) and the store / add / join-backward epilogues."""
    from faster_distributed_training_amd.ops import _native
    N, H, K, Nout = shape
    torch.manual_seed(1)
    shp = ci.ConvShape(Nout, K, 1, 1, 0)  # forward conv Nout -> K; its dgrad is the expanding GEMM
    w = torch.randn(K, Nout, 1, 1, device=cuda) / Nout ** 0.5
    _, wd = ci.alloc_packed(shp, cuda, fwd=False)
    ci.pack_weights([(w, None, wd, shp)])
    g, y = make((N, H, H, K), cuda), make((N, H, H, K), cuda)
    al = torch.randn(K, device=cuda) * 0.1
    be = torch.randn(K, device=cuda) * 0.1
    gs = torch.randn(K, device=cuda) if scaled else None
    xs = (N, H, H, Nout)
    prev = make(xs, cuda)
    kw = {}
    e = {"store": ci.EPI_STORE, "add": ci.EPI_ADD}.get(epi, ci.EPI_JOINBWD)
    if e == ci.EPI_JOINBWD:
        jo = make(xs, cuda)
        bits = (jo.reshape(-1, 8) > 0).to(torch.int32)
        mask = (bits << torch.arange(8, device=cuda, dtype=torch.int32)).sum(1).to(torch.uint8)
        kw = dict(ex=make(xs, cuda), act=1, jmask=mask, jyb=make(xs, cuda) if epi == "join_shortcut" else None)
    tile, M = _tile(K), N * H * H

    def run(kgv, xn):
        out = Guarded(xs, cuda, init=prev)
        part = _slots(3, Nout, cuda, M, 11) if e == ci.EPI_JOINBWD else None
        ci.conv_dgrad(g, y, al, be, wd, shp, xs, epi=e, out=out.t, part=part, tile=tile, nsplit=1, gs=gs, kg=kgv,
                      xn=xn, **kw)
        return out, part

    for det in (False, True):
        _native.set_deterministic(det)
        try:
            base, p0 = run(1, None)
            for xn in _xns(Nout):
                new, p1 = run(10, xn)
                assert torch.equal(new.bits(), base.bits()), (det, xn)
                assert p0 is None or torch.equal(_bits32(p1), _bits32(p0)), (det, xn)
                assert new.intact() and base.intact(), (det, xn)
        finally:
            _native.set_deterministic(False)
    if shape == REF_SHAPE and epi == "store":
        # the budget of tests/test_conv_kernels.py::test_conv_dgrad
        gt = (g.float() * (gs if scaled else 1.0) + al + be * y.float()).to(BF).float()
        ref = nhwc(torch.nn.grad.conv2d_input((N, Nout, H, H), w.to(BF).float(), nchw(gt)))
        out, _ = run(10, 2)
        assert rel(out.t, ref) < 1e-2, rel(out.t, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(512, 16, 128, 512), (512, 8, 256, 1024), (1024, 4, 512, 2048)])
def test_x1_many_workgroups_bit_identical(cuda, shape):
    """Hundreds of workgroups, two per CU, on a full GPU: the weight ring's buffer reuse is timing
    dependent (a refill racing a neighbour wave's fragment reads showed as 64-pixel x 16-channel
    blocks of wrong output at these sizes, never at the small ones above), so the comparison is
    repeated."""
    from faster_distributed_training_amd.ops import _native
    N, H, K, Nout = shape
    torch.manual_seed(2)
    tile = _tile(K)
    _native.set_deterministic(True)  # one statistics slot per row block (default mode shares slots here)
    try:
        _many_workgroups(cuda, N, H, K, Nout, tile)
    finally:
        _native.set_deterministic(False)


def _many_workgroups(cuda, N, H, K, Nout, tile):
    shp = ci.ConvShape(K, Nout, 1, 1, 0)
    x = make((N, H, H, K), cuda)
    w = torch.randn(Nout, K, 1, 1, device=cuda) / K ** 0.5
    wf, wd = ci.alloc_packed(shp, cuda)
    ci.pack_weights([(w, wf, wd, shp)])
    s, t = torch.randn(K, device=cuda), torch.randn(K, device=cuda) * 0.3
    p0 = ci.stat_slots(2, Nout, cuda, N * H * H)
    y0, _ = ci.conv_fwd(x, wf, shp, s, t, 1, 1.0, tile=tile, nsplit=1, kg=1, part=p0)
    # the same GEMM shape as a data gradient: conv Nout -> K, gradient [.., K] -> [.., Nout]
    shd = ci.ConvShape(Nout, K, 1, 1, 0)
    wdd = wf.reshape(Nout, 1, K)  # [Cin][taps][Cout] of the Nout -> K convolution
    yy = make((N, H, H, K), cuda)
    al, be = torch.randn(K, device=cuda) * 0.1, torch.randn(K, device=cuda) * 0.1
    xs = (N, H, H, Nout)
    d0, _ = ci.conv_dgrad(x, yy, al, be, wdd, shd, xs, tile=tile, nsplit=1, kg=1)
    for rep in range(3):
        for xn in (1, 2):
            p1 = ci.stat_slots(2, Nout, cuda, N * H * H)
            y1, _ = ci.conv_fwd(x, wf, shp, s, t, 1, 1.0, tile=tile, nsplit=1, kg=10, xn=xn, part=p1)
            assert torch.equal(y1.view(torch.int16), y0.view(torch.int16)), (rep, xn)
            assert torch.equal(_bits32(p1), _bits32(p0)), (rep, xn)
            d1, _ = ci.conv_dgrad(x, yy, al, be, wdd, shd, xs, tile=tile, nsplit=1, kg=10, xn=xn)
            assert torch.equal(d1.view(torch.int16), d0.view(torch.int16)), (rep, xn)


@pytest.mark.gpu
def test_x1_explicit_kg_on_unsupported_launch_is_an_error(cuda):
    """An explicit kg 10 outside the support set (a 3x3 convolution) is refused natively."""
    shp = ci.ConvShape(64, 128, 3, 1, 1)
    x = make((2, 4, 4, 64), cuda)
    w = torch.randn(128, 64, 3, 3, device=cuda)
    wf, _ = ci.alloc_packed(shp, cuda, dgrad=False)
    ci.pack_weights([(w, wf, None, shp)])
    with pytest.raises(RuntimeError, match="kg 10"):
        ci.conv_fwd(x, wf, shp, tile=(128, 128, 32), nsplit=1, kg=10)


@pytest.mark.gpu
def test_x1_engine_train_step_on_switched_table(cuda, monkeypatch):
    """The ResNet-50 engine step against the fp32 reference with every supported 1x1 launch switched
    to kg 10 by its table entry (the shipped table switches a measured subset)."""
    from test_resnet_engine import _train_step_vs_reference

    def tuned(op, batch, h, shp):
        if ci._is_pure(shp) and op in ("fwd0", "fwd1", "dgrad22"):
            K, nout = (shp.cin, shp.cout) if op.startswith("fwd") else (shp.cout, shp.cin)
            if nout % 128 == 0 and K >= 64:
                return {"tile": [64 if K >= 512 else 128, 128, 32], "nsplit": 1, "kg": 10, "xn": 2 if nout >= 1024 else 1}
        return None

    monkeypatch.setattr(ci, "tuned", tuned)
    ci.LAUNCH_LOG = []
    try:
        _train_step_vs_reference(cuda, "resnet50", batch=64)
        log = list(ci.LAUNCH_LOG)
    finally:
        ci.LAUNCH_LOG = None
    for kind in ("fwd", "dgrad"):
        assert sum(1 for e in log if e[0] == kind and e[5] == 10) >= 8, kind


# ---------------------------------------------------------------------------------- CPU
def test_x1_predicate_support_set():
    ok = ci.x1_ok
    assert ok(True, ci.PRO_AFFINE_ACT, ci.EPI_STATS, 1, 64, 256, 128, 128, 1)
    assert ok(True, ci.PRO_NONE, ci.EPI_STATS, 0, 256, 1024, 128, 128, 8)
    assert ok(True, ci.PRO_FOLD, ci.EPI_JOINBWD, 1, 512, 2048, 64, 128, 4)
    assert ok(True, ci.PRO_FOLD, ci.EPI_ADD, 0, 128, 256, 128, 128, 2)
    assert ok(True, ci.PRO_FOLD, ci.EPI_STORE, 0, 128, 512, 128, 128)
    assert not ok(False, ci.PRO_NONE, ci.EPI_STATS, 0, 64, 256, 128, 128)              # 3x3 / strided
    assert not ok(True, ci.PRO_AFFINE_ACT, ci.EPI_STATS, 2, 64, 256, 128, 128)         # CELU
    assert not ok(True, ci.PRO_NONE, ci.EPI_NORMACT, 0, 64, 256, 128, 128)             # frozen epilogue
    assert not ok(True, ci.PRO_FOLD, ci.EPI_ACTBWD, 1, 64, 256, 128, 128)
    assert not ok(True, ci.PRO_JOIN, ci.EPI_STATS, 1, 256, 64, 128, 128)
    assert not ok(True, ci.PRO_FOLD, ci.EPI_JOINBWD, 1, 64, 256, 128, 128, relu_mask=False)
    # the resident fragments fill the register budget at BM * K = 128 * 256 = 64 * 512
    assert not ok(True, ci.PRO_NONE, ci.EPI_STATS, 0, 512, 2048, 128, 128)
    assert not ok(True, ci.PRO_NONE, ci.EPI_STATS, 0, 1024, 2048, 64, 128)
    assert not ok(True, ci.PRO_NONE, ci.EPI_STATS, 0, 64, 256, 64, 128)                # (BM, K) not instantiated
    assert not ok(True, ci.PRO_NONE, ci.EPI_STATS, 0, 32, 256, 128, 128)               # K below one tile
    assert not ok(True, ci.PRO_NONE, ci.EPI_STATS, 0, 64, 192, 128, 128)               # Cout % BN
    assert not ok(True, ci.PRO_NONE, ci.EPI_STATS, 0, 64, 256, 128, 64)                # BN not instantiated
    assert not ok(True, ci.PRO_NONE, ci.EPI_STATS, 0, 64, 768, 128, 128, 4)            # xn does not divide 6
    # LDS of the largest header: two workgroups per CU at every K
    assert ci.x1_lds_bytes(ci.PRO_FOLD, ci.EPI_JOINBWD, 64) == 73472
    assert ci.x1_lds_bytes(ci.PRO_FOLD, ci.EPI_JOINBWD, 512) == 78848 <= ci.X1_LDS_MAX


def test_x1_table_entry_falls_back_to_its_tile():
    ent = {"tile": [128, 128, 32], "nsplit": 1, "kg": 10, "xn": 2, "loop": "rot"}
    t3 = tuple(ent["tile"])
    assert ci._kg(ent, None, t3, 1, 64, ci.PRO_NONE, True) == 10
    assert ci._loop_kg(ent, 10) == 10
    # not in the support set for this launch: the entry's tile on the implicit-GEMM kernel
    assert ci._kg(ent, None, t3, 1, 64, ci.PRO_NONE, False) == 1
    assert ci._loop_kg(ent, 1) == 4 and ci._tile3(ent["tile"], 100, 256) == t3
    # an explicit kg wins over the entry
    assert ci._kg(ent, 1, t3, 1, 64, ci.PRO_NONE, True) == 1
    assert ci._kg(None, 10, t3, 1, 64, ci.PRO_NONE, False) == 10


class _FakeNative:
    def __init__(self):
        self.calls = []

    def conv_igemm(self, *a):
        self.calls.append(a)


def test_x1_frozen_forward_over_a_switched_entry_keeps_the_implicit_gemm(monkeypatch):
    """fwd0 entries are shared with the frozen forward (EPI_NORMACT): an entry carrying "kg": 10
    sends the training launch to kg 10 (its nsplit argument carrying xn) and the frozen launch to
    the entry's tile on the implicit-GEMM kernel."""
    fake = _FakeNative()
    monkeypatch.setattr(ci._native, "native", lambda: fake)
    monkeypatch.setattr(ci, "_sp", lambda: 0)
    shp = ci.ConvShape(64, 256, 1, 1, 0)
    key = ci.tune_key(2, 4, shp)
    monkeypatch.setattr(ci, "_TUNED", {key: {"fwd0": {"tile": [128, 128, 32], "nsplit": 1, "kg": 10, "xn": 2}}})
    x = torch.zeros(2, 4, 4, 64, dtype=BF)
    wf = torch.zeros(256, 1, 64, dtype=BF)
    es, et = torch.ones(256), torch.zeros(256)
    ci.LAUNCH_LOG = []
    try:
        ci.conv_fwd(x, wf, shp, norm=(es, et))
        ci.conv_fwd(x, wf, shp, part=torch.zeros(1, 2, 256))
        log = list(ci.LAUNCH_LOG)
    finally:
        ci.LAUNCH_LOG = None
    frozen, train = log
    assert frozen[2] and frozen[3] == (128, 128, 32) and frozen[5] != 10
    assert train[2] and train[3] == (128, 128, 32) and train[5] == 10
    # native arguments: ..., BM, BN, BK, nsplit, slab, cnt, kg, stream, jz
    assert fake.calls[0][-9:-2] == (128, 128, 32, 1, 0, 0, 1)
    assert fake.calls[1][-9:-2] == (128, 128, 32, 2, 0, 0, 10)

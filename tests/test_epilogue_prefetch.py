"""The join-backward epilogue's operand prefetch (conv_epilogue's PF, csrc/kernels/conv_igemm_impl.h) on
the activation-stationary 1x1 kernel: the same launch with the switch off (operands loaded sweep by
sweep) and on (a pass's operands requested before its staging) -- output bits, statistics-slot bits
and the sentinels around the in-place output, in normal and deterministic mode, at every xn.  One
case is also held to an fp32 PyTorch evaluation: the incoming gradient is read from the buffer the
result is written to, and a load that slipped behind its store would be wrong on both sides of the
off / on comparison.  CPU tests: the switch's default and override."""
import pytest
import torch

from faster_distributed_training_amd.ops import conv_igemm as ci
from test_conv_x1 import BF, Guarded, _bits32, _slots, _tile, _xns, make, nchw, nhwc, rel

# (N, H, K, Nout) of the GEMM out[N*H*H][Nout] = X[N*H*H][K] W[Nout][K]^T
SHAPES = [
    (3, 5, 64, 256),    # M = 75 < BM: every hoisted sweep has rows past M; K = 64
    (4, 4, 64, 128),    # a single column tile
    (5, 6, 128, 512),   # M = 180: a full and a partial row block, 4 column tiles, K = 128: the ring's
                        # counted-vmcnt branch runs between prefetching epilogues
    (2, 4, 512, 2048),  # K = 512: the BM = 64 instantiation
]
REF_SHAPE = (5, 6, 128, 512)


def _problem(cuda, shape, shortcut, scaled, seed=3):
    N, H, K, Nout = shape
    torch.manual_seed(seed)
    shp = ci.ConvShape(Nout, K, 1, 1, 0)  # forward conv Nout -> K; its dgrad is the expanding GEMM
    w = torch.randn(K, Nout, 1, 1, device=cuda) / Nout ** 0.5
    _, wd = ci.alloc_packed(shp, cuda, fwd=False)
    ci.pack_weights([(w, None, wd, shp)])
    xs = (N, H, H, Nout)
    jo = make(xs, cuda)
    bits = (jo.reshape(-1, 8) > 0).to(torch.int32)
    mask = (bits << torch.arange(8, device=cuda, dtype=torch.int32)).sum(1).to(torch.uint8)
    return dict(shp=shp, w=w, wd=wd, xs=xs, g=make((N, H, H, K), cuda), y=make((N, H, H, K), cuda),
                al=torch.randn(K, device=cuda) * 0.1, be=torch.randn(K, device=cuda) * 0.1,
                gs=torch.randn(K, device=cuda) if scaled else None, prev=make(xs, cuda), ex=make(xs, cuda),
                jyb=make(xs, cuda) if shortcut else None, jo=jo, mask=mask, tile=_tile(K), M=N * H * H)


def _run(p, cuda, xn, prefetch, monkeypatch):
    monkeypatch.setattr(ci, "EPI_PREFETCH", prefetch)
    out = Guarded(p["xs"], cuda, init=p["prev"])
    part = _slots(3, p["xs"][3], cuda, p["M"], 11)
    ci.conv_dgrad(p["g"], p["y"], p["al"], p["be"], p["wd"], p["shp"], p["xs"], epi=ci.EPI_JOINBWD, out=out.t, part=part,
                  tile=p["tile"], nsplit=1, gs=p["gs"], kg=10, xn=xn, ex=p["ex"], act=1, jmask=p["mask"], jyb=p["jyb"])
    return out, part


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("shortcut", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
def test_prefetch_bit_identical_to_load_per_sweep(cuda, monkeypatch, shape, shortcut, scaled):
    from faster_distributed_training_amd.ops import _native
    p = _problem(cuda, shape, shortcut, scaled)
    for det in (False, True):
        _native.set_deterministic(det)
        try:
            for xn in _xns(shape[3]):
                base, p0 = _run(p, cuda, xn, False, monkeypatch)
                new, p1 = _run(p, cuda, xn, True, monkeypatch)
                assert torch.equal(new.bits(), base.bits()), (det, xn)
                assert torch.equal(_bits32(p1), _bits32(p0)), (det, xn)
                assert new.intact() and base.intact(), (det, xn)
        finally:
            _native.set_deterministic(False)


@pytest.mark.gpu
@pytest.mark.parametrize("shortcut", [False, True])
def test_prefetch_in_place_gradient_against_fp32(cuda, monkeypatch, shortcut):
    """out starts as the other branch's gradient: g_pre = (out + dA) * [join > 0], against fp32
    PyTorch with the budget of tests/test_conv_x1.py's reference case; the statistics rows
    (sum g_pre*ex, sum g_pre, sum g_pre*jyb) against the same evaluation with that file's budget
    for statistics (2e-3: both sides sum the same 180 fp32 terms per channel, in another order)."""
    N, H, K, Nout = REF_SHAPE
    p = _problem(cuda, REF_SHAPE, shortcut, True)
    gt = (p["g"].float() * p["gs"] + p["al"] + p["be"] * p["y"].float()).to(BF).float()
    dA = nhwc(torch.nn.grad.conv2d_input((N, Nout, H, H), p["w"].to(BF).float(), nchw(gt)))
    ref = (p["prev"].float() + dA) * (p["jo"] > 0).float()
    for xn in (1, 2):
        before = _slots(3, Nout, cuda, p["M"], 11).sum(0)
        out, part = _run(p, cuda, xn, True, monkeypatch)
        assert rel(out.t, ref) < 1e-2, (xn, rel(out.t, ref))
        st = part.sum(0) - before
        rf = ref.reshape(-1, Nout)
        assert rel(st[0], (rf * p["ex"].float().reshape(-1, Nout)).sum(0)) < 2e-3
        assert rel(st[1], rf.sum(0)) < 2e-3
        if shortcut:
            assert rel(st[2], (rf * p["jyb"].float().reshape(-1, Nout)).sum(0)) < 2e-3


# ---------------------------------------------------------------------------------- CPU
def test_prefetch_switch_default_and_override():
    assert ci.epi_prefetch_default({}) is True
    assert ci.epi_prefetch_default({"FDT_EPI_PREFETCH": "1"}) is True
    assert ci.epi_prefetch_default({"FDT_EPI_PREFETCH": "0"}) is False


class _FakeNative:
    def __init__(self):
        self.prefetch, self.launches = [], 0

    def set_conv_epi_prefetch(self, on):
        self.prefetch.append(on)

    def conv_igemm(self, *a):
        self.launches += 1


@pytest.mark.parametrize("on", [True, False])
def test_prefetch_switch_reaches_the_join_backward_launch(monkeypatch, on):
    """The stationary join-backward launch asks natively for the switch's value (off: the depth-0
    instantiation); the store epilogue and the implicit-GEMM kernel do not touch it."""
    fake = _FakeNative()
    monkeypatch.setattr(ci._native, "native", lambda: fake)
    monkeypatch.setattr(ci, "_sp", lambda: 0)
    monkeypatch.setattr(ci, "EPI_PREFETCH", on)
    shp = ci.ConvShape(256, 64, 1, 1, 0)
    xs = (2, 4, 4, 256)
    g, y = torch.zeros(2, 4, 4, 64, dtype=BF), torch.zeros(2, 4, 4, 64, dtype=BF)
    al, be, wd = torch.zeros(64), torch.zeros(64), torch.zeros(256, 1, 64, dtype=BF)
    out, ex = torch.zeros(xs, dtype=BF), torch.zeros(xs, dtype=BF)
    part, mask = torch.zeros(1, 3, 256), torch.zeros(2 * 4 * 4 * 256 // 8, dtype=torch.uint8)
    kw = dict(out=out, tile=(128, 128, 32), nsplit=1)
    ci.conv_dgrad(g, y, al, be, wd, shp, xs, epi=ci.EPI_STORE, kg=10, **kw)
    ci.conv_dgrad(g, y, al, be, wd, shp, xs, epi=ci.EPI_JOINBWD, kg=1, ex=ex, part=part, act=1, jmask=mask, **kw)
    assert fake.prefetch == [] and fake.launches == 2
    ci.conv_dgrad(g, y, al, be, wd, shp, xs, epi=ci.EPI_JOINBWD, kg=10, ex=ex, part=part, act=1, jmask=mask, **kw)
    assert fake.prefetch == [on] and fake.launches == 3

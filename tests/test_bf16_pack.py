"""Bit-exactness of the packed bf16 helpers (csrc/kernels/common.h): ``pack_bf16x2`` -- one
vector convert for a pair of floats -- and ``relu_bf16x2`` -- the ReLU of the conv staging
prologues, applied to the packed pair as a signed 16-bit max with 0."""
import struct

import pytest
import torch
import torch.nn.functional as F

from faster_distributed_training_amd.ops import _native
from faster_distributed_training_amd.ops import conv_igemm as ci

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


# fp32 bit patterns -> the bf16 bits round-to-nearest-even must give
EDGES = [
    (0x3F808000, 0x3F80),  # tie, even below: rounds down
    (0x3F818000, 0x3F82),  # tie, odd below: rounds up
    (0x3F808001, 0x3F81),  # just above a tie
    (0x3F807FFF, 0x3F80),  # just below a tie
    (0xBF808000, 0xBF80),  # the same ties, negative
    (0xBF818000, 0xBF82),
    (0x7F7FFFFF, 0x7F80),  # largest finite fp32 -> +inf
    (0xFF7FFFFF, 0xFF80),
    (0x7F7F7FFF, 0x7F7F),  # just below the tie under the largest finite bf16
    (0x7F7F8000, 0x7F80),  # tie at the largest finite bf16 (odd) -> +inf
    (0x00000001, 0x0000),  # smallest fp32 denormal -> +0
    (0x80000001, 0x8000),
    (0x00008000, 0x0000),  # tie between 0 and the smallest bf16 denormal -> even (0)
    (0x00008001, 0x0001),
    (0x00018000, 0x0002),  # denormal tie, odd below
    (0x007FFFFF, 0x0080),  # largest denormal -> smallest normal
    (0x00400000, 0x0040),  # a denormal bf16 holds exactly
    (0x00000000, 0x0000),
    (0x80000000, 0x8000),
    (0x7F800000, 0x7F80),
    (0xFF800000, 0xFF80),
    (0x7FC00000, 0x7FC0),  # canonical quiet NaN
]
NANS = [0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F800001, 0x7F80FFFF]  # stay NaN, whatever the payload


def test_pack_bf16x2_bits(cuda):
    """A table of fp32 edge values through ``cast_bf16`` (whose stores are ``pack_bf16x2``
    pairs), every value in the low and in the high half of a pair: the same bits as
    ``Tensor.to(torch.bfloat16)`` and as the table."""
    nat = _native.native()
    vals = [b for b, _ in EDGES]
    want = [w for _, w in EDGES]
    if len(vals) % 2 == 0:  # an odd count, so that the doubled table puts each value in both halves
        vals.append(0x3F800000)
        want.append(0x3F80)
    bits = vals + vals
    while len(bits) % 4:
        bits.append(0)
    n_edges = 2 * len(vals)
    x = torch.tensor(bits, dtype=torch.int64).to(torch.int32).to(cuda).view(torch.float32)
    y = torch.full((x.numel(),), float("nan"), device=cuda, dtype=BF)
    nat.cast_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _native.stream_ptr())
    torch.cuda.synchronize()
    got = (y.view(torch.int16).to(torch.int32) & 0xFFFF).tolist()
    ref = (x.to(BF).view(torch.int16).to(torch.int32) & 0xFFFF).tolist()
    for i in range(n_edges):
        assert got[i] == ref[i] == (want + want)[i], (i, hex(bits[i]), hex(got[i]), hex(ref[i]))
    # NaNs of either sign and any payload stay NaN, in either half
    nb = NANS + [0x3F800000] + NANS + [0x3F800000]
    xn = torch.tensor(nb, dtype=torch.int64).to(torch.int32).to(cuda).view(torch.float32)
    yn = torch.zeros(xn.numel(), device=cuda, dtype=BF)
    nat.cast_bf16(xn.data_ptr(), yn.data_ptr(), xn.numel(), _native.stream_ptr())
    assert torch.equal(torch.isnan(yn), torch.isnan(xn))
    assert yn[len(NANS)].item() == 1.0


def _edge_rows(dev, C):
    """[2][C] bf16 rows of values a ReLU-after-rounding could get wrong: +-0, the smallest
    normals, values next to zero, +inf, large magnitudes of both signs."""
    e = [0.0, -0.0, f32(0x00800000), f32(0x80800000), 1e-30, -1e-30, float("inf"), -3.0e38, 3.0e38,
         -1.0, 1.0, -2.0 ** -100, 2.0 ** -100, -0.00390625, 0.00390625, -65280.0]
    row = torch.tensor((e * (C // len(e) + 1))[:C], device=dev, dtype=torch.float32).to(BF)
    return torch.stack([row, row.flip(0)])


@pytest.mark.parametrize("case", [(3, 5, 64, 256), (2, 8, 256, 384)])
@pytest.mark.parametrize("tile", [(128, 128, 32), (64, 64, 64), (128, 64, 64)])
def test_join_prologue_relu_bits(cuda, case, tile):
    """PRO_JOIN with unit scales (z = y + r is then exact in fp32 on both sides): the stored
    join output holds exactly the bits of relu(z) rounded to bf16 -- never a set sign bit --
    and the mask bit is z > 0 from the fp32 value."""
    N, H, C, Cout = case
    torch.manual_seed(11)
    shp = ci.ConvShape(C, Cout, 1, 1, 0)
    y = torch.randn(N, H, H, C, device=cuda).to(BF)
    r = (torch.randn(N, H, H, C, device=cuda) * 0.5).to(BF)
    y.view(-1, C)[:2] = _edge_rows(cuda, C)
    r.view(-1, C)[:2] = 0
    y.view(-1, C)[2:4] = 0
    r.view(-1, C)[2:4] = _edge_rows(cuda, C)
    s = torch.ones(C, device=cuda)
    t = torch.zeros(C, device=cuda)
    w = torch.randn(Cout, C, 1, 1, device=cuda) / C ** 0.5
    wf, _ = ci.alloc_packed(shp, cuda, dgrad=False)
    ci.pack_weights([(w, wf, None, shp)])
    z = y.float() + r.float()
    want = torch.relu(z).to(BF)
    want_mask = (z.reshape(-1, 8) > 0).to(torch.int32)
    want_mask = (want_mask << torch.arange(8, device=cuda, dtype=torch.int32)).sum(1).to(torch.uint8)
    jout = torch.full_like(y, float("nan"))
    jmask = torch.zeros(y.numel() // 8, device=cuda, dtype=torch.uint8)
    ci.conv_fwd_join(y, r, s, t, None, None, wf, shp, jout, jmask, tile=tile, nsplit=1, kg=1)
    assert torch.equal(jout, want)
    assert (jout.view(torch.int16) >= 0).all(), "a ReLU output with the sign bit set"
    assert torch.equal(jmask, want_mask)


@pytest.mark.parametrize("case", [(3, 5, 64, 256), (2, 8, 256, 384)])
@pytest.mark.parametrize("tile", [(128, 128, 32), (64, 64, 64)])
def test_affine_prologue_relu_matches_materialised(cuda, case, tile):
    """PRO_AFFINE_ACT with ReLU and (s, t) = (1, 0) stages exactly relu(x): the same output and
    statistics, bit for bit, as the prologue-free kernel on a materialised relu(x) (same tile,
    same K loop, hence the same MFMA sequence); with a random affine, the fp32 oracle."""
    N, H, C, Cout = case
    torch.manual_seed(12)
    shp = ci.ConvShape(C, Cout, 1, 1, 0)
    x = torch.randn(N, H, H, C, device=cuda).to(BF)
    # (the edge rows with their large magnitudes cut to 225, so that the statistics' sums of
    # squares stay in range)
    x.view(-1, C)[:2] = _edge_rows(cuda, C).float().clamp(-225.0, 225.0).to(BF)
    w = torch.randn(Cout, C, 1, 1, device=cuda) / C ** 0.5
    wf, _ = ci.alloc_packed(shp, cuda, dgrad=False)
    ci.pack_weights([(w, wf, None, shp)])
    one = torch.ones(C, device=cuda)
    zero = torch.zeros(C, device=cuda)
    y1, _ = ci.conv_fwd(x, wf, shp, one, zero, 1, 1.0, tile=tile, nsplit=1, kg=1)
    y0, _ = ci.conv_fwd(torch.relu(x), wf, shp, tile=tile, nsplit=1, kg=1)
    assert torch.equal(y1, y0)
    # random affine against fp32 PyTorch, the tolerances of test_conv_kernels.py
    s = torch.rand(C, device=cuda) + 0.5
    t = torch.randn(C, device=cuda) * 0.3
    a = torch.relu(x.float() * s + t).to(BF).float()
    ref = F.conv2d(a.permute(0, 3, 1, 2), w.to(BF).float()).permute(0, 2, 3, 1)
    y2, p2 = ci.conv_fwd(x, wf, shp, s, t, 1, 1.0, tile=tile, nsplit=1, kg=1)
    rel = lambda u, v: ((u.float() - v.float()).norm() / (v.float().norm() + 1e-12)).item()  # noqa: E731
    assert rel(y2, ref) < 1e-2
    ps = p2.sum(0)
    yf = ref.reshape(-1, Cout)
    assert rel(ps[0], yf.sum(0)) < 2e-3 and rel(ps[1], (yf * yf).sum(0)) < 2e-3

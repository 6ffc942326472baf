"""CutMix: the host mirror of the box draw, ``cutmix_data`` on the CPU, the trainer / CLI
switches (CPU), and the ``cutmix_prep`` / ``cutmix_fwd`` / ``cutmix_bwd`` kernels against
them (GPU)."""
import math

import pytest
import torch

from faster_distributed_training_amd.ops import mixup as M

SEED = 20240611  # (checked: per-sample centres at b = 1024 cover all 32 rows and columns)


def _area_lam(box, H, W):
    bx = box.long()
    area = ((bx[:, 1] - bx[:, 0]) * (bx[:, 3] - bx[:, 2])).float()
    return 1.0 - area / torch.tensor(float(H * W), dtype=torch.float32)


def _select_oracle(x, perm, box):
    """Explicit indexing: out[i] = x[i] with box i cut out of x[perm[i]] (dense CPU NCHW)."""
    xc = x.detach().cpu().contiguous()
    out = xc.clone()
    for i in range(xc.shape[0]):
        y0, y1, x0, x1 = [int(v) for v in box[i]]
        out[i, :, y0:y1, x0:x1] = xc[int(perm[i]), :, y0:y1, x0:x1]
    return out


# ------------------------------------------------------------------------------ cutmix_boxes
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("H,W,bh,bw", [(32, 32, 13, 20), (5, 7, 3, 4), (32, 32, 1, 1), (9, 4, 9, 4)])
def test_boxes_bounds_and_extent(H, W, bh, bw, per_sample):
    box, lam = M.cutmix_boxes(SEED, 257, H, W, bh, bw, per_sample)
    assert box.dtype == torch.int32 and box.shape == (257, 4) and lam.dtype == torch.float32 and lam.shape == (257,)
    y0, y1, x0, x1 = box.long().unbind(1)
    assert bool(((0 <= y0) & (y0 <= y1) & (y1 <= H)).all()) and bool(((0 <= x0) & (x0 <= x1) & (x1 <= W)).all())
    assert bool((y1 - y0 <= 2 * (bh // 2)).all()) and bool((x1 - x0 <= 2 * (bw // 2)).all())
    free_y, free_x = (y0 > 0) & (y1 < H), (x0 > 0) & (x1 < W)  # the box touches neither edge
    assert bool((y1 - y0 == 2 * (bh // 2))[free_y].all()) and bool((x1 - x0 == 2 * (bw // 2))[free_x].all())
    assert torch.equal(lam, _area_lam(box, H, W))
    if not per_sample:
        assert bool((box == box[0]).all()) and bool((lam == lam[0]).all())


def test_boxes_empty_and_full():
    for per_sample in (False, True):
        box, lam = M.cutmix_boxes(SEED, 64, 32, 32, 0, 0, per_sample)
        assert bool((box[:, 0] == box[:, 1]).all()) and bool((box[:, 2] == box[:, 3]).all())
        assert bool((lam == 1.0).all())
        box, lam = M.cutmix_boxes(SEED, 64, 32, 32, 32, 32, per_sample)
        assert torch.equal(lam, _area_lam(box, 32, 32)) and bool((lam < 1.0).all())
        # a full-size box around a centre: at least the centre's quadrant, at most the image
        assert bool(((box[:, 1] - box[:, 0]) >= 16).all()) and bool(((box[:, 3] - box[:, 2]) >= 16).all())


def test_boxes_centres_cover_the_image():
    """Per-sample mode, b = 1024 on 32 x 32: every row and every column occurs as a centre
    (bh = bw = 2: the box ends at min(c + 1, 32) = c + 1, so the centre is c = y1 - 1)."""
    box, _ = M.cutmix_boxes(SEED, 1024, 32, 32, 2, 2, True)
    y0, y1, x0, x1 = box.long().unbind(1)
    cy, cx = y1 - 1, x1 - 1
    assert sorted(set(cy.tolist())) == list(range(32)) and sorted(set(cx.tolist())) == list(range(32))
    # and the per-batch draw is the per-sample draw of sample 0
    one, _ = M.cutmix_boxes(SEED, 4, 32, 32, 2, 2, False)
    assert bool((one == box[0]).all())
    with pytest.raises(ValueError):
        M.cutmix_boxes(SEED, 4, 32, 32, 33, 2, False)


def test_seeded_permutation_is_a_permutation():
    p = M.seeded_permutation(SEED, 1000)
    assert torch.equal(p.sort().values, torch.arange(1000))
    assert not torch.equal(p, M.seeded_permutation(SEED + 1, 1000))


# ------------------------------------------------------------------------------ cutmix_data (CPU)
@pytest.mark.parametrize("per_sample", [False, True])
def test_cutmix_data_cpu_matches_pixel_loop(per_sample):
    torch.manual_seed(0)
    B, C, H, W = 5, 3, 6, 7
    x = torch.randn(B, C, H, W)
    y = torch.arange(B) * 3 + 1
    g = torch.Generator().manual_seed(11)
    mixed, ya, yb, lam_vec = M.cutmix_data(x, y, alpha=1.0, per_sample=per_sample, generator=g)
    # replay the host draws
    g2 = torch.Generator().manual_seed(11)
    lam = M.sample_lambda(1.0, g2)
    seed = int(torch.randint(0, 2**62, (1,), generator=g2).item())
    r = math.sqrt(1.0 - lam)
    box, lv = M.cutmix_boxes(seed, B, H, W, int(H * r), int(W * r), per_sample)
    perm = M.seeded_permutation(seed, B)
    assert ya is y and torch.equal(yb, y[perm])
    assert torch.equal(lam_vec, lv) and torch.equal(lam_vec, _area_lam(box, H, W))
    ref = torch.empty_like(x)
    for i in range(B):
        for h in range(H):
            for w in range(W):
                inside = box[i, 0] <= h < box[i, 1] and box[i, 2] <= w < box[i, 3]
                ref[i, :, h, w] = x[perm[i], :, h, w] if inside else x[i, :, h, w]
    assert torch.equal(mixed, ref)
    assert torch.equal(mixed, _select_oracle(x, perm, box))


def test_cutmix_data_cpu_lambda_one_and_autograd():
    x = torch.randn(4, 3, 6, 7)
    y = torch.arange(4)
    mixed, ya, yb, lam_vec = M.cutmix_data(x, y, alpha=0.0)  # alpha <= 0: lambda = 1, nothing pasted
    assert torch.equal(mixed, x) and bool((lam_vec == 1.0).all())
    xg = x.clone().requires_grad_()
    g = torch.Generator().manual_seed(5)
    mixed, _, _, _ = M.cutmix_data(xg, y, alpha=1.0, per_sample=True, generator=g)
    mixed.sum().backward()
    assert xg.grad is not None and float(xg.grad.sum()) == x.numel()  # every output pixel has one source


# ------------------------------------------------------------------------------ config, CLI, trainer (CPU)
def test_config_refusals():
    from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="cutmix_prob"):
            ResNetConfig(cutmix_prob=bad)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="label_smoothing"):
            ResNetConfig(label_smoothing=bad)
    with pytest.raises(ValueError, match="meta_learning"):
        ResNetConfig(cutmix_prob=0.5, meta_learning=True)
    c = ResNetConfig(cutmix_prob=1.0, label_smoothing=0.0)
    assert (c.cutmix_alpha, c.cutmix_per_sample) == (1.0, False)
    d = ResNetConfig()
    assert (d.cutmix_prob, d.cutmix_alpha, d.cutmix_per_sample, d.label_smoothing) == (0.0, 1.0, False, 0.0)


def test_cli_flags():
    import resnet_infer
    a, base = resnet_infer.parse(["--cutmix_prob", "0.5", "--cutmix_alpha", "0.7", "--cutmix_per_sample",
                                  "--label_smoothing", "0.1", "--synthetic", "--bs", "16"])
    cfg = resnet_infer.config_from_args(a, base)
    assert (cfg.cutmix_prob, cfg.cutmix_alpha, cfg.cutmix_per_sample, cfg.label_smoothing) == (0.5, 0.7, True, 0.1)
    assert cfg.bs == 16 and cfg.synthetic
    a, base = resnet_infer.parse(["--synthetic"])
    cfg = resnet_infer.config_from_args(a, base)
    assert (cfg.cutmix_prob, cfg.cutmix_alpha, cfg.cutmix_per_sample, cfg.label_smoothing) == (0.0, 1.0, False, 0.0)
    with pytest.raises(SystemExit):
        resnet_infer.parse(["--cutmix_prob", "0.5", "--meta_learning"])
    with pytest.raises(SystemExit):
        resnet_infer.parse(["--label_smoothing", "1.0"])


def _cpu_cfg(tmp_path, **kw):
    from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig
    base = dict(arch="resnet18", bs=8, epoch=1, synthetic=True, eval=False, plot=False, steps_per_epoch=2,
                checkpoint_dir=str(tmp_path), optimizer="madgrad", seed=7, extra={"subset_stride": 50})
    base.update(kw)
    return ResNetConfig(**base)


def test_trainer_cpu_cutmix_run_and_unchanged_default(tmp_path, monkeypatch):
    import json
    from faster_distributed_training_amd.train.resnet_trainer import ResNetTrainer
    monkeypatch.setenv("FDT_NATIVE", "0")
    log = tmp_path / "cm.jsonl"
    t = ResNetTrainer(_cpu_cfg(tmp_path, cutmix_prob=1.0, label_smoothing=0.1, log_path=str(log)))
    rec = t.train_epoch(0)
    assert rec["steps"] == 2 and math.isfinite(rec["train_loss"])
    with open(log) as f:
        first = json.loads(f.readline())
    assert first["config"]["cutmix_prob"] == 1.0 and first["config"]["label_smoothing"] == 0.1
    assert first["config"]["cutmix_alpha"] == 1.0 and first["config"]["cutmix_per_sample"] is False
    # the new fields at their defaults change nothing
    named = ResNetTrainer(_cpu_cfg(tmp_path, cutmix_prob=0.0, label_smoothing=0.0)).train_epoch(0)
    plain = ResNetTrainer(_cpu_cfg(tmp_path)).train_epoch(0)
    assert named["train_loss"] == plain["train_loss"] and named["train_acc"] == plain["train_acc"]
    assert rec["train_loss"] != plain["train_loss"]


# ------------------------------------------------------------------------------ GPU: cutmix_prep
@pytest.mark.gpu
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("H,W,bh,bw", [(32, 32, 0, 0), (32, 32, 32, 32), (32, 32, 13, 20), (5, 7, 3, 4)])
@pytest.mark.parametrize("b", [1, 5, 64, 1024])
def test_cutmix_prep_matches_host_mirror(cuda, b, H, W, bh, bw, per_sample):
    from faster_distributed_training_amd.ops import _native
    nat = _native.native()
    seed = SEED + 17 * b
    y = torch.randint(0, 100, (b,), device=cuda)
    perm = torch.empty(b, device=cuda, dtype=torch.int32)
    yb = torch.empty(b, device=cuda, dtype=torch.int64)
    box = torch.full((b, 4), -1, device=cuda, dtype=torch.int32)
    lv = torch.empty(b, device=cuda, dtype=torch.float32)
    nat.cutmix_prep(y.data_ptr(), b, H, W, bh, bw, int(per_sample), seed, perm.data_ptr(), yb.data_ptr(),
                    box.data_ptr(), lv.data_ptr(), _native.stream_ptr())
    perm_m = torch.empty(b, device=cuda, dtype=torch.int32)
    yb_m = torch.empty(b, device=cuda, dtype=torch.int64)
    lv_m = torch.empty(b, device=cuda, dtype=torch.float32)
    nat.mixup_prep(y.data_ptr(), b, 0.25, seed, perm_m.data_ptr(), yb_m.data_ptr(), lv_m.data_ptr(),
                   _native.stream_ptr())
    ref_box, ref_lv = M.cutmix_boxes(seed, b, H, W, bh, bw, per_sample)
    assert torch.equal(box.cpu(), ref_box)
    assert torch.equal(lv.cpu(), ref_lv)  # bit for bit
    assert torch.equal(perm, perm_m) and torch.equal(perm.cpu().long(), M.seeded_permutation(seed, b))
    assert torch.equal(yb, y[perm.long()]) and torch.equal(yb, yb_m)


@pytest.mark.gpu
@pytest.mark.parametrize("per_sample", [False, True])
def test_cutmix_data_gpu_equals_cpu(cuda, per_sample):
    """The same generator state gives the same permutation, boxes and mixed batch on both paths."""
    torch.manual_seed(3)
    x = torch.randn(64, 3, 32, 32)
    y = torch.randint(0, 10, (64,))
    mc, _, ybc, lvc = M.cutmix_data(x, y, 1.0, per_sample, torch.Generator().manual_seed(9))
    yg = y.to(cuda)
    mg, yag, ybg, lvg = M.cutmix_data(x.to(cuda), yg, 1.0, per_sample, torch.Generator().manual_seed(9))
    assert yag is yg and torch.equal(mg.cpu(), mc) and torch.equal(ybg.cpu(), ybc) and torch.equal(lvg.cpu(), lvc)


# ------------------------------------------------------------------------------ GPU: cutmix_fwd / bwd
def _hand_boxes(H, W):
    """Empty, full, clipped at the top-left corner, clipped at the bottom-right corner, interior with
    an x-range that starts and ends off an 8-element boundary (3..13 where the image allows), one pixel."""
    xe = 13 if W > 13 else W - 1
    return torch.tensor([[2, 2, 4, 4], [0, H, 0, W], [0, H // 2 + 1, 0, min(W, 9) - 2],
                         [H - 3, H, W - 3, W], [1, H - 1, 3, xe], [H // 2, H // 2 + 1, W - 2, W - 1]],
                        dtype=torch.int32)


def _perm_with_fixed_point(n):
    p = list(range(n))
    p[0], p[n - 1] = p[n - 1], p[0]
    if n > 4:
        p[2], p[3] = p[3], p[2]
    return torch.tensor(p)  # (index 1 stays a fixed point)


def _make(layout, cuda):
    """x on the GPU in the layout under test."""
    torch.manual_seed(1)
    if layout == "nhwc_bf16":
        N, C, H, W, cp = 5, 3, 32, 32, 8
        buf = torch.zeros(N, H, W, cp, device=cuda, dtype=torch.bfloat16)
        buf[..., :C] = torch.randn(N, H, W, C, device=cuda).to(torch.bfloat16)
        x = buf.permute(0, 3, 1, 2)[:, :C]
        assert M.padded_channels_last(x) == cp
        return x
    shape, dt = {"nchw_bf16": ((5, 3, 32, 32), torch.bfloat16), "nchw_fp32_scalar": ((5, 3, 5, 7), torch.float32),
                 "nchw_fp16": ((4, 8, 8, 8), torch.float16), "nchw_fp32_vec": ((4, 2, 6, 16), torch.float32)}[layout]
    return torch.randn(*shape, device=cuda).to(dt)


LAYOUTS = ["nhwc_bf16", "nchw_bf16", "nchw_fp32_scalar", "nchw_fp16", "nchw_fp32_vec"]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_cutmix_fwd_hand_boxes(cuda, layout):
    x = _make(layout, cuda)
    N, C, H, W = x.shape
    boxes = _hand_boxes(H, W)
    perm = _perm_with_fixed_point(N)
    for sel in (boxes[:N], boxes[-N:]):  # every box kind, N samples per launch
        out = M.cutmix_select(x, perm.to(cuda), sel.to(cuda))
        assert out.shape == x.shape and out.dtype == x.dtype
        assert torch.equal(out.cpu().contiguous(), _select_oracle(x, perm, sel))
        if layout == "nhwc_bf16":
            assert M.padded_channels_last(out) == 8  # the layout is kept ...
            whole = torch.as_strided(out, (N, H, W, 8), (H * W * 8, W * 8, 8, 1))
            assert int(torch.count_nonzero(whole[..., C:])) == 0  # ... and the pad channels are still zero
            assert torch.equal(whole[..., :C].permute(0, 3, 1, 2), out)
        else:
            assert out.is_contiguous()


def _ulp_bf16(ref):
    _, e = torch.frexp(ref.abs().float())  # |ref| = m * 2^e, m in [0.5, 1): bf16 ulp = 2^(e - 8)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float32), e - 8)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_cutmix_bwd_against_autograd(cuda, layout):
    x = _make(layout, cuda)
    N, C, H, W = x.shape
    perm = _perm_with_fixed_point(N)
    assert int(perm[1]) == 1
    boxes = _hand_boxes(H, W)
    torch.manual_seed(2)
    g = torch.randn(N, C, H, W).to(x.dtype)
    for sel in (boxes[:N], boxes[-N:]):
        xg = x.detach().requires_grad_()
        out = M.cutmix_select(xg, perm.to(cuda), sel.to(cuda))
        gout = g.to(cuda)
        if layout == "nhwc_bf16":  # the gradient arrives in the layout of the output
            gb = torch.zeros(N, H, W, 8, device=cuda, dtype=x.dtype)
            gb[..., :C] = gout.permute(0, 2, 3, 1)
            gout = gb.permute(0, 3, 1, 2)[:, :C]
        out.backward(gout)
        # oracle: torch autograd through the indexing form, in fp32
        x2 = x.detach().cpu().float().contiguous().requires_grad_()
        ref = torch.where(M._box_mask(sel, H, W), x2[perm], x2)
        ref.backward(g.float())
        got = xg.grad.cpu().float()
        assert torch.equal(got[1], g[1].float())  # the fixed point: gx[i] == g[i]
        if x.dtype == torch.float32:
            assert torch.equal(got, x2.grad)  # at most two terms per element: exact
        elif x.dtype == torch.bfloat16:
            assert bool(((got - x2.grad).abs() <= _ulp_bf16(x2.grad)).all())
        else:
            assert torch.allclose(got, x2.grad, rtol=2.0 ** -10, atol=1e-7)  # one fp16 ulp


# ------------------------------------------------------------------------------ GPU: one engine step
@pytest.mark.gpu
def test_engine_step_with_cutmix_and_smoothing(cuda, tmp_path):
    from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig, ResNetTrainer
    cfg = ResNetConfig(arch="resnet18", bs=32, epoch=1, synthetic=True, eval=False, plot=False, steps_per_epoch=2,
                       checkpoint_dir=str(tmp_path), optimizer="madgrad", seed=7, precision="bf16", graphs=True,
                       cutmix_prob=1.0, label_smoothing=0.1, extra={"subset_stride": 50})
    tr = ResNetTrainer(cfg)
    seen = []
    tr.model.register_forward_pre_hook(lambda m, inp: seen.append(M.padded_channels_last(inp[0])))
    before = tr.flat.data.detach().clone()
    it = iter(tr.train_loader)
    losses = [float(tr.train_step(*next(it)).detach()) for _ in range(2)]
    assert all(math.isfinite(v) for v in losses)
    assert not torch.equal(before, tr.flat.data)
    assert seen == [8, 8]  # the stem takes the same padded-NHWC path as with mixup
    m = tr.meter.reduced()
    assert math.isfinite(m["loss"]) and m["total"] == 64.0

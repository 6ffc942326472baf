"""Layer-wise adaptive rates over the flat buffers: LARS and LAMB (optim/flat_optim.py,
csrc/kernels/optim_layerwise.hip).

CPU: the torch-op paths against an independent fp64 per-tensor reference written here (no
FlatParams), the reduction to flat SGD, state_dict round trips, skipped steps, the --fsdp refusal
and the trainers' trust_* log fields.  GPU: the HIP kernels against fp64 trust ratios, against the
CPU path, poisoned alignment padding, determinism, skipped steps, a partitioned layout and the
ResNet engine."""
import json
import math

import pytest
import torch
import torch.nn as nn

from faster_distributed_training_amd.optim import flat_optim as O
from faster_distributed_training_amd.utils.flat import FlatParams

TOL = dict(atol=1e-6, rtol=1e-5)  # as tests/test_optim.py


# ------------------------------------------------------------------------------ fp64 reference
class _Net(nn.Module):
    """A 2-D weight, a 1-D bias, a 4-D weight, and a 2-D weight whose gradient stays zero."""

    def __init__(self, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.lin = nn.Linear(6, 5)
        self.conv = nn.Conv2d(2, 3, 3, bias=False)
        self.still = nn.Parameter(torch.randn(4, 3))


def _grads(params, seed, zero=("still",)):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.zeros(p.shape) if any(z in n for z in zero) else torch.randn(p.shape, generator=g)
            for n, p in params]


def _ref_lars(params, steps, coefs, lr, momentum, nesterov, wd, eta, eps, exclude_1d):
    """The rule as the paper and the project's documentation state it, per tensor, in fp64."""
    ps = [p.detach().double().clone() for p in params]
    bufs = [None] * len(ps)
    for grads, c in zip(steps, coefs):
        c = 1.0 if c is None else c
        for i, (p, g) in enumerate(zip(ps, grads)):
            g = g.double()
            adapted = p.ndim > 1 or not exclude_1d
            wd_s = wd if adapted else 0.0
            wn, gn = p.norm().item(), c * g.norm().item()
            q = eta * wn / (gn + wd_s * wn + eps) if (adapted and wn > 0 and gn > 0) else 1.0
            d = q * (c * g + wd_s * p)
            if momentum != 0:
                bufs[i] = d.clone() if bufs[i] is None else momentum * bufs[i] + d
                d = d + momentum * bufs[i] if nesterov else bufs[i]
            ps[i] = p - lr * d
    return ps


def _ref_lamb(params, steps, coefs, lr, b1, b2, eps, wd, exclude_1d):
    ps = [p.detach().double().clone() for p in params]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    trust = []
    for t, (grads, c) in enumerate(zip(steps, coefs), start=1):
        c = 1.0 if c is None else c
        trust = []
        for i, (p, g) in enumerate(zip(ps, grads)):
            g = c * g.double()
            adapted = p.ndim > 1 or not exclude_1d
            ms[i] = b1 * ms[i] + (1 - b1) * g
            vs[i] = b2 * vs[i] + (1 - b2) * g * g
            u = (ms[i] / (1 - b1 ** t)) / ((vs[i] / (1 - b2 ** t)).sqrt() + eps) + (wd if adapted else 0.0) * p
            wn, un = p.norm().item(), u.norm().item()
            q = wn / un if (adapted and wn > 0 and un > 0) else 1.0
            trust.append(q)
            ps[i] = p - lr * q * u
    return ps, trust


def _drive(net, opt, steps, coefs, device="cpu"):
    params = list(net.parameters())
    for grads, c in zip(steps, coefs):
        for p, g in zip(params, grads):
            p.grad.copy_(g)
        opt.step(grad_scale=None if c is None else torch.tensor([c], dtype=torch.float32, device=device))


# ------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("momentum,nesterov,wd,clip,exclude_1d", [
    (0.0, False, 0.0, False, True), (0.9, False, 5e-4, False, True), (0.9, True, 5e-4, True, True),
    (0.9, False, 5e-4, True, False), (0.0, False, 5e-4, True, False), (0.9, True, 0.0, False, False)])
def test_lars_cpu_matches_fp64_reference(momentum, nesterov, wd, clip, exclude_1d):
    net = _Net()
    init = [p.detach().clone() for p in net.parameters()]
    steps = [_grads(net.named_parameters(), s) for s in range(5)]
    coefs = [0.5 if (clip and s % 2 == 0) else None for s in range(5)]
    flat = FlatParams(net)
    # (eta far above the training default so that the adapted update is well above the tolerance)
    opt = O.LARS(flat, lr=0.5, momentum=momentum, nesterov=nesterov, weight_decay=wd, eta=0.05, exclude_1d=exclude_1d)
    _drive(net, opt, steps, coefs)
    ref = _ref_lars(init, steps, coefs, 0.5, momentum, nesterov, wd, 0.05, 1e-8, exclude_1d)
    for (n, p), r, p0 in zip(net.named_parameters(), ref, init):
        assert torch.allclose(p, r.float(), **TOL), n
        assert not torch.allclose(p, p0, atol=1e-4) or (wd == 0 and "still" in n), n  # it moved
    # the zero-gradient slot and (when excluded) the bias have q = 1
    by_name = {sl.name: float(opt.trust[i]) for i, sl in enumerate(flat.slots)}
    assert by_name["still"] == 1.0
    assert (by_name["lin.bias"] == 1.0) == exclude_1d
    assert 0 < by_name["lin.weight"] < 1.0 and by_name["lin.weight"] != by_name["conv.weight"]
    s = opt.trust_summary()
    adapted = [v for n, v in by_name.items() if exclude_1d is False or not n.endswith("bias")]
    assert s["min"] == min(adapted) and s["max"] == max(adapted) and s["min"] <= s["med"] <= s["max"]


@pytest.mark.parametrize("wd,clip,exclude_1d", [(0.0, False, True), (0.01, True, True), (0.01, False, False)])
def test_lamb_cpu_matches_fp64_reference(wd, clip, exclude_1d):
    net = _Net()
    init = [p.detach().clone() for p in net.parameters()]
    steps = [_grads(net.named_parameters(), s) for s in range(5)]
    coefs = [0.5 if (clip and s % 2 == 0) else None for s in range(5)]
    flat = FlatParams(net)
    opt = O.LAMB(flat, lr=0.05, weight_decay=wd, exclude_1d=exclude_1d)
    _drive(net, opt, steps, coefs)
    ref, trust = _ref_lamb(init, steps, coefs, 0.05, 0.9, 0.999, 1e-6, wd, exclude_1d)
    names = [n for n, _ in net.named_parameters()]
    for n, p, r, p0 in zip(names, net.parameters(), ref, init):
        assert torch.allclose(p, r.float(), **TOL), n
        assert not torch.allclose(p, p0, atol=1e-4) or (wd == 0 and n == "still"), n
    got = {sl.name: float(opt.trust[i]) for i, sl in enumerate(flat.slots)}
    for n, q in zip(names, trust):
        assert got[n] == pytest.approx(q, rel=1e-5), n
    assert (got["lin.bias"] == 1.0) == exclude_1d
    assert got["still"] == 1.0 if wd == 0 else got["still"] != 1.0  # u = wd p: |p| / |u| = 1 / wd


@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_without_trust_ratio_is_flat_sgd_bitwise(nesterov):
    """eta <= 0: no slot is adapted and every slot keeps the decay -- the SGD rule, bit for bit."""
    a, b = _Net(), _Net()
    fa, fb = FlatParams(a), FlatParams(b)
    oa = O.LARS(fa, lr=0.1, momentum=0.9, nesterov=nesterov, weight_decay=5e-4, eta=0.0)
    ob = O.SGD(fb, lr=0.1, momentum=0.9, nesterov=nesterov, weight_decay=5e-4)
    steps = [_grads(a.named_parameters(), s, zero=()) for s in range(5)]
    coefs = [0.37, None, 0.9, None, None]
    _drive(a, oa, steps, coefs)
    _drive(b, ob, steps, coefs)
    assert torch.equal(fa.data, fb.data)
    assert torch.equal(oa.state["__flat__"]["momentum_buffer"], ob.state["__flat__"]["momentum_buffer"])
    assert torch.equal(oa.trust, torch.ones_like(oa.trust)) and oa.trust_summary() is None


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_state_dict_round_trip_continues_bitwise(kind):
    def make(net):
        flat = FlatParams(net)
        if kind == "lars":
            return flat, O.LARS(flat, lr=0.5, momentum=0.9, weight_decay=5e-4, eta=0.05)
        return flat, O.LAMB(flat, lr=0.05, weight_decay=0.01)
    a, b = _Net(), _Net()
    steps = [_grads(a.named_parameters(), s) for s in range(6)]
    fa, oa = make(a)
    _drive(a, oa, steps[:3], [None] * 3)
    sd = oa.state_dict()
    assert set(k for k, v in sd["flat_state"].items() if torch.is_tensor(v)) == (
        {"momentum_buffer"} if kind == "lars" else {"exp_avg", "exp_avg_sq"})  # trust ratios are not state
    fb, ob = make(b)
    with torch.no_grad():
        fb.data.copy_(fa.data)
    ob.load_state_dict(sd)
    _drive(a, oa, steps[3:], [None] * 3)
    _drive(b, ob, steps[3:], [None] * 3)
    assert torch.equal(fa.data, fb.data) and torch.equal(oa.trust, ob.trust)
    for k, v in oa.state["__flat__"].items():
        if torch.is_tensor(v):
            assert torch.equal(v, ob.state["__flat__"][k]), k


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_skipped_step_cpu(kind):
    def run(skip_at):
        net = _Net()
        flat = FlatParams(net)
        opt = (O.LARS(flat, lr=0.5, momentum=0.9, weight_decay=5e-4, eta=0.05) if kind == "lars"
               else O.LAMB(flat, lr=0.05, weight_decay=0.01))
        good = [_grads(net.named_parameters(), s) for s in range(3)]
        params = list(net.parameters())
        i = 0
        for k in range(3 + (skip_at is not None)):
            if k == skip_at:
                before = flat.data.clone()
                state = {n: v.clone() for n, v in opt.state.get("__flat__", {}).items() if torch.is_tensor(v)}
                flat.grad.fill_(float("inf"))
                opt.step(found_inf=torch.ones(1, dtype=torch.int32))
                assert torch.equal(flat.data, before) and not flat.grad.any()
                for n, v in state.items():
                    assert torch.equal(opt.state["__flat__"][n], v), n
                assert opt.applied_k == k  # the count advanced on applied steps only
                continue
            for p, g in zip(params, good[i]):
                p.grad.copy_(g)
            opt.step(found_inf=torch.zeros(1, dtype=torch.int32))
            assert not flat.grad.any()
            i += 1
        assert opt.applied_k == 3
        return flat.data.clone()
    clean = run(None)
    assert torch.equal(run(1), clean)  # LAMB: the bias correction of the steps after the skip did not move
    assert torch.equal(run(0), clean)  # (the first step skipped: the momentum buffer still starts at d)


def test_tile_table_covers_slots_exactly():
    T = O.LAYER_TILE
    sizes = [1, 3, 64, 65, T - 1, T, T + 1, 3 * T + 5]
    params = nn.ParameterList([nn.Parameter(torch.zeros(1, n)) for n in sizes] + [nn.Parameter(torch.zeros(70))])
    for part in (0, 2):
        flat = FlatParams(params, partition=part)
        tiles, slots = O.build_tile_table(flat)
        seen = torch.zeros(flat.numel, dtype=torch.int32)
        for si, first, n, t0 in tiles.tolist():
            assert 0 < n <= T and first % 4 == 0 and t0 == slots[si, 0]
            seen[first:first + n] += 1
        want = torch.zeros_like(seen)
        for si, sl in enumerate(flat.slots):
            want[sl.offset:sl.offset + sl.numel] = 1
            t0, nt, adapted, decayed = slots[si].tolist()
            assert nt == -(-sl.numel // T) and adapted == decayed == int(len(sl.shape) > 1)
            assert int(tiles[t0:t0 + nt, 2].sum()) == sl.numel and bool((tiles[t0:t0 + nt, 0] == si).all())
        assert torch.equal(seen, want)  # every slot element once, no padding element
    _, slots = O.build_tile_table(flat, exclude_1d=False)
    assert bool(slots[:, 2:].all())
    _, slots = O.build_tile_table(flat, adapt=False)
    assert not slots[:, 2].any() and bool(slots[:, 3].all())


def test_fsdp_is_refused_at_parse_time_and_in_the_trainers():
    """The CLIs that carry the new switches wrap the reference-compatible ones: resnet_infer.py and
    transformer_train.py."""
    import resnet_infer
    import transformer_train
    from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig, ResNetTrainer
    from faster_distributed_training_amd.train.transformer_trainer import TransformerConfig, TransformerTrainer
    for cli in (resnet_infer, transformer_train):
        for kind in ("lars", "lamb"):
            with pytest.raises(ValueError, match="whole parameter slots"):
                cli.parse(["--optimizer", kind, "--fsdp", "--synthetic"])
            cfg = cli.config_from_args(*cli.parse(["--optimizer", kind, "--synthetic", "--trust_coef", "0.02"]))
            assert cfg.trust_coef == 0.02 and cfg.optimizer == kind and cfg.synthetic
        cfg = cli.config_from_args(*cli.parse(["--synthetic"]))
        assert cfg.trust_coef == 1e-3 and cfg.optimizer == "auto"
        # every other value is the wrapped CLI's: passed on, and checked there
        cfg = cli.config_from_args(*cli.parse(["--synthetic", "--optimizer", "sgd", "--fsdp"]))
        assert cfg.optimizer == "sgd" and cfg.fsdp
        with pytest.raises(SystemExit):
            cli.parse(["--optimizer", "lion"])
    with pytest.raises(ValueError, match="whole parameter slots"):
        ResNetTrainer(ResNetConfig(optimizer="lars", fsdp=True, synthetic=True))
    with pytest.raises(ValueError, match="whole parameter slots"):
        TransformerTrainer(TransformerConfig(optimizer="lamb", fsdp=True, synthetic=True))
    O.check_layerwise_config("sgd", True)
    O.check_layerwise_config("lars", False)


def test_launcher_reaches_lamb_on_the_transformer_two_ranks(tmp_path):
    """run_distributed.sh starts the transformer through transformer_train.py: two gloo ranks on the CPU
    train with --optimizer lamb (plain data parallel: every rank steps on the all-reduced gradients)."""
    import os
    import socket
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, FDT_NATIVE="0", NGPU="2", MASTER_PORT=str(port), OMP_NUM_THREADS="2", PYTHONPATH=root)
    r = subprocess.run(["bash", os.path.join(root, "run_distributed.sh"), "transformer", "--batch_size", "4", "--layers", "1",
                        "--d_model", "64", "--synthetic", "--epoch", "1", "--steps", "2", "--no_plot", "--no_eval",
                        "--checkpoint_dir", str(tmp_path / "ck"), "--optimizer", "lamb"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DDP bucket reducer, world 2" in r.stdout and "epoch 0:" in r.stdout
    # (the wrapped CLI alone refuses the value: only the wrapper can have built this optimizer)
    import transformer_test
    with pytest.raises(SystemExit):
        transformer_test.parse(["--optimizer", "lamb"])


RESNET_KEYS = {"epoch", "steps", "epoch_time_s", "img_per_s", "train_loss", "train_acc", "peak_mem_gb", "lr",
               "skipped_steps", "time"}  # ("time": the logger's stamp)
TRUST_KEYS = {"trust_min", "trust_med", "trust_max"}


def _last_record(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()][-1]


def test_resnet_trainer_cpu_logs_trust_fields(tmp_path, monkeypatch):
    from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig, ResNetTrainer
    monkeypatch.setenv("FDT_NATIVE", "0")

    def run(kind):
        log = tmp_path / f"{kind}.jsonl"
        cfg = ResNetConfig(arch="resnet18", bs=8, epoch=1, synthetic=True, eval=False, plot=False, steps_per_epoch=2,
                           checkpoint_dir=str(tmp_path), optimizer=kind, seed=7, extra={"subset_stride": 50},
                           log_path=str(log), trust_coef=0.02)
        t = ResNetTrainer(cfg)
        rec = t.train_epoch(0)
        assert rec["steps"] == 2 and math.isfinite(rec["train_loss"])
        return t, _last_record(log)
    t, rec = run("lars")
    assert isinstance(t.optimizer, O.LARS) and t.optimizer.group["eta"] == 0.02
    assert t.optimizer.group["weight_decay"] == 5e-4 and t.optimizer.group["momentum"] == t.cfg.momentum
    assert set(rec) == RESNET_KEYS | TRUST_KEYS
    assert 0 < rec["trust_min"] <= rec["trust_med"] <= rec["trust_max"] and math.isfinite(rec["trust_max"])
    t, rec = run("lamb")
    assert isinstance(t.optimizer, O.LAMB) and set(rec) == RESNET_KEYS | TRUST_KEYS
    t, rec = run("sgd")
    assert type(t.optimizer) is O.SGD and set(rec) == RESNET_KEYS  # exactly the record it always wrote


def test_transformer_trainer_cpu_logs_trust_fields(tmp_path, monkeypatch):
    from faster_distributed_training_amd.train.transformer_trainer import TransformerConfig, TransformerTrainer
    monkeypatch.setenv("FDT_NATIVE", "0")

    def run(kind):
        log = tmp_path / f"{kind}.jsonl"
        cfg = TransformerConfig(batch_size=8, epoch=1, synthetic=True, eval=False, plot=False, steps_per_epoch=2,
                                n_layers=1, d_model=64, heads=4, d_ff=128, d_hidden=128, length_buckets=(32,),
                                checkpoint_dir=str(tmp_path), optimizer=kind, seed=3, log_path=str(log))
        t = TransformerTrainer(cfg)
        rec = t.train_epoch(0)
        assert rec["steps"] == 2 and math.isfinite(rec["train_loss"])
        return t, _last_record(log)
    t, rec = run("lamb")
    assert isinstance(t.optimizer, O.LAMB) and t.optimizer.group["weight_decay"] == 0.01
    assert TRUST_KEYS <= set(rec) and 0 < rec["trust_min"] <= rec["trust_med"] <= rec["trust_max"]
    base = set(rec) - TRUST_KEYS
    t, rec = run("lars")
    assert isinstance(t.optimizer, O.LARS) and set(rec) == base | TRUST_KEYS
    t, rec = run("sgd")
    assert type(t.optimizer) is O.SGD and set(rec) == base


# ------------------------------------------------------------------------------ GPU
T = O.LAYER_TILE
# (name, shape): sizes where the tile logic can break; 2-D = adapted, 1-D = excluded.  "z20" gets
# an all-zero gradient; "b100" is an excluded slot between two adapted ones; "big" spans 41 tiles.
GPU_SLOTS = [("a1", (1, 1)), ("a3", (1, 3)), ("a4", (2, 2)), ("a63", (7, 9)), ("a64", (8, 8)), ("a65", (5, 13)),
             ("tm1", (1, T - 1)), ("b100", (100,)), ("t0", (64, T // 64)), ("tp1", (1, T + 1)), ("b65", (65,)),
             ("t3", (1, 3 * T + 5)), ("z20", (4, 5)), ("big", (1, 40 * T + 7))]
NAMES = [n for n, _ in GPU_SLOTS]


def _gpu_model(device, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [nn.Parameter((0.1 * torch.randn(shape, generator=g) + 0.02).to(device)) for _, shape in GPU_SLOTS]


def _gpu_grads(step):
    g = torch.Generator().manual_seed(500 + step)
    return [torch.zeros(shape) if n == "z20" else 0.3 * torch.randn(shape, generator=g) for n, shape in GPU_SLOTS]


def _make(kind, device, partition=0, shadow=True, reverse=True, **kw):
    params = _gpu_model(device)
    flat = FlatParams(params, device=device, names=NAMES, with_shadow=shadow and device.type == "cuda",
                      partition=partition, reverse=reverse)
    if kind == "lamb":
        opt = O.LAMB(flat, **dict(dict(lr=0.05, weight_decay=0.01), **kw))
    elif kind == "sgd":
        opt = O.SGD(flat, **dict(dict(lr=0.5, momentum=0.9, weight_decay=5e-4), **kw))
    else:
        opt = O.LARS(flat, **dict(dict(lr=0.5, momentum=0.9, weight_decay=5e-4, eta=0.05,
                                       nesterov=kind == "lars_nesterov"), **kw))
    return params, flat, opt


def _step(params, opt, grads, coef=None, found_inf=None):
    dev = opt.flat.device
    for p, g in zip(params, grads):
        p.grad.copy_(g)
    opt.step(grad_scale=None if coef is None else torch.tensor([coef], dtype=torch.float32, device=dev),
             found_inf=None if found_inf is None else torch.full((1,), found_inf, dtype=torch.int32, device=dev))


def _state(opt):
    return {k: v for k, v in opt.state["__flat__"].items() if torch.is_tensor(v)}


def _pad_mask(flat):
    m = torch.ones(flat.numel, dtype=torch.bool)
    for sl in flat.slots:
        m[sl.offset:sl.offset + sl.numel] = False
    return m.to(flat.device)


KINDS = ["lars", "lars_nesterov", "lamb"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_trust_ratios_match_fp64(cuda, kind):
    """opt.trust after one step against the fp64 per-slot value, rtol 1e-5.  A tile partial is a
    fixed tree over at most LAYER_TILE = 4096 non-negative fp32 terms (16 per lane in sequence,
    6 butterfly levels, 4 waves), combined in fp64: relative error about (log2 4096 + 2) 2^-24
    ~ 1e-6 before the square root, so 1e-5 is a tenfold margin."""
    params, flat, opt = _make(kind, cuda)
    assert flat.numel > 150_000 and opt.ntiles > 41 and O.LAYER_TILE == 4096
    p0 = [p.detach().cpu() for p in params]
    grads = _gpu_grads(0)
    _step(params, opt, grads, coef=0.5)
    if kind == "lamb":
        _, want = _ref_lamb(p0, [grads], [0.5], 0.05, 0.9, 0.999, 1e-6, 0.01, True)
    else:
        want = []
        for p, g in zip(p0, grads):
            wn, gn = p.double().norm().item(), 0.5 * g.double().norm().item()
            want.append(0.05 * wn / (gn + 5e-4 * wn + 1e-8) if (p.ndim > 1 and gn > 0) else 1.0)
    got = dict(zip([sl.name for sl in flat.slots], opt.trust.cpu().tolist()))
    worst = 0.0
    for n, w in zip(NAMES, want):
        worst = max(worst, abs(got[n] - w) / w)
        assert got[n] == pytest.approx(w, rel=1e-5), n
    print(f"{kind}: worst relative trust-ratio error {worst:.2e}")
    assert got["b100"] == 1.0 and got["b65"] == 1.0
    if kind == "lars":
        assert got["z20"] == 1.0
    norms = dict(zip([sl.name for sl in flat.slots], opt.norms.cpu().tolist()))
    for n, p in zip(NAMES, p0):
        assert norms[n][0] == pytest.approx(p.double().norm().item(), rel=1e-5), n
    s = opt.trust_summary()
    adapted = [got[n] for n, sh in GPU_SLOTS if len(sh) > 1]
    assert s["min"] == min(adapted) and s["max"] == max(adapted)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_padding_is_not_read_as_data(cuda, kind):
    def run(poison):
        params, flat, opt = _make(kind, cuda)
        pad = _pad_mask(flat)
        assert int(pad.sum()) > 0
        bufs = [opt._state_buf(n) for n in (("exp_avg", "exp_avg_sq") if kind == "lamb" else ("momentum_buffer",))]
        if poison:
            flat.data[pad] = 1e30
            flat.grad[pad] = 1e30
            flat.shadow[pad] = 3.0
            for i, b in enumerate(bufs):
                b[pad] = 7.0 + i
        trust = []
        for s in range(2):  # (the second step reads the momentum buffer)
            _step(params, opt, _gpu_grads(s))
            trust.append(opt.trust.clone())
        return flat, opt, pad, bufs, trust
    fa, oa, pad, _, ta = run(False)
    fb, ob, _, bufs, tb = run(True)
    assert all(torch.equal(x, y) for x, y in zip(ta, tb))
    assert torch.equal(fa.data[~pad], fb.data[~pad]) and torch.equal(fa.shadow[~pad], fb.shadow[~pad])
    for k, v in _state(oa).items():
        assert torch.equal(v[~pad], _state(ob)[k][~pad]), k
    assert torch.isfinite(fb.data[~pad]).all() and not fb.grad[~pad].any()
    assert bool((fb.data[pad] == 1e30).all()) and bool((fb.shadow[pad] == 3.0).all())
    for i, b in enumerate(bufs):
        assert bool((b[pad] == 7.0 + i).all())
    assert not fa.data[pad].any() and not fa.shadow[pad].any()  # clean run: padding still zero


@pytest.fixture(scope="module")
def cpu_runs():
    """Five CPU-path steps of every kind (clip coefficient on step 1 only), computed once."""
    out = {}
    for kind in KINDS:
        params, flat, opt = _make(kind, torch.device("cpu"))
        for s in range(5):
            _step(params, opt, _gpu_grads(s), coef=0.5 if s == 1 else None)
        out[kind] = (flat.data.clone(), {k: v.clone() for k, v in _state(opt).items()}, opt.trust.clone())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_matches_cpu_path(cuda, cpu_runs, kind):
    params, flat, opt = _make(kind, cuda)
    for s in range(5):
        _step(params, opt, _gpu_grads(s), coef=0.5 if s == 1 else None)
        assert not flat.grad.any()
        assert torch.equal(flat.shadow, flat.data.to(torch.bfloat16))
    data, state, trust = cpu_runs[kind]
    assert torch.allclose(flat.data.cpu(), data, **TOL)
    for k, v in state.items():
        assert torch.allclose(_state(opt)[k].cpu(), v, **TOL), k
    assert torch.allclose(opt.trust.cpu(), trust, rtol=1e-5, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_two_fresh_runs_are_bitwise_equal(cuda, kind):
    def run():
        params, flat, opt = _make(kind, cuda)
        for s in range(3):
            _step(params, opt, _gpu_grads(s), coef=0.7)
        return flat.data.clone(), {k: v.clone() for k, v in _state(opt).items()}, opt.trust.clone()
    a, b = run(), run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert all(torch.equal(v, b[1][k]) for k, v in a[1].items())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_skipped_step_gpu(cuda, kind):
    params, flat, opt = _make(kind, cuda)
    _step(params, opt, _gpu_grads(0), found_inf=0)
    before = (flat.data.clone(), flat.shadow.clone(), {k: v.clone() for k, v in _state(opt).items()})
    bad = _gpu_grads(1)
    bad[-1][0, 5] = float("inf")
    bad[3][0, 0] = float("nan")
    _step(params, opt, bad, found_inf=1)
    assert torch.equal(flat.data, before[0]) and torch.equal(flat.shadow, before[1])
    for k, v in before[2].items():
        assert torch.equal(_state(opt)[k], v), k
    assert not flat.grad.any()
    assert int(opt.kskip.item()) == (1 if kind == "lamb" else 0)
    _step(params, opt, _gpu_grads(2), found_inf=0)
    # a run that never saw the bad gradient
    params2, flat2, opt2 = _make(kind, cuda)
    _step(params2, opt2, _gpu_grads(0), found_inf=0)
    _step(params2, opt2, _gpu_grads(2), found_inf=0)
    assert torch.equal(flat.data, flat2.data) and torch.equal(opt.trust, opt2.trust)
    for k, v in _state(opt2).items():
        assert torch.equal(_state(opt)[k], v), k
    assert int(opt2.kskip.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_partitioned_layout_gives_the_same_parameters(cuda, kind):
    pa, fa, oa = _make(kind, cuda)
    # (registration order: the small slots fill run 0, a gap follows, "big" is run 1)
    pb, fb, ob = _make(kind, cuda, partition=2, reverse=False)
    assert fb.runs is not None and fb.numel > fa.numel and [s.offset for s in fa.slots] != [s.offset for s in fb.slots]
    for s in range(3):
        _step(pa, oa, _gpu_grads(s))
        _step(pb, ob, _gpu_grads(s))
    by_name = {sl.name: (j, sl) for j, sl in enumerate(fb.slots)}
    ta, tb = oa.trust.cpu(), ob.trust.cpu()
    for i, sl in enumerate(fa.slots):
        j, other = by_name[sl.name]
        assert torch.equal(fa.data[sl.offset:sl.offset + sl.numel], fb.data[other.offset:other.offset + sl.numel]), sl.name
        assert ta[i] == tb[j], sl.name


@pytest.mark.gpu
@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_without_trust_ratio_is_flat_sgd_bitwise_gpu(cuda, nesterov):
    """eta <= 0 on the GPU: lars_apply with q = 1 on every slot against sgd_kernel, bit for bit --
    parameters, momentum buffer and bf16 shadow (the trust ratios are still computed, and unused)."""
    pa, fa, oa = _make("lars", cuda, eta=0.0, nesterov=nesterov)
    pb, fb, ob = _make("sgd", cuda, nesterov=nesterov)
    for s in range(4):
        _step(pa, oa, _gpu_grads(s), coef=0.37 if s == 1 else None)
        _step(pb, ob, _gpu_grads(s), coef=0.37 if s == 1 else None)
        assert torch.equal(fa.data, fb.data) and torch.equal(fa.shadow, fb.shadow), s
        assert torch.equal(_state(oa)["momentum_buffer"], _state(ob)["momentum_buffer"]), s
    assert torch.equal(oa.trust, torch.ones_like(oa.trust)) and oa.trust_summary() is None
    assert not torch.equal(fa.data, _make("sgd", cuda)[1].data)  # it moved


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_exclude_1d_false_gpu_matches_cpu(cuda, kind):
    """exclude_1d=False: the 1-D slots get a trust ratio and the decay like every other."""
    runs = {}
    for dev in (torch.device("cpu"), cuda):
        params, flat, opt = _make(kind, dev, exclude_1d=False)
        for s in range(3):
            _step(params, opt, _gpu_grads(s), coef=0.5 if s == 1 else None)
        runs[dev.type] = (flat.data.cpu(), opt.trust.cpu(), {k: v.cpu() for k, v in _state(opt).items()})
        names = [sl.name for sl in flat.slots]
    (dc, tc, sc), (dg, tg, sg) = runs["cpu"], runs["cuda"]
    assert torch.allclose(dg, dc, **TOL) and torch.allclose(tg, tc, rtol=1e-5, atol=0)
    for k, v in sc.items():
        assert torch.allclose(sg[k], v, **TOL), k
    got = dict(zip(names, tg.tolist()))
    assert got["b100"] != 1.0 and got["b65"] != 1.0
    assert bool(opt.slot_rows[:, 2:].all())  # every slot adapted and decayed


def _flat_reference(kind, p, grads, seg, nseg, steps):
    """fp64, vectorised over segments (every slot adapted): LARS(lr .5, momentum .9, wd 5e-4, eta .05)
    or LAMB(lr .05, wd .01), as _ref_lars / _ref_lamb."""
    p = p.double()
    buf = m = v = None
    qs = []

    def norms(x):
        return torch.zeros(nseg, dtype=torch.float64).index_add_(0, seg, x * x).sqrt()
    for t in range(1, steps + 1):
        g = grads(t - 1).double()
        if kind == "lars":
            wn, gn = norms(p), norms(g)
            q = torch.where((wn > 0) & (gn > 0), 0.05 * wn / (gn + 5e-4 * wn + 1e-8), torch.ones_like(wn))
            d = q[seg] * (g + 5e-4 * p)
            buf = d if buf is None else 0.9 * buf + d
            p = p - 0.5 * buf
        else:
            m = 0.1 * g if m is None else 0.9 * m + 0.1 * g
            v = 0.001 * g * g if v is None else 0.999 * v + 0.001 * g * g
            u = (m / (1 - 0.9 ** t)) / ((v / (1 - 0.999 ** t)).sqrt() + 1e-6) + 0.01 * p
            wn, un = norms(p), norms(u)
            q = torch.where((wn > 0) & (un > 0), wn / un, torch.ones_like(wn))
            p = p - 0.05 * q[seg] * u
        qs.append(q)
    return p, qs


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_more_tiles_than_workgroups(cuda, kind):
    """The grid is capped at 16384 workgroups; more tiles than that are walked grid-stride.  16421
    one-element slots (a tile each) and one slot of two tiles, two steps, against fp64."""
    n1 = 16384 + 37
    g0 = torch.Generator().manual_seed(77)
    params = [nn.Parameter(v.reshape(1, 1)) for v in (0.1 * torch.randn(n1, generator=g0) + 0.5).unbind()]
    params.append(nn.Parameter(0.1 * torch.randn(1, T + 3, generator=g0)))
    flat = FlatParams(params, device=cuda, with_shadow=True)
    opt = (O.LAMB(flat, lr=0.05, weight_decay=0.01) if kind == "lamb"
           else O.LARS(flat, lr=0.5, momentum=0.9, weight_decay=5e-4, eta=0.05))
    assert opt.ntiles == n1 + 2 and opt.ntiles > 16384
    idx = torch.cat([torch.arange(sl.offset, sl.offset + sl.numel) for sl in flat.slots])
    seg = torch.cat([torch.full((sl.numel,), i) for i, sl in enumerate(flat.slots)])
    p0 = flat.data.cpu()[idx]

    def grads(step):
        return 0.3 * torch.randn(idx.numel(), generator=torch.Generator().manual_seed(900 + step))
    trust = []
    for s in range(2):
        flat.grad[idx.to(cuda)] = grads(s).to(cuda)
        opt.step()
        assert not flat.grad.any()
        trust.append(opt.trust.cpu().double())
    want, qs = _flat_reference(kind, p0, grads, seg, len(flat.slots), 2)
    got = flat.data.cpu()[idx]
    assert torch.allclose(got, want.float(), **TOL)
    # The 1e-5 bound on a trust ratio covers the REDUCTION (test_trust_ratios_match_fp64), so it is
    # asked where the summed terms carry no more than fp32 rounding: LARS's p and g in both steps,
    # LAMB's u in the first step (m^ = g', v^ = g'^2: u = +-1 + wd p).  In LAMB's second step a
    # one-element u = m^ / sqrt(v^) + wd p can cancel to almost nothing, its fp32 rounding is then
    # unbounded relative to |u| = the whole norm, and what is asked is the parameters (above).
    assert torch.allclose(trust[0], qs[0], rtol=1e-5, atol=0)
    if kind == "lars":
        assert torch.allclose(trust[1], qs[1], rtol=1e-5, atol=0)
    assert torch.equal(flat.shadow, flat.data.to(torch.bfloat16)) and not torch.allclose(got, p0, atol=1e-3)


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.gpu
def test_engine_trains_with_lars_and_sees_the_new_weights(cuda, tmp_path):
    """ResNet-18, batch 32, synthetic data, graphs on, 3 LARS steps through the trainer.  After each
    step the engine's eval logits (packed conv weights: the LARS step invalidates the pack, the
    engine repacks) against the PyTorch forward of a copy holding the same weights, within the
    bound tests/test_resnet_engine.py::test_engine_eval_matches_reference uses."""
    from faster_distributed_training_amd.models import resnet as R
    from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig, ResNetTrainer
    # (lr and eta far above a training recipe: every step moves the weights by several percent, so
    # a forward that still used the previous step's packed weights would miss the bound)
    cfg = ResNetConfig(arch="resnet18", bs=32, epoch=1, synthetic=True, eval=False, plot=False, steps_per_epoch=3,
                       checkpoint_dir=str(tmp_path), optimizer="lars", lr=0.2, trust_coef=0.25, graphs=True, seed=5,
                       extra={"subset_stride": 50})
    tr = ResNetTrainer(cfg)
    assert isinstance(tr.optimizer, O.LARS) and tr.model.use_fast_path(torch.empty(1, device=cuda))
    ref = R.resnet18(10).to(cuda)
    ref.fast_path = False
    torch.manual_seed(11)
    xe = torch.randn(32, 3, 32, 32, device=cuda)
    it = iter(tr.train_loader)
    w0 = tr.flat.data.clone()
    prev = None
    for _ in range(3):
        tr.model.train()
        x, y = next(it)
        loss = tr.train_step(x, y)
        assert torch.isfinite(loss).item()
        ref.load_state_dict(tr.model.state_dict())
        tr.model.eval()
        ref.eval()
        with torch.no_grad():
            out_r = ref(xe)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out_rb = ref(xe)
                out_e = tr.model(xe)
        e_eng, e_ref = _rel(out_e, out_r), _rel(out_rb, out_r)
        print(f"engine vs fp32 {e_eng:.3e}, bf16 autocast vs fp32 {e_ref:.3e}"
              + ("" if prev is None else f", previous weights vs these {_rel(prev, out_r):.3e}"))
        assert e_eng < max(2.0 * e_ref, 3e-2), (e_eng, e_ref)
        # the bound tells new weights from stale ones: the previous step's logits are far outside it
        # (measured 0.55-0.77)
        assert prev is None or _rel(prev, out_r) > 0.1
        prev = out_r
    assert torch.isfinite(tr.flat.data).all() and not torch.equal(tr.flat.data, w0)
    assert _rel(tr.flat.data, w0) > 1e-2
    s = tr.optimizer.trust_summary()
    assert 0 < s["min"] <= s["med"] <= s["max"]

"""Weight EMA over the flat buffers (optim/ema.py, csrc/kernels/ema.hip).

CPU: the torch-op path against an fp64 oracle written here, skipped updates, the in-place swap,
state_dict round trips (also across slot orders), auto-resume, the best checkpoint's ``ema`` entry
with ``--eval_ema``, the refusals and the transformer CLI.  GPU: the two kernels at sizes placed
around one workgroup's and one full grid's trip, skipped launches, the kernel path against the CPU
path, the ResNet engine (packed conv layouts) and the transformer (bf16 shadow) under
``applied()``, and the ResNet trainer end to end with a skipped step.

Error bound of N updates, per element (``_bound``): N * 8 * 2^-24 * max(|p|, |e|) over the run --
one rounding of e - p (|e - p| <= 2 max: 2 units of 2^-24 max), one of the fma (1 unit), two ulp of
slack for d (4 units), rounded up to 8."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn as nn

from faster_distributed_training_amd.ops import _native
from faster_distributed_training_amd.optim import ema as E
from faster_distributed_training_amd.utils.flat import FlatParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _reset_deterministic():
    yield
    _native.set_deterministic(False)  # (trainers built with deterministic=True switch it on for the process)


class _Net(nn.Module):
    """The small module of tests/test_layerwise_optim.py: a 2-D weight, a 1-D bias, a 4-D weight, a 2-D one."""

    def __init__(self, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.lin = nn.Linear(6, 5)
        self.conv = nn.Conv2d(2, 3, 3, bias=False)
        self.still = nn.Parameter(torch.randn(4, 3))


# ------------------------------------------------------------------------------ fp64 oracle
def _d(decay, warmup, t):
    """The stated schedule, rounded to fp32."""
    d = float(torch.tensor(decay, dtype=torch.float32))
    if warmup:
        d = min(d, float(torch.tensor((1.0 + t) / (10.0 + t), dtype=torch.float64).float()))
    return d


class _Oracle:
    def __init__(self, e, decay, warmup):
        self.e = e.detach().double().cpu().clone()
        self.decay, self.warmup, self.t = decay, warmup, 0
        self.n = 0
        self.mx = self.e.abs()

    def update(self, p):
        p = p.detach().double().cpu()
        d = _d(self.decay, self.warmup, self.t)
        self.mx = torch.maximum(self.mx, torch.maximum(p.abs(), self.e.abs()))
        self.e = p + d * (self.e - p)
        self.mx = torch.maximum(self.mx, self.e.abs())
        self.t += 1
        self.n += 1
        return d

    def bound(self, scale=1.0):
        return scale * self.n * 8 * 2.0 ** -24 * self.mx

    def check(self, e, scale=1.0):
        err = (e.detach().double().cpu() - self.e).abs()
        bound = self.bound(scale)
        worst = float((err - bound).max())
        print(f"ema oracle: n={self.n} max err {float(err.max()):.3e} max bound {float(bound.max()):.3e}")
        assert bool((err <= bound).all()), f"error exceeds the bound by {worst:.3e}"


def _walk(flat, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        flat.data.add_(0.1 * torch.randn(flat.numel, generator=g).to(flat.device))


# ------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("decay", [0.0, 0.5, 0.999])
def test_rule_matches_fp64_oracle(decay, warmup):
    flat = FlatParams(_Net())
    ema = E.FlatEMA(flat, decay, warmup)
    assert torch.equal(ema.e, flat.data) and ema.e.data_ptr() != flat.data.data_ptr() and ema.e.dtype == torch.float32
    ref = _Oracle(ema.e, decay, warmup)
    for s in range(8):
        _walk(flat, s)
        ema.update()
        d = ref.update(flat.data)
        assert E.ema_decay_at(decay, warmup, s) == d
        ref.check(ema.e)
        if decay == 0.0:
            assert torch.equal(ema.e, flat.data)  # bitwise
    assert ema.k == 8 and int(ema.kskip) == 0 and ema.decay_eff() == _d(decay, warmup, 7)


def test_skipped_update_changes_nothing_and_the_next_uses_the_applied_count():
    flat = FlatParams(_Net())
    ema = E.FlatEMA(flat, 0.999, warmup=True)
    ref = _Oracle(ema.e, 0.999, True)
    bad, ok = torch.ones(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    for s in range(3):
        _walk(flat, s)
        ema.update(found_inf=ok)
        ref.update(flat.data)
    _walk(flat, 3)
    before = ema.e.clone()
    ema.update(found_inf=bad)
    assert torch.equal(ema.e, before) and int(ema.kskip) == 1 and ema.k == 4 and ema.applied_k == 3
    _walk(flat, 4)
    p, e0 = flat.data.double(), ema.e.double()
    ema.update(found_inf=ok)
    d = ref.update(flat.data)  # (the oracle never saw the skipped call: t = 3)
    assert d == _d(0.999, True, 3) < 0.999
    ref.check(ema.e)
    # d as the update applied it: (1 + 3) / (10 + 3), not the (1 + 4) / (10 + 4) of the call count
    m = (e0 - p).abs() > 1e-3
    got = ((ema.e.double() - p)[m] / (e0 - p)[m]).median().item()
    assert abs(got - 4 / 13) < 1e-4 < abs(got - 5 / 14)
    assert ema.decay_eff() == d


class _StubPlan:
    def __init__(self):
        self.invalidated = 0

    def invalidate_pack(self):
        self.invalidated += 1


def test_swap_is_in_place_and_twice_the_identity():
    net = _Net()
    flat = FlatParams(net, with_shadow=True)
    plan = _StubPlan()
    flat.pack_owner = types.SimpleNamespace(_plan=plan)
    ema = E.FlatEMA(flat, 0.5, warmup=False)
    _walk(flat, 0)
    ema.update()
    flat.refresh_shadow()
    p0, e0, sh0 = flat.data.clone(), ema.e.clone(), flat.shadow.clone()
    ptrs = (flat.data.data_ptr(), ema.e.data_ptr(), flat.shadow.data_ptr())
    assert not torch.equal(p0, e0)
    seen = plan.invalidated
    ema.swap()
    assert plan.invalidated > seen and ema.swapped
    assert torch.equal(flat.data, e0) and torch.equal(ema.e, p0)
    assert torch.equal(flat.shadow, flat.data.bfloat16())
    for sl in flat.slots:  # the model's parameters are views: they now hold the former average
        assert torch.equal(sl.param.data.reshape(-1), e0[sl.offset:sl.offset + sl.numel])
    with pytest.raises(RuntimeError):
        ema.update()
    ema.swap()
    assert not ema.swapped
    assert torch.equal(flat.data, p0) and torch.equal(ema.e, e0) and torch.equal(flat.shadow, sh0)
    assert ptrs == (flat.data.data_ptr(), ema.e.data_ptr(), flat.shadow.data_ptr())
    with pytest.raises(KeyError):
        with ema.applied():
            assert torch.equal(flat.data, e0)
            raise KeyError("inside")
    assert torch.equal(flat.data, p0) and torch.equal(ema.e, e0) and not ema.swapped


def test_state_dict_round_trip_and_slot_remap():
    flat = FlatParams(_Net())
    ema = E.FlatEMA(flat, 0.9, warmup=True)
    for s in range(3):
        _walk(flat, s)
        ema.update(found_inf=torch.tensor([int(s == 1)], dtype=torch.int32))
    sd = ema.state_dict()
    assert {"e", "k", "kskip", "decay", "warmup", "slots"} <= set(sd)
    same = E.FlatEMA(FlatParams(_Net()), 0.5, warmup=False)
    same.load_state_dict(sd)
    assert torch.equal(same.e, ema.e) and same.k == 3 and int(same.kskip) == 1
    assert same.decay == 0.9 and same.warmup is True
    other_flat = FlatParams(_Net(), reverse=False)
    assert [s.name for s in other_flat.slots] != [s.name for s in flat.slots]
    other = E.FlatEMA(other_flat, 0.9)
    other.load_state_dict(sd)
    by_name = {s.name: s for s in flat.slots}
    for sl in other_flat.slots:
        src = by_name[sl.name]
        assert torch.equal(other.e[sl.offset:sl.offset + sl.numel], ema.e[src.offset:src.offset + src.numel])
    with pytest.raises(ValueError, match="slot table"):
        other.load_state_dict({k: v for k, v in sd.items() if k != "slots"})
    sd_bad = dict(sd, slots=[(n + "x", o, k) for n, o, k in sd["slots"]])
    with pytest.raises(ValueError):
        other.load_state_dict(sd_bad)


def test_model_state_dict_holds_the_average():
    net = _Net()
    flat = FlatParams(net)
    ema = E.FlatEMA(flat, 0.5, warmup=False)
    _walk(flat, 0)
    ema.update()
    p0 = flat.data.clone()
    msd = ema.model_state_dict(net)
    assert torch.equal(flat.data, p0) and set(msd) == set(net.state_dict())
    for sl in flat.slots:
        assert torch.equal(msd[sl.name].reshape(-1), ema.e[sl.offset:sl.offset + sl.numel])
        assert msd[sl.name].data_ptr() != sl.param.data_ptr()


# ------------------------------------------------------------------------------ trainers (torch-op path)
def _cfg(tmp_path, **kw):
    from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig
    base = dict(arch="resnet18", bs=8, epoch=1, synthetic=True, eval=False, plot=False, steps_per_epoch=4,
                checkpoint_dir=str(tmp_path), optimizer="sgd", lr=0.05, seed=7, extra={"subset_stride": 500})
    base.update(kw)
    return ResNetConfig(**base)


def test_auto_resume_reproduces_parameters_and_average(tmp_path):
    """As tests/test_resilience.py: a run interrupted after epoch 1 of 3 and resumed from *_last.pth ends
    where the uninterrupted one ends -- parameters and e, bit for bit."""
    from faster_distributed_training_amd.train.resnet_trainer import ResNetTrainer
    kw = dict(ema_decay=0.9, warmup_epochs=1.5, deterministic=True)  # (bitwise-repeatable on a GPU as well)
    a = ResNetTrainer(_cfg(tmp_path / "a", epoch=3, **kw)).fit()
    b1 = ResNetTrainer(_cfg(tmp_path / "b", epoch=1, save_last=True, **kw)).fit()
    ck = torch.load(b1.last_path, weights_only=True)
    assert ck["ema_state"]["k"] == 4 and "slots" in ck["ema_state"]
    b2 = ResNetTrainer(_cfg(tmp_path / "b", epoch=2, auto_resume=True, **kw))
    assert b2.start_epoch == 1 and b2.global_step == 4 and b2.ema.k == 4
    assert torch.equal(b2.ema.e, b1.ema.e)
    b2.fit()
    assert torch.equal(a.flat.data, b2.flat.data), (a.flat.data - b2.flat.data).abs().max()
    assert torch.equal(a.ema.e, b2.ema.e) and a.ema.k == b2.ema.k == 12
    assert not torch.equal(a.ema.e, a.flat.data)
    # a *_last.pth of a run without the average does not resume one with it
    ResNetTrainer(_cfg(tmp_path / "c", epoch=1, save_last=True, deterministic=True)).fit()
    with pytest.raises(RuntimeError, match="EMA state"):
        ResNetTrainer(_cfg(tmp_path / "c", epoch=1, auto_resume=True, **kw))


def _records(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def _infer(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)  # (the path the training run took: --deterministic on both sides)
    return subprocess.run([sys.executable, os.path.join(ROOT, "resnet_infer.py")] + args, cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=600)


def test_best_checkpoint_carries_the_average_and_eval_ema_scores_it(tmp_path):
    from faster_distributed_training_amd.train.resnet_trainer import ResNetTrainer
    log = tmp_path / "train.jsonl"
    tr = ResNetTrainer(_cfg(tmp_path, epoch=1, eval=True, ema_decay=0.9, deterministic=True, log_path=str(log)))
    before_eval = {}

    def spy(epoch, save=True, _orig=tr.test):  # the state the evaluation must leave behind
        before_eval.update(p=tr.flat.data.clone(), e=tr.ema.e.clone())
        return _orig(epoch, save)
    tr.test = spy
    tr.fit()
    assert torch.equal(tr.flat.data, before_eval["p"]) and torch.equal(tr.ema.e, before_eval["e"])
    ck = torch.load(tr.ckpt_path, weights_only=True)
    assert set(ck["ema"]) == {"net", "updates", "decay"} and ck["ema"]["updates"] == 4 and ck["ema"]["decay"] == 0.9
    trained = {k: v.detach().cpu() for k, v in tr.model.state_dict().items()}
    averaged = tr.ema.model_state_dict(tr.model)
    assert set(ck["net"]) == set(trained) == set(ck["ema"]["net"])
    assert all(torch.equal(ck["net"][k], trained[k]) for k in trained)
    assert all(torch.equal(ck["ema"]["net"][k], averaged[k]) for k in averaged)
    assert any(not torch.equal(ck["net"][k], ck["ema"]["net"][k]) for k in trained)
    recs = _records(log)
    logged = [r for r in recs if "test_acc" in r and r["epoch"] == ck["epoch"]][-1]["test_acc"]
    assert logged == ck["acc"]
    assert [r for r in recs if "train_loss" in r][-1]["ema_decay_eff"] == _d(0.9, True, 3)

    args = ["--arch", "resnet18", "--synthetic", "--bs", "8", "--subset_stride", "500", "--seed", "7", "--no_plot",
            "--deterministic", "--checkpoint_dir", str(tmp_path), "--resume", "--eval_only"]
    r = _infer(args + ["--eval_ema", "--log", str(tmp_path / "ema.jsonl")], tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert _records(tmp_path / "ema.jsonl")[-1]["test_acc"] == logged
    r = _infer(args + ["--log", str(tmp_path / "net.jsonl")], tmp_path)  # without the flag: 'net', as before
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # without an 'ema' entry: refused, non-zero exit
    del ck["ema"]
    torch.save(ck, tr.ckpt_path)
    r = _infer(args + ["--eval_ema"], tmp_path)
    assert r.returncode != 0 and "no averaged weights" in (r.stdout + r.stderr)
    # --eval_ema without --resume --eval_only: refused when the arguments are parsed
    r = _infer(["--synthetic", "--eval_ema"], tmp_path)
    assert r.returncode != 0 and "--resume --eval_only" in (r.stdout + r.stderr)


def test_calibration_under_the_average_does_not_leak_into_training(tmp_path):
    """--eval_stats running --calibrate_batches N with an EMA: the statistics are re-estimated for the averaged
    weights, go into the checkpoint's ``ema`` entry, and the ones training left are put back (and saved next to
    the trained ``net``)."""
    from faster_distributed_training_amd.models.resnet import running_stats_state
    from faster_distributed_training_amd.train.resnet_trainer import ResNetTrainer
    tr = ResNetTrainer(_cfg(tmp_path, epoch=1, eval=True, ema_decay=0.9, deterministic=True, eval_stats="running",
                            calibrate_batches=2))
    seen = {}

    def spy(epoch, save=True, _orig=tr.test):
        seen.update(stats=running_stats_state(tr.model), p=tr.flat.data.clone())
        return _orig(epoch, save)
    tr.test = spy
    tr.fit()
    after = running_stats_state(tr.model)
    assert seen["stats"] and set(after) == set(seen["stats"])
    assert all(torch.equal(after[k], seen["stats"][k]) for k in after)
    assert torch.equal(tr.flat.data, seen["p"])
    ck = torch.load(tr.ckpt_path, weights_only=True)
    assert set(ck["ema"]) == {"net", "updates", "decay", "fused_stats"}
    assert all(torch.equal(ck["fused_stats"][k], seen["stats"][k]) for k in after)
    assert any(not torch.equal(ck["ema"]["fused_stats"][k], seen["stats"][k]) for k in after if "running_mean" in k)


def test_refusals():
    import resnet_infer
    import transformer_train
    from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig, ResNetTrainer
    from faster_distributed_training_amd.train.transformer_trainer import TransformerConfig, TransformerTrainer
    E.check_ema_config(0.0, fsdp=True, sharded=True)  # off: nothing to refuse
    E.check_ema_config(0.999)
    with pytest.raises(ValueError, match="--fsdp"):
        E.check_ema_config(0.999, fsdp=True)
    with pytest.raises(ValueError, match="sharded NGD"):
        E.check_ema_config(0.999, sharded=True)
    with pytest.raises(ValueError):
        E.check_ema_config(1.0)
    with pytest.raises(ValueError, match="--fsdp"):
        ResNetTrainer(ResNetConfig(ema_decay=0.9, fsdp=True, synthetic=True))
    with pytest.raises(ValueError, match="--fsdp"):
        TransformerTrainer(TransformerConfig(ema_decay=0.9, fsdp=True, synthetic=True))
    with pytest.raises(ValueError, match="sharded NGD"):
        ResNetTrainer(ResNetConfig(arch="resnet18", ema_decay=0.9, ngd=True, force_sharded=True, synthetic=True,
                                   extra={"subset_stride": 500}))
    assert not torch.distributed.is_initialized()  # refused before any process group is set up
    with pytest.raises(ValueError, match="--fsdp"):
        transformer_train.parse(["--synthetic", "--ema_decay", "0.9", "--fsdp"])
    with pytest.raises(SystemExit):
        resnet_infer.parse(["--synthetic", "--ema_decay", "0.9", "--fsdp"])
    for cli in (resnet_infer, transformer_train):
        cfg = cli.config_from_args(*cli.parse(["--synthetic", "--ema_decay", "0.99", "--no_ema_warmup",
                                               "--warmup_epochs", "2.5", "--warmup_start_factor", "0.2"]))
        assert (cfg.ema_decay, cfg.ema_warmup, cfg.warmup_epochs, cfg.warmup_start_factor) == (0.99, False, 2.5, 0.2)
        cfg = cli.config_from_args(*cli.parse(["--synthetic"]))
        assert (cfg.ema_decay, cfg.ema_warmup, cfg.warmup_epochs, cfg.warmup_start_factor) == (0.0, True, 0.0, 0.1)


def test_transformer_cli_trains_with_ema_and_warmup(tmp_path):
    env = dict(os.environ, FDT_NATIVE="0", PYTHONPATH=ROOT, OMP_NUM_THREADS="4")
    log = tmp_path / "tr.jsonl"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "transformer_train.py"), "--synthetic", "--ema_decay", "0.99",
                        "--warmup_epochs", "0.5", "--batch_size", "4", "--layers", "1", "--d_model", "64", "--epoch", "1",
                        "--steps", "4", "--no_plot", "--no_eval", "--checkpoint_dir", str(tmp_path / "ck"),
                        "--log", str(log)], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = [x for x in _records(log) if "train_loss" in x][-1]
    assert rec["steps"] == 4 and rec["ema_decay_eff"] == _d(0.99, True, 3)
    assert rec["lr_last_step"] > 0 and "lr" in rec


# ------------------------------------------------------------------------------ GPU: kernels
def _sizes():
    b, u, g = _native.native().ema_launch_config()
    wg = 4 * b * u  # elements of one workgroup's trip
    return [4, wg - 4, wg, wg + 4, 4 * b * g + 4, 4 * b * u * g + 4]  # (the last: a second, partial trip)


PAD, SENTINEL = 64, -777.0


def _buffers(n, seed, dev, shadow=False):
    """p, e (and a bf16 shadow) of n elements, each with PAD sentinel elements allocated past n."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        t = torch.full((n + PAD,), SENTINEL, dtype=torch.float32)
        t[:n] = torch.randn(n, generator=g)
        out.append(t.to(dev))
    if shadow:
        out.append(torch.full((n + PAD,), SENTINEL, dtype=torch.bfloat16, device=dev))
    return out


def _pads_intact(n, *ts):
    return all(bool((t[n:] == SENTINEL).all()) for t in ts)


def _sp():
    return _native.stream_ptr()


@pytest.fixture(scope="module")
def sizes(cuda):
    return _sizes()


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(6))
def test_ema_update_kernel_matches_fp64_oracle(cuda, sizes, which):
    n = sizes[which]
    nat = _native.native()
    kskip = torch.zeros(1, dtype=torch.int32, device=cuda)
    for decay, warmup in ((0.999, 1), (0.5, 0)):
        p, e = _buffers(n, which, cuda)
        ref = _Oracle(e[:n], decay, bool(warmup))
        nat.ema_update(p.data_ptr(), e.data_ptr(), n, decay, warmup, 0, kskip.data_ptr(), 0, _sp())
        ref.update(p[:n])
        ref.check(e[:n])  # one update from a random e
        for k in range(1, 5):  # ... and a chain of 5, p moving
            p[:n] += 0.1
            nat.ema_update(p.data_ptr(), e.data_ptr(), n, decay, warmup, k, kskip.data_ptr(), 0, _sp())
            ref.update(p[:n])
        ref.check(e[:n])
        assert _pads_intact(n, p, e)
        # two runs are bitwise equal
        p2, e2 = _buffers(n, which, cuda)
        for k in range(5):
            if k:
                p2[:n] += 0.1
            nat.ema_update(p2.data_ptr(), e2.data_ptr(), n, decay, warmup, k, kskip.data_ptr(), 0, _sp())
        assert torch.equal(e, e2)
    # decay 0: a bitwise copy, p untouched
    p, e = _buffers(n, 100 + which, cuda)
    p0 = p.clone()
    nat.ema_update(p.data_ptr(), e.data_ptr(), n, 0.0, 0, 0, kskip.data_ptr(), 0, _sp())
    assert torch.equal(e[:n], p[:n]) and torch.equal(p, p0) and _pads_intact(n, p, e)
    assert int(kskip) == 0


@pytest.mark.gpu
def test_skipped_launch_leaves_e_and_counts_once(cuda, sizes):
    nat = _native.native()
    bad = torch.ones(1, dtype=torch.int32, device=cuda)
    ok = torch.zeros(1, dtype=torch.int32, device=cuda)
    kskip = torch.zeros(1, dtype=torch.int32, device=cuda)
    for i, n in enumerate(sizes):
        p, e = _buffers(n, i, cuda)
        e0 = e.clone()
        nat.ema_update(p.data_ptr(), e.data_ptr(), n, 0.9, 1, 3, kskip.data_ptr(), bad.data_ptr(), _sp())
        assert torch.equal(e, e0)
        assert int(kskip) == i + 1  # once per launch, whatever the grid
    # the next applied launch: t = k - kskip
    n = sizes[2]
    p, e = _buffers(n, 9, cuda)
    ref = _Oracle(e[:n], 0.999, True)
    ref.t = 10 - len(sizes)
    nat.ema_update(p.data_ptr(), e.data_ptr(), n, 0.999, 1, 10, kskip.data_ptr(), ok.data_ptr(), _sp())
    assert ref.update(p[:n]) < 0.999
    ref.check(e[:n])
    assert int(kskip) == len(sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(6))
def test_ema_swap_kernel(cuda, sizes, which):
    n = sizes[which]
    nat = _native.native()
    p, e, sh = _buffers(n, which, cuda, shadow=True)
    p0, e0, sh0 = p.clone(), e.clone(), sh.clone()
    nat.ema_swap(p.data_ptr(), e.data_ptr(), sh.data_ptr(), n, _sp())
    assert torch.equal(p[:n], e0[:n]) and torch.equal(e[:n], p0[:n])
    assert torch.equal(sh[:n], p[:n].bfloat16())
    assert _pads_intact(n, p, e, sh)
    nat.ema_swap(p.data_ptr(), e.data_ptr(), 0, n, _sp())  # no shadow: nothing else is written
    assert torch.equal(p, p0) and torch.equal(e, e0)
    assert torch.equal(sh[:n], e0[:n].bfloat16()) and _pads_intact(n, sh)
    del sh0


@pytest.mark.gpu
def test_kernel_path_matches_cpu_path(cuda):
    net_c, net_g = _Net(), _Net()
    flat_c, flat_g = FlatParams(net_c), FlatParams(net_g.to(cuda), with_shadow=True)
    ema_c, ema_g = E.FlatEMA(flat_c, 0.999, True), E.FlatEMA(flat_g, 0.999, True)
    assert ema_g._native and not ema_c._native
    ref = _Oracle(ema_c.e, 0.999, True)
    for s in range(5):
        _walk(flat_c, s)
        flat_g.data.copy_(flat_c.data)
        ema_c.update()
        ema_g.update()
        ref.update(flat_c.data)
    err = (ema_g.e.cpu().double() - ema_c.e.double()).abs()
    assert bool((err <= ref.bound(2.0)).all())  # each side is within the bound of the oracle
    ref.check(ema_g.e)
    p0, e0 = flat_g.data.clone(), ema_g.e.clone()
    with ema_g.applied():
        assert torch.equal(flat_g.data, e0) and torch.equal(flat_g.shadow, e0.bfloat16())
        assert torch.equal(net_g.lin.weight.data.reshape(-1), e0[flat_g.slot_of(net_g.lin.weight).offset:][:30])
    assert torch.equal(flat_g.data, p0) and torch.equal(ema_g.e, e0) and torch.equal(flat_g.shadow, p0.bfloat16())


# ------------------------------------------------------------------------------ GPU: engines
def _resnet_trainer(tmp_path, **kw):
    from faster_distributed_training_amd.train.resnet_trainer import ResNetTrainer
    return ResNetTrainer(_cfg(tmp_path, optimizer="madgrad", lr=0.02, deterministic=True, graphs=True, **kw))


@pytest.mark.gpu
def test_resnet_engine_evaluates_the_average_and_restores(cuda, tmp_path):
    """The case that goes wrong when the packed conv layouts are not refreshed after a swap."""
    from faster_distributed_training_amd.train.resnet_trainer import build_model

    def run(evaluate):
        tr = _resnet_trainer(tmp_path, ema_decay=0.5, ema_warmup=False)
        assert tr.model.use_fast_path(torch.empty(1, device=cuda)) and tr.ema._native
        it = iter(tr.train_loader)
        batches = [next(it) for _ in range(4)]
        xfix = batches[0][0].clone()
        tr.model.train()
        for x, y in batches[:3]:
            tr.train_step(x, y)
        if evaluate:
            def logits(model):
                model.eval()
                with torch.no_grad(), tr._autocast():
                    return model(xfix).float().clone()
            before = logits(tr.model)
            with tr.ema.applied():
                inside = logits(tr.model)
            with torch.random.fork_rng(devices=[cuda]):  # (its initialisation must not draw from the run's streams)
                other = build_model(tr.cfg, cuda)
            other.load_state_dict(tr.ema.model_state_dict(tr.model))
            assert torch.equal(inside, logits(other))
            assert not torch.equal(inside, before)
            assert torch.equal(logits(tr.model), before)
            tr.model.train()
        tr.train_step(*batches[3])
        torch.cuda.synchronize()
        return tr.flat.data.clone(), tr.ema.e.clone()

    pa, ea = run(True)
    pb, eb = run(False)
    assert torch.equal(pa, pb) and torch.equal(ea, eb)


@pytest.mark.gpu
def test_transformer_evaluates_the_average_through_the_shadow(cuda, monkeypatch):
    import faster_distributed_training_amd.train.transformer_trainer as T
    monkeypatch.setattr(T, "SHADOW", True)
    _native.set_deterministic(True)

    def trainer(**kw):
        torch.manual_seed(0)
        cfg = T.TransformerConfig(batch_size=32, synthetic=True, eval=False, plot=False, ngd=False, optimizer="sgd",
                                  epoch=1, steps_per_epoch=8, length_buckets=(128,), extra={"subset_stride": 50},
                                  n_layers=2, **kw)
        return T.TransformerTrainer(cfg)

    tr = trainer(ema_decay=0.5, ema_warmup=False)
    assert tr.flat.shadow is not None and tr.ema._native
    it = iter(tr.train_loader)
    batches = [next(it) for _ in range(3)]
    for b in batches:
        tr.train_step(*b)
    tokens, _, types_, masks = batches[0]

    def logits(t):
        t.model.eval()
        with torch.no_grad(), t._autocast():
            out = t.model(tokens, types_, t.pos_index, masks.view(masks.shape[0], 1, 1, -1))[0]
        return out.float().clone()

    before = logits(tr)
    p0, sh0 = tr.flat.data.clone(), tr.flat.shadow.clone()
    with tr.ema.applied():
        inside = logits(tr)
    other = trainer()
    assert [s.name for s in other.flat.slots] == [s.name for s in tr.flat.slots]
    with torch.no_grad():
        other.flat.data.copy_(tr.ema.e)
    other.flat.refresh_shadow()
    assert torch.equal(inside, logits(other))
    assert not torch.equal(inside, before)
    assert torch.equal(tr.flat.data, p0) and torch.equal(tr.flat.shadow, sh0)
    assert torch.equal(logits(tr), before)


@pytest.mark.gpu
def test_trainer_end_to_end_with_a_skipped_step(cuda, tmp_path, monkeypatch):
    """Step 2's input is made non-finite: the optimizer and the average both skip it on the device."""
    from faster_distributed_training_amd.train import resilience
    from faster_distributed_training_amd.train.resnet_trainer import ResNetTrainer
    monkeypatch.setenv("FDT_FAULT_STEP", "2")
    log = tmp_path / "log.jsonl"
    tr = ResNetTrainer(_cfg(tmp_path, bs=32, steps_per_epoch=3, epoch=2, eval=True, ema_decay=0.9, warmup_epochs=1.0,
                            nonfinite_guard=True, log_path=str(log), extra={"subset_stride": 100}))
    step = tr.train_step

    def faulty(x, y):  # FDT_FAULT_STEP names the step whose gradients go non-finite here
        try:
            return step(x, y)
        except resilience.InjectedFault:
            monkeypatch.delenv("FDT_FAULT_STEP")
            return step(torch.full_like(x, float("nan")), y)
    tr.train_step = faulty
    tr.fit()
    recs = _records(log)
    assert sum(r.get("skipped_steps", 0) for r in recs) == 1
    assert int(tr.ema.kskip) == 1 and tr.ema.k == 6 and tr.ema.applied_k == 5
    assert bool(torch.isfinite(tr.ema.e).all()) and bool(torch.isfinite(tr.flat.data).all())
    tests = [r for r in recs if "test_acc" in r]
    assert len(tests) == 2 and all(0.0 <= r["test_acc"] <= 100.0 for r in tests)
    train = [r for r in recs if "train_loss" in r]
    assert train[-1]["ema_decay_eff"] == _d(0.9, True, 4) and "lr_last_step" in train[0]

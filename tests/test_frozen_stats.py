"""Tracked FusedConvBN running statistics and batch-independent (frozen) evaluation on the
CPU / oracle path: buffers and schema, the tracking arithmetic, batch independence, checkpoint
round trips, calibration, and the CLI switches."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from faster_distributed_training_amd.models import resnet as R
from faster_distributed_training_amd.models.resnet import FusedConvBN
from faster_distributed_training_amd.train import checkpoint as ckpt
from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig, ResNetTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("running_mean", "running_var", "num_batches_tracked")


def _model(seed=0):
    torch.manual_seed(seed)
    m = R.resnet18(10)
    m.fast_path = False
    return m


def _units(m):
    return [(n, u) for n, u in m.named_modules() if isinstance(u, FusedConvBN)]


def _batches(n, bs=8, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(bs, 3, 32, 32, generator=g) for _ in range(n)]


def _tracked(momentum=0.1, batches=3):
    m = _model()
    R.enable_running_stats(m, momentum=momentum)
    m.train()
    with torch.no_grad():
        for x in _batches(batches):
            m(x)
    return m


def test_default_schema_and_buffers_unchanged():
    m = _model()
    keys = list(m.state_dict())
    bufs = [n for n, _ in m.named_buffers()]
    # the reference schema: FusedConvBN contributes its weight only, buffers come from BatchNorm2d alone
    assert all(k.endswith(("conv_weight", "weight", "bias") + STATS) for k in keys)
    assert not any("running" in k or "num_batches" in k for k in keys
                   if isinstance(m.get_submodule(k.rsplit(".", 1)[0]), FusedConvBN))
    nbn = sum(isinstance(u, torch.nn.BatchNorm2d) for u in m.modules())
    assert len(bufs) == 3 * nbn
    assert all(isinstance(m.get_submodule(n.rsplit(".", 1)[0]), torch.nn.BatchNorm2d) for n in bufs)
    assert m.eval_stats == "batch" and not any(u.track_running_stats for _, u in _units(m))
    assert FusedConvBN.track_running_stats is False and FusedConvBN.momentum == 0.1


def test_enable_running_stats_keeps_state_dict_and_adds_buffers():
    m = _model()
    keys = list(m.state_dict())
    nbuf = len(list(m.named_buffers()))
    assert R.enable_running_stats(m, momentum=0.2) is m
    assert list(m.state_dict()) == keys
    names = [n for n, _ in m.named_buffers()]
    assert len(names) == nbuf + 3 * len(_units(m))
    for n, u in _units(m):
        assert u.track_running_stats and u.momentum == 0.2
        assert all(f"{n}.{k}" in names for k in STATS)
        assert float(u.running_mean.abs().max()) == 0 and float((u.running_var - 1).abs().max()) == 0
        assert int(u.num_batches_tracked) == 0
    # (a reference-schema state_dict still loads strictly)
    m.load_state_dict(_model(3).state_dict())


@pytest.mark.parametrize("momentum", [0.1, -1.0, None])
def test_tracking_matches_hand_computation(momentum):
    m = _model()
    R.enable_running_stats(m, momentum=momentum)
    seen = {n: [] for n, _ in _units(m)}
    hooks = [u.register_forward_pre_hook(lambda mod, inp, n=n: seen[n].append(inp[0].detach().clone()))
             for n, u in _units(m)]
    m.train()
    with torch.no_grad():
        for x in _batches(3):
            m(x)
    for h in hooks:
        h.remove()
    for n, u in _units(m):
        assert len(seen[n]) == 3 and int(u.num_batches_tracked) == 3
        rm, rv = torch.zeros(u.num_features), torch.ones(u.num_features)
        means, variances = [], []
        for xin in seen[n]:
            y = F.conv2d(xin, u.conv_weight.detach(), stride=1, padding=u.padding)
            mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=True)
            means.append(mean)
            variances.append(var)
            if momentum is not None and momentum >= 0:
                rm = (1 - momentum) * rm + momentum * mean
                rv = (1 - momentum) * rv + momentum * var
        if momentum is None or momentum < 0:  # cumulative: the plain average over the batches
            rm, rv = torch.stack(means).mean(0), torch.stack(variances).mean(0)
        assert float((u.running_mean - rm).abs().max()) <= 1e-5, n
        assert float((u.running_var - rv).abs().max()) <= 1e-5, n


def test_batch_independence():
    m = _tracked()
    m.eval()
    x = _batches(1, seed=5)[0]
    with torch.no_grad():
        m.eval_stats = "running"
        one, full = m(x[:1]), m(x[:8])
        assert float((one[0] - full[0]).abs().max()) <= 1e-5
        # the defect: with batch statistics an image's logits depend on its batch
        m.eval_stats = "batch"
        one_b, full_b = m(x[:1]), m(x[:8])
    assert float((one_b[0] - full_b[0]).abs().max()) > 1e-2


def test_eval_stats_needs_tracking_and_valid_mode():
    m = _model()
    with pytest.raises(RuntimeError, match="enable_running_stats"):
        m.eval_stats = "running"
    with pytest.raises(ValueError):
        m.eval_stats = "population"
    R.enable_running_stats(m)
    m._fsdp = object()
    with pytest.raises(RuntimeError, match="FSDP"):
        m.eval_stats = "running"


def test_checkpoint_round_trip(tmp_path):
    m = _tracked()
    m.eval()
    m.eval_stats = "running"
    path = str(tmp_path / "ck" / "resnet_ckpt.pth")
    ckpt.save_checkpoint(path, m, 12.5, 3, extra={"fused_stats": R.running_stats_state(m)})
    ck = ckpt.load_checkpoint(path)
    assert set(ck["net"]) == set(_model().state_dict())  # `net` stays in the reference schema
    assert len(ck["fused_stats"]) == 3 * len(_units(m))
    m2 = _model(9)
    ckpt.load_model_state(m2, ck["net"])
    R.load_running_stats(m2, ck["fused_stats"])
    m2.eval()
    m2.eval_stats = "running"
    x = _batches(1, seed=6)[0]
    with torch.no_grad():
        assert torch.equal(m(x), m2(x))
    bad = dict(ck["fused_stats"])
    bad.pop(next(iter(bad)))
    with pytest.raises(KeyError):
        R.load_running_stats(_model(), bad)


def _cfg(tmp_path, **kw):
    base = dict(arch="resnet18", bs=8, epoch=1, synthetic=True, eval=False, plot=False, steps_per_epoch=2,
                checkpoint_dir=str(tmp_path), optimizer="madgrad", seed=7, fast_path=False,
                extra={"subset_stride": 100})
    base.update(kw)
    return ResNetConfig(**base)


def test_missing_statistics_raise_and_calibration_lifts_it(tmp_path):
    # a checkpoint in the reference schema: no FusedConvBN statistics
    ckpt.save_checkpoint(str(tmp_path / "resnet_ckpt.pth"), _model(), 10.0, 0)
    with pytest.raises(RuntimeError, match="fused_stats"):
        ResNetTrainer(_cfg(tmp_path, resume=True, eval_stats="running"))
    tr = ResNetTrainer(_cfg(tmp_path, resume=True, eval_stats="running", calibrate_batches=2))
    u = tr.model.conv1[0]
    assert int(u.num_batches_tracked) == 0
    tr.model.eval()
    tr.calibrate()
    assert int(u.num_batches_tracked) == 2 and u.momentum == 0.1 and not tr.model.training
    assert float((u.running_var - 1).abs().max()) > 1e-3
    bn = next(b for b in tr.model.modules() if isinstance(b, torch.nn.BatchNorm2d))
    assert int(bn.num_batches_tracked) == 2 and bn.momentum == 0.1
    acc = tr.test(0, save=False)  # recalibrates, then scores frozen
    assert 0.0 <= acc <= 100.0 and tr.model.eval_stats == "running"


def test_calibration_is_the_average_of_clean_batch_statistics():
    m = _tracked(momentum=0.5, batches=2)  # stale statistics, to be replaced
    xs = _batches(3, seed=11)
    m.eval()
    R.calibrate_running_stats(m, [(x, None) for x in xs])
    assert not m.training
    ref = _model()
    R.enable_running_stats(ref, momentum=None)
    for u in ref.modules():
        if isinstance(u, torch.nn.BatchNorm2d):
            u.momentum = None
    ref.train()
    with torch.no_grad():
        for x in xs:
            ref(x)
    for (n, b), (_, br) in zip(m.named_buffers(), ref.named_buffers()):
        assert torch.allclose(b.float(), br.float(), atol=1e-6), n
    assert all(u.momentum == 0.5 for _, u in _units(m))
    with pytest.raises(ValueError):
        R.calibrate_running_stats(m, [])


def test_last_checkpoint_restores_buffers_exactly(tmp_path):
    a = ResNetTrainer(_cfg(tmp_path, save_last=True, eval_stats="running")).fit()
    ck = ckpt.load_checkpoint(a.last_path)
    assert "fused_stats" in ck and set(ck["net"]) == set(_model().state_dict())
    b = ResNetTrainer(_cfg(tmp_path, auto_resume=True, eval_stats="running"))
    na, nb = dict(a.model.named_buffers()), dict(b.model.named_buffers())
    assert set(na) == set(nb) and any(k.endswith("conv1.0.running_mean") for k in na)
    for k in na:
        assert torch.equal(na[k], nb[k]), k
    assert int(a.model.conv1[0].num_batches_tracked) == 2


def test_trainer_rejects_running_stats_with_fsdp(tmp_path):
    with pytest.raises(ValueError, match="fsdp"):
        ResNetTrainer(_cfg(tmp_path, eval_stats="running", fsdp=True))
    import resnet_infer
    with pytest.raises(SystemExit):
        resnet_infer.parse(["--eval_stats", "running", "--fsdp"])
    with pytest.raises(SystemExit):
        resnet_infer.parse(["--eval_only"])
    with pytest.raises(SystemExit):
        resnet_infer.parse(["--no_such_flag"])
    # calibration would start tracking under batch statistics: refused, by the CLI and the trainer
    with pytest.raises(SystemExit):
        resnet_infer.parse(["--calibrate_batches", "2"])
    with pytest.raises(ValueError, match="eval_stats running"):
        ResNetTrainer(_cfg(tmp_path, calibrate_batches=2))
    with pytest.raises(ValueError, match="resume"):
        ResNetTrainer(_cfg(tmp_path, eval_only=True))
    a, base = resnet_infer.parse([])
    assert a.eval_stats == "batch" and a.calibrate_batches == 0 and not a.eval_only
    import resnet50_test
    assert resnet_infer.config_from_args(a, base) == resnet50_test.config_from_args(resnet50_test.parse([]))
    a, base = resnet_infer.parse(["--bs", "7", "--eval_stats", "running", "--calibrate_batches", "3", "-r", "--eval_only"])
    cfg = resnet_infer.config_from_args(a, base)
    assert (cfg.bs, cfg.eval_stats, cfg.calibrate_batches, cfg.eval_only, cfg.resume) == (7, "running", 3, True, True)


def _run(args, cwd, timeout=600):
    env = dict(os.environ, FDT_NATIVE="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_running_stats_then_eval_only_is_batch_size_independent(tmp_path):
    # resnet_infer.py is resnet50_test.py's CLI plus the inference switches; --steps is its step limit
    cli = os.path.join(ROOT, "resnet_infer.py")
    common = ["--synthetic", "--eval_stats", "running", "--arch", "resnet18", "--subset_stride", "100", "--no_plot"]
    out = _run([cli] + common + ["--epoch", "1", "--steps", "2", "--bs", "16"], tmp_path)
    assert "epoch 0:" in out and "test epoch 0" in out
    ck = torch.load(tmp_path / "checkpoint" / "resnet_ckpt.pth", weights_only=True)
    assert "fused_stats" in ck and not any("running" in k for k in ck["net"] if "conv1.0" in k)
    accs = []
    for bs in ("16", "7"):
        o = _run([cli] + common + ["--eval_only", "--resume", "--bs", bs], tmp_path)
        assert not re.search(r"^epoch \d+:", o, re.M)  # nothing is trained
        accs.append(float(re.search(r"eval-only: acc ([0-9.]+)%", o).group(1)))
    assert accs[0] == accs[1], accs


def test_launcher_two_ranks_track_and_share_statistics(tmp_path):
    """The multi-GPU launcher reaches the switches (two gloo ranks on the CPU): both ranks track,
    rank 0's statistics are broadcast before the frozen evaluation, and the checkpoint carries them."""
    env = dict(os.environ, FDT_NATIVE="0", NGPU="2", MASTER_PORT=str(30200 + os.getpid() % 400), OMP_NUM_THREADS="2",
               PYTHONPATH=ROOT)
    r = subprocess.run(["bash", os.path.join(ROOT, "run_distributed.sh"), "resnet", "--arch", "resnet18", "--bs", "8",
                        "--subset_stride", "100", "--synthetic", "--epoch", "1", "--steps", "2", "--no_plot",
                        "--eval_stats", "running", "--checkpoint_dir", str(tmp_path / "ck")],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "epoch 0:" in r.stdout and "test epoch 0" in r.stdout
    ck = torch.load(tmp_path / "ck" / "resnet_ckpt.pth", weights_only=True)
    assert all(k.startswith("module.") for k in ck["net"]) and not any("running" in k for k in ck["net"] if "conv1.0" in k)
    assert int(ck["fused_stats"]["conv1.0.num_batches_tracked"]) == 2

"""Per-step LR warm-up on top of the per-epoch schedulers (train/resnet_trainer.py ``scaled_lr``), and
the contract that a run with the EMA / warm-up fields at their defaults is untouched.

For global step s < S = round(warmup_epochs * steps per epoch) the optimizer steps with
scheduler_lr(epoch) * f(s), f(s) = start + (1 - start) s / S; the scaled value is put back after the
step, so the (recursive) cosine scheduler's per-epoch sequence is the one of a run without warm-up."""
import json

import pytest
import torch

from faster_distributed_training_amd.ops import _native
from faster_distributed_training_amd.train.resnet_trainer import (ResNetConfig, ResNetTrainer, check_warmup_config,
                                                                  warmup_factor)

NEW_NAMES = {"ema", "ema_state", "ema_decay_eff", "lr_last_step", "ema_decay", "warmup_epochs"}


@pytest.fixture(autouse=True)
def _reset_deterministic():
    yield
    _native.set_deterministic(False)


def _cfg(tmp_path, **kw):
    base = dict(arch="resnet18", bs=8, epoch=3, synthetic=True, eval=False, plot=False, steps_per_epoch=4,
                checkpoint_dir=str(tmp_path), optimizer="sgd", lr=0.05, seed=7, deterministic=True,
                extra={"subset_stride": 500})
    base.update(kw)
    return ResNetConfig(**base)


def _run(cfg):
    """Fit, recording the lr every optimizer step saw and the scheduler's rate in every epoch."""
    tr = ResNetTrainer(cfg)
    seen, sched = [], []
    inner, epoch = tr.optimizer._step, tr.train_epoch

    def spy_step(*a, **k):
        seen.append(tr.optimizer.group["lr"])
        return inner(*a, **k)

    def spy_epoch(e):
        sched.append(tr.scheduler.get_last_lr()[0])
        assert tr.optimizer.group["lr"] == sched[-1]  # nothing scaled is left behind between steps
        return epoch(e)
    tr.optimizer._step, tr.train_epoch = spy_step, spy_epoch
    tr.fit()
    return tr, seen, sched


def _records(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def test_warmup_scales_each_step_and_leaves_the_scheduler_alone(tmp_path):
    log = tmp_path / "w.jsonl"
    tw, seen_w, sched_w = _run(_cfg(tmp_path / "w", warmup_epochs=1.5, log_path=str(log)))
    t0, seen_0, sched_0 = _run(_cfg(tmp_path / "0"))
    S, start = 6, 0.1
    assert tw.warmup_steps == S and t0.warmup_steps == 0 and len(seen_w) == len(seen_0) == 12
    assert sched_w == sched_0 and len(set(sched_0)) == 3  # cosine: a new rate every epoch, untouched by the warm-up
    assert tw.optimizer.group["lr"] == t0.optimizer.group["lr"]
    for s in range(12):
        base = sched_0[s // 4]
        assert seen_0[s] == base
        if s < S:
            assert seen_w[s] == base * (start + (1.0 - start) * s / S)  # exactly
            assert seen_w[s] < base
        else:
            assert seen_w[s] == seen_0[s]  # bitwise: the rate is not touched from step S on
    assert seen_w[0] == sched_0[0] * start
    # the epoch record keeps the scheduler's value and gains the last step's
    recs = [r for r in _records(log) if "train_loss" in r]
    assert [r["lr"] for r in recs] == sched_0
    assert [r["lr_last_step"] for r in recs] == [seen_w[3], seen_w[7], seen_w[11]]
    assert not any("lr_last_step" in r for r in _records(log) if "train_loss" not in r)


def test_warmup_factor_and_config_checks():
    assert warmup_factor(0, 6, 0.1) == 0.1 and warmup_factor(3, 6, 0.1) == 0.1 + 0.9 * 3 / 6
    assert warmup_factor(6, 6, 0.1) is None and warmup_factor(0, 0, 0.1) is None
    check_warmup_config(0.0, 0.1)
    check_warmup_config(2.5, 1.0)
    with pytest.raises(ValueError):
        check_warmup_config(-1.0, 0.1)
    with pytest.raises(ValueError):
        ResNetConfig(warmup_epochs=1.0, warmup_start_factor=1.5)


def test_defaults_change_nothing(tmp_path):
    """Run 1 sets none of the new fields, run 2 sets ema_decay=0.0 and warmup_epochs=0.0 explicitly: the
    same trajectory, and none of the new names in the records or in the best checkpoint."""

    def run(name, **kw):
        log = tmp_path / f"{name}.jsonl"
        tr = ResNetTrainer(_cfg(tmp_path / name, epoch=2, eval=True, save_last=True, log_path=str(log), **kw))
        lrs = []
        inner = tr.optimizer._step

        def spy(*a, **k):
            lrs.append(tr.optimizer.group["lr"])
            return inner(*a, **k)
        tr.optimizer._step = spy
        tr.fit()
        assert tr.ema is None and tr.warmup_steps == 0 and tr.lr_last_step is None
        return tr, _records(log), lrs

    a, ra, la = run("a")
    b, rb, lb = run("b", ema_decay=0.0, warmup_epochs=0.0)
    assert torch.equal(a.flat.data, b.flat.data) and la == lb
    for recs in (ra, rb):
        assert recs and not any(NEW_NAMES & set(r) for r in recs)
        assert not any(NEW_NAMES & set(r.get("config", {})) for r in recs)
    for tr in (a, b):
        best = torch.load(tr.ckpt_path, weights_only=True)
        assert set(best) == {"net", "acc", "epoch"}
        last = torch.load(tr.last_path, weights_only=True)
        assert not NEW_NAMES & set(last)
    assert [{k: v for k, v in r.items() if k not in ("time", "epoch_time_s", "img_per_s", "peak_mem_gb")} for r in ra] == \
           [{k: v for k, v in r.items() if k not in ("time", "epoch_time_s", "img_per_s", "peak_mem_gb")} for r in rb]


@pytest.mark.gpu
def test_ngd_graph_replays_pick_the_scaled_rate_up(cuda):
    """NGD replayed as HIP graphs reads [lr, momentum] from its device ``lr_dev``, filled from
    ``group["lr"]`` before every replay: a step under ``scaled_lr`` replays with the scaled rate (as
    tests/test_ngd_graphs.py: eager and replayed optimizers from the same state, same gradients)."""
    import torch.nn as nn
    from faster_distributed_training_amd.optim.ngd import NGD
    from faster_distributed_training_amd.train.resnet_trainer import scaled_lr
    from faster_distributed_training_amd.utils.flat import FlatParams

    def make(graphs):
        torch.manual_seed(0)
        m = nn.Sequential(nn.Conv2d(64, 64, 3), nn.Conv2d(64, 128, 1), nn.Linear(256, 512), nn.Linear(512, 96)).to(cuda)
        flat = FlatParams(m, device=cuda)
        opt = NGD(flat, lr=0.05, momentum=0.9, weight_decay=1e-4)
        opt.graphs = graphs
        return flat, opt

    fa, oa = make(False)
    fb, ob = make(True)
    gen = torch.Generator().manual_seed(1)
    coef = torch.ones((), device=cuda)
    S, start, steps = 18, 0.1, 22  # the warm-up ends inside the replayed range (replays start at step 10)
    for s in range(steps):
        g = (torch.randn(fa.numel, generator=gen) * 1e-2).to(cuda)
        fa.grad.copy_(g)
        fb.grad.copy_(g)
        f = warmup_factor(s, S, start)
        before = fb.data.clone()
        for o in (oa, ob):
            if f is None:
                o.step(grad_scale=coef)
            else:
                with scaled_lr(o, f):
                    o.step(grad_scale=coef)
            assert o.group["lr"] == 0.05  # put back
            o.sync_state()
        torch.cuda.synchronize()
        err = ((fa.data - fb.data).abs().max() / fa.data.abs().max()).item()
        assert err <= 1e-6, (s, err)
        if ob.graph_replays:
            want = torch.tensor(0.05 * (1.0 if f is None else f), dtype=torch.float32)
            assert float(ob.lr_dev[0]) == float(want), (s, float(ob.lr_dev[0]))
        assert not torch.equal(before, fb.data)
    assert ob.graph_replays == steps - 10 and oa.graph_replays == 0

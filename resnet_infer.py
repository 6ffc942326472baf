#!/usr/bin/env python3
"""Train ResNet with tracked FusedConvBN statistics, and evaluate a checkpoint batch-independently.

Takes every flag of ``resnet50_test.py`` (which stays CLI-compatible with the reference) and adds
the inference switches:

  --eval_stats {batch,running}   statistics the FusedConvBN units evaluate with (default: batch)
  --calibrate_batches N          re-estimate the running statistics on N clean training batches
                                 before each evaluation
  --eval_only                    with --resume: load, (calibrate,) evaluate once and exit

and the data set switch:

  --dataset {cifar10,cifar100}   cifar100: 100 fine labels, checkpoints resnet_cifar100_*.pth, top-5 in the evaluation

and the training-recipe switches:

  --cutmix_prob P                share of the steps that use CutMix instead of input mixup (1: CutMix only)
  --cutmix_alpha A               Beta(A, A) for the CutMix box area (default 1)
  --cutmix_per_sample            a box per sample (default: one box per batch)
  --label_smoothing E            smoothing of the training loss, 0 <= E < 1 (the evaluation loss stays unsmoothed)

and the large-batch optimizers (layer-wise trust ratios, ``optim/flat_optim.py`` LARS / LAMB):

  --optimizer {lars,lamb}        besides every value ``resnet50_test.py`` takes, which are passed on to it
  --trust_coef ETA               LARS trust coefficient (default 1e-3; <= 0: no trust ratio, plain SGD)

and their companions, a weight EMA (``optim/ema.py``) and a per-step LR warm-up:

  --ema_decay D                  > 0: average the weights after every step, evaluate and checkpoint the average
  --no_ema_warmup                use D from the first update (default: min(D, (1 + t) / (10 + t)))
  --warmup_epochs E              linear per-step LR warm-up over E epochs (fractions allowed)
  --warmup_start_factor F        the first step's share of the scheduled rate (default 0.1)
  --eval_ema                     with --resume --eval_only: score the checkpoint's averaged weights

Without the new switches it behaves exactly like ``resnet50_test.py``.

Examples:
    python resnet_infer.py --eval_stats running                       # track statistics, evaluate frozen
    python resnet_infer.py --eval_stats running --resume --eval_only --bs 1
    python resnet_infer.py --eval_stats running --calibrate_batches 8 --resume --eval_only
    python resnet_infer.py --dataset cifar100 --synthetic --bs 256 --epoch 1
    python resnet_infer.py --dataset cifar100 --cutmix_prob 0.5 --label_smoothing 0.1
    python resnet_infer.py --synthetic --bs 1024 --optimizer lars --lr 0.4
    python resnet_infer.py --bs 1024 --optimizer lars --lr 0.4 --warmup_epochs 5 --ema_decay 0.999
    python resnet_infer.py --resume --eval_only --eval_ema            # score the averaged weights of a checkpoint
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resnet50_test  # noqa: E402


def parse(argv=None):
    """-> (inference switches, ``resnet50_test`` arguments)."""
    p = argparse.ArgumentParser(description="ResNet inference switches; every other flag is resnet50_test.py's",
                                add_help=False, allow_abbrev=False)
    p.add_argument("--eval_stats", default="batch", choices=["batch", "running"],
                   help="statistics the FusedConvBN units evaluate with: the batch's (reference behaviour) or "
                        "tracked running statistics (batch-independent inference)")
    p.add_argument("--calibrate_batches", default=0, type=int,
                   help="before each evaluation, re-estimate the running statistics on N clean training batches")
    p.add_argument("--eval_only", action="store_true", help="with --resume: load, (calibrate,) evaluate once and exit")
    p.add_argument("--dataset", default="cifar10", choices=["cifar10", "cifar100"],
                   help="cifar100: the 100 fine labels, a 100-class head, checkpoints in resnet_cifar100_*.pth, "
                        "top-5 accuracy in the evaluation")
    p.add_argument("--cutmix_prob", default=0.0, type=float,
                   help="share of the training steps that use CutMix instead of input mixup (1: CutMix only)")
    p.add_argument("--cutmix_alpha", default=1.0, type=float, help="Beta(alpha, alpha) for the CutMix box area")
    p.add_argument("--cutmix_per_sample", action="store_true", help="a CutMix box per sample (default: one per batch)")
    p.add_argument("--label_smoothing", default=0.0, type=float,
                   help="label smoothing of the training loss, in [0, 1); the evaluation loss stays unsmoothed")
    p.add_argument("--optimizer", default=None,
                   help="lars / lamb: layer-wise trust ratios (SGD / AdamW form); any other value is resnet50_test.py's")
    p.add_argument("--trust_coef", default=1e-3, type=float,
                   help="--optimizer lars: trust coefficient eta (<= 0: no trust ratio, plain SGD)")
    p.add_argument("--ema_decay", default=0.0, type=float,
                   help="> 0: keep an exponential moving average of the weights (one fused launch per step) and "
                        "evaluate it; the best checkpoint gains an 'ema' entry")
    p.add_argument("--no_ema_warmup", action="store_true",
                   help="use --ema_decay from the first update (default: min(decay, (1 + t) / (10 + t)))")
    p.add_argument("--warmup_epochs", default=0.0, type=float,
                   help="linear per-step LR warm-up over this many epochs (fractions allowed), on top of the scheduler")
    p.add_argument("--warmup_start_factor", default=0.1, type=float,
                   help="share of the scheduled rate that the first step takes under --warmup_epochs")
    p.add_argument("--eval_ema", action="store_true",
                   help="with --resume --eval_only: load the checkpoint's averaged weights ('ema' entry) instead of 'net'")
    argv = list(sys.argv[1:] if argv is None else argv)
    if "-h" in argv or "--help" in argv:
        p.print_help()
        print()
    a, rest = p.parse_known_args(argv)
    from faster_distributed_training_amd.optim.flat_optim import LAYERWISE, check_layerwise_config
    if a.optimizer is not None and a.optimizer not in LAYERWISE:
        rest += ["--optimizer", a.optimizer]  # (one of its own: it checks the choice)
        a.optimizer = None
    base = resnet50_test.parse(rest)
    check_layerwise_config(a.optimizer or base.optimizer, base.fsdp)  # (a ValueError, with the reason)
    from faster_distributed_training_amd.optim.ema import check_ema_config
    from faster_distributed_training_amd.train.resnet_trainer import (check_eval_config, check_mix_config,
                                                                      check_warmup_config)
    try:
        check_ema_config(a.ema_decay, base.fsdp)  # (sharded NGD: the trainer refuses, once the world is known)
        check_warmup_config(a.warmup_epochs, a.warmup_start_factor)
        if a.eval_ema and not (a.eval_only and base.resume):
            raise ValueError("--eval_ema scores a checkpoint's averaged weights: pass --resume --eval_only")
        check_eval_config(a.eval_stats, base.fsdp, a.calibrate_batches, a.eval_only, base.resume)
        check_mix_config(a.cutmix_prob, a.label_smoothing, base.meta_learning)
    except ValueError as e:
        p.error(str(e))
    return a, base


def config_from_args(a, base):
    # (num_classes=None: the data set decides)
    return dataclasses.replace(resnet50_test.config_from_args(base), eval_stats=a.eval_stats,
                               calibrate_batches=a.calibrate_batches, eval_only=a.eval_only,
                               dataset=a.dataset, num_classes=None, cutmix_prob=a.cutmix_prob,
                               cutmix_alpha=a.cutmix_alpha, cutmix_per_sample=a.cutmix_per_sample,
                               label_smoothing=a.label_smoothing, trust_coef=a.trust_coef,
                               ema_decay=a.ema_decay, ema_warmup=not a.no_ema_warmup,
                               warmup_epochs=a.warmup_epochs, warmup_start_factor=a.warmup_start_factor,
                               eval_ema=a.eval_ema,
                               **({"optimizer": a.optimizer} if a.optimizer else {}))


def main(argv=None):
    a, base = parse(argv)
    from faster_distributed_training_amd.train.resnet_trainer import main_ddp
    return main_ddp(config_from_args(a, base))  # (fit, or with --eval_only one evaluation; then cleanup)


if __name__ == "__main__":
    main()

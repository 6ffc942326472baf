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

Without the new switches it behaves exactly like ``resnet50_test.py``.

Examples:
    python resnet_infer.py --eval_stats running                       # track statistics, evaluate frozen
    python resnet_infer.py --eval_stats running --resume --eval_only --bs 1
    python resnet_infer.py --eval_stats running --calibrate_batches 8 --resume --eval_only
    python resnet_infer.py --dataset cifar100 --synthetic --bs 256 --epoch 1
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
    argv = list(sys.argv[1:] if argv is None else argv)
    if "-h" in argv or "--help" in argv:
        p.print_help()
        print()
    a, rest = p.parse_known_args(argv)
    base = resnet50_test.parse(rest)
    from faster_distributed_training_amd.train.resnet_trainer import check_eval_config
    try:
        check_eval_config(a.eval_stats, base.fsdp, a.calibrate_batches, a.eval_only, base.resume)
    except ValueError as e:
        p.error(str(e))
    return a, base


def config_from_args(a, base):
    # (num_classes=None: the data set decides)
    return dataclasses.replace(resnet50_test.config_from_args(base), eval_stats=a.eval_stats,
                               calibrate_batches=a.calibrate_batches, eval_only=a.eval_only,
                               dataset=a.dataset, num_classes=None)


def main(argv=None):
    a, base = parse(argv)
    from faster_distributed_training_amd.train.resnet_trainer import main_ddp
    return main_ddp(config_from_args(a, base))  # (fit, or with --eval_only one evaluation; then cleanup)


if __name__ == "__main__":
    main()

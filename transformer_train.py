#!/usr/bin/env python3
"""Train the Transformer text classifier with the large-batch optimizers.

Takes every flag of ``transformer_test.py`` (which stays CLI-compatible with the reference) and adds
the layer-wise trust ratios of ``optim/flat_optim.py`` (LARS / LAMB):

  --optimizer {lamb,lars}        besides every value ``transformer_test.py`` takes, which are passed on to it
  --trust_coef ETA               LARS trust coefficient (default 1e-3; <= 0: no trust ratio, plain SGD)

and their companions, a weight EMA (``optim/ema.py``) and a per-step LR warm-up:

  --ema_decay D                  > 0: average the weights after every step, evaluate and checkpoint the average
  --no_ema_warmup                use D from the first update (default: min(D, (1 + t) / (10 + t)))
  --warmup_epochs E              linear per-step LR warm-up over E epochs (fractions allowed), on top of OneCycleLR
  --warmup_start_factor F        the first step's share of the scheduled rate (default 0.1)

Without the new switches it behaves exactly like ``transformer_test.py``.  ``--fsdp`` with ``lars`` or
``lamb`` is refused: an FSDP shard view holds no whole parameter slots; ``--ema_decay`` is refused under
``--fsdp`` and sharded NGD, where a rank holds only a shard of the weights.

``run_distributed.sh transformer`` starts this file, so the multi-GPU launcher reaches both.

Examples:
    python transformer_train.py --synthetic -b 256 --epoch 1 --optimizer lamb --lr 1e-3
    NGPU=8 bash run_distributed.sh transformer --optimizer lamb --lr 1e-3
    python transformer_train.py --synthetic --epoch 1 --ema_decay 0.999 --warmup_epochs 0.5
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import transformer_test  # noqa: E402


def parse(argv=None):
    """-> (optimizer switches, ``transformer_test`` arguments)."""
    p = argparse.ArgumentParser(description="Large-batch optimizer switches; every other flag is transformer_test.py's",
                                add_help=False, allow_abbrev=False)
    p.add_argument("--optimizer", default=None,
                   help="lamb / lars: layer-wise trust ratios (AdamW / SGD form); any other value is transformer_test.py's")
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
    argv = list(sys.argv[1:] if argv is None else argv)
    if "-h" in argv or "--help" in argv:
        p.print_help()
        print()
    a, rest = p.parse_known_args(argv)
    from faster_distributed_training_amd.optim.flat_optim import LAYERWISE, check_layerwise_config
    if a.optimizer is not None and a.optimizer not in LAYERWISE:
        rest += ["--optimizer", a.optimizer]  # (one of its own: it checks the choice)
        a.optimizer = None
    base = transformer_test.parse(rest)
    check_layerwise_config(a.optimizer or base.optimizer, base.fsdp)  # (a ValueError, with the reason)
    from faster_distributed_training_amd.optim.ema import check_ema_config
    from faster_distributed_training_amd.train.resnet_trainer import check_warmup_config
    check_ema_config(a.ema_decay, base.fsdp)  # (sharded NGD: the trainer refuses, once the world is known)
    check_warmup_config(a.warmup_epochs, a.warmup_start_factor)
    return a, base


def config_from_args(a, base):
    return dataclasses.replace(transformer_test.config_from_args(base), trust_coef=a.trust_coef,
                               ema_decay=a.ema_decay, ema_warmup=not a.no_ema_warmup,
                               warmup_epochs=a.warmup_epochs, warmup_start_factor=a.warmup_start_factor,
                               **({"optimizer": a.optimizer} if a.optimizer else {}))


def main(argv=None):
    a, base = parse(argv)
    from faster_distributed_training_amd.parallel.dist import cleanup
    from faster_distributed_training_amd.train.transformer_trainer import TransformerTrainer
    trainer = TransformerTrainer(config_from_args(a, base))
    trainer.fit()
    cleanup()
    return trainer


if __name__ == "__main__":
    main()

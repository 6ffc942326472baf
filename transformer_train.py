#!/usr/bin/env python3
"""Train the Transformer text classifier with the large-batch optimizers.

Takes every flag of ``transformer_test.py`` (which stays CLI-compatible with the reference) and adds
the layer-wise trust ratios of ``optim/flat_optim.py`` (LARS / LAMB):

  --optimizer {lamb,lars}        besides every value ``transformer_test.py`` takes, which are passed on to it
  --trust_coef ETA               LARS trust coefficient (default 1e-3; <= 0: no trust ratio, plain SGD)

Without the new switches it behaves exactly like ``transformer_test.py``.  ``--fsdp`` with ``lars`` or
``lamb`` is refused: an FSDP shard view holds no whole parameter slots.

``run_distributed.sh transformer`` starts this file, so the multi-GPU launcher reaches both.

Examples:
    python transformer_train.py --synthetic -b 256 --epoch 1 --optimizer lamb --lr 1e-3
    NGPU=8 bash run_distributed.sh transformer --optimizer lamb --lr 1e-3
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
    return a, base


def config_from_args(a, base):
    return dataclasses.replace(transformer_test.config_from_args(base), trust_coef=a.trust_coef,
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

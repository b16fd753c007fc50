#!/usr/bin/env python3
"""Golden figures for the evaluation loop, from the REFERENCE itself: its ``evaluations.test``, imported unmodified, run on the CPU with
``nn.CrossEntropyLoss()`` over an ``nn.Identity()`` model and a DataLoader of fixed fp32 logits -- so the figures depend on the logits,
the targets and the batch size alone (torch.max's tie rule, the mean of BATCH means, scikit-learn's macro averages at zero_division=0).

The fixtures go to tests/golden/eval/<case>.npz -- a subdirectory, so the enumerations of tests/golden/*.npz see nothing new.  Each holds
    logits [N, C] fp32, targets [N] int64, batch_size
    loss, accuracy, precision, recall, f1      what evaluations.test returned (fp64; the inference time is dropped)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py <path of the reference checkout>
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "eval")
sys.dont_write_bytecode = True
SEED0 = 9300


def case_c10():
    """10 classes, 37 samples in batches of 8: the last batch holds 5, so a per-sample mean differs from the mean of batch means."""
    logits = 2.0 * torch.randn(37, 10)
    targets = torch.randint(0, 10, (37,))
    hit = torch.rand(37) < 0.6
    logits[hit, targets[hit]] += 4.0
    return logits, targets, 8


def case_c100():
    """100 classes, 50 samples: most classes are absent, some are only predicted, some only targets."""
    logits = torch.randn(50, 100)
    targets = torch.randint(0, 100, (50,))
    hit = torch.rand(50) < 0.5
    logits[hit, targets[hit]] += 6.0
    return logits, targets, 16


def case_ties():
    """Small integer logits: most rows hold their maximum more than once, and the lowest index must win."""
    logits = torch.randint(-1, 3, (20, 6)).float()
    targets = torch.randint(0, 6, (20,))
    return logits, targets, 7


CASES = {"c10_n37_b8": case_c10, "c100_n50_b16": case_c100, "ties_c6_n20_b7": case_ties}


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import evaluations as REF                    # the reference module
    os.makedirs(OUT, exist_ok=True)
    for i, (name, make) in enumerate(CASES.items()):
        torch.manual_seed(SEED0 + i)
        logits, targets, bs = make()
        loader = DataLoader(TensorDataset(logits, targets), batch_size=bs, shuffle=False)
        loss, acc, prec, rec, f1, _ = REF.test(nn.Identity(), torch.device("cpu"), loader, 0, nn.CrossEntropyLoss())
        pred = logits.max(1)[1]
        ties = int((logits == logits.max(1, keepdim=True)[0]).sum(1).gt(1).sum())
        only_pred = len(set(pred.tolist()) - set(targets.tolist()))
        only_true = len(set(targets.tolist()) - set(pred.tolist()))
        absent = logits.shape[1] - len(set(pred.tolist()) | set(targets.tolist()))
        path = os.path.join(OUT, name + ".npz")
        np.savez(path, logits=logits.numpy(), targets=targets.numpy(), batch_size=np.int64(bs), loss=np.float64(loss), accuracy=np.float64(acc),
                 precision=np.float64(prec), recall=np.float64(rec), f1=np.float64(f1))
        size = os.path.getsize(path)
        print(f"{name:16s} {size / 1024:5.1f} KiB  loss {loss:.6f} acc {acc:.4f} P {prec:.4f} R {rec:.4f} F1 {f1:.4f}  rows with tied maxima {ties}, "
              f"classes only predicted {only_pred} / only targets {only_true} / absent {absent}")
        assert size <= 128 * 1024, (name, size)


if __name__ == "__main__":
    main()

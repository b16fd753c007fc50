"""The criterion and the test metrics of the reference's loop, kept on the device.

``CrossEntropyLoss`` is generic_train.py:26's ``nn.CrossEntropyLoss()`` on the kernels of csrc/kan_loss.hip; ``ClassMetrics`` owns the counters
those kernels add to, and turns them into what evaluations.py:146-151 returns (loss, accuracy, scikit-learn's macro precision / recall / F1 at
``zero_division=0``) with ONE device read, where the reference reads the loss and the correct count every batch and copies every prediction.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import ops


def _ints(v):
    return [int(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]


class ClassMetrics:
    """The metrics buffer of ``ops.cross_entropy`` for ``num_classes`` classes: int64 words [correct, samples, batches, bad_target,
    loss_sum (the bits of a double), 3 unused], then tp[C], pred[C], true[C] (include/kanconv.h).  Every ``cross_entropy(..., metrics=self)``
    adds one batch to it on the device; ``result()`` is the only host read."""

    def __init__(self, num_classes: int, device="cuda"):
        if int(num_classes) < 1:
            raise ValueError(f"num_classes must be at least 1, got {num_classes}")
        self.num_classes = int(num_classes)
        self.buffer = torch.zeros(L.XENT_HEADER_WORDS + 3 * self.num_classes, dtype=torch.int64, device=device)

    def reset(self) -> None:
        self.buffer.zero_()

    def result(self) -> Dict[str, float]:
        """One device read.  Raises ``KanConvError`` if any batch held a target outside [0, num_classes)."""
        host = self.buffer.cpu()
        head, Cn = host[:L.XENT_HEADER_WORDS], self.num_classes
        if int(head[3]) != 0:
            raise L.KanConvError(f"{int(head[3])} target(s) outside [0, {Cn}) since the last reset: those rows were left out of the loss, "
                                 "the gradients and every counter")
        per_class = host[L.XENT_HEADER_WORDS:].reshape(3, Cn)
        return self.summarize(per_class[0], per_class[1], per_class[2], int(head[0]), int(head[1]), int(head[2]),
                              float(head[4:5].view(torch.float64)))

    @staticmethod
    def summarize(tp, pred, true, correct: int, samples: int, batches: int, loss_sum: float) -> Dict[str, float]:
        """The figures of evaluations.py:146-151 from the counters, in fp64: per class precision = tp / pred, recall = tp / true,
        F1 = 2 tp / (pred + true), each 0 where its denominator is 0 (``zero_division=0``), averaged over the classes that occur among the
        targets or the predictions (scikit-learn's macro average drops labels that appear in neither); loss = loss_sum / batches (a mean of batch
        means), accuracy = correct / samples.  Pure: no device, no state."""
        tp, pred, true = _ints(tp), _ints(pred), _ints(true)
        if not len(tp) == len(pred) == len(true):
            raise ValueError("tp, pred and true must have one entry per class")
        seen = [c for c in range(len(tp)) if pred[c] + true[c] > 0]

        def macro(num, den):
            return sum((num(c) / den(c) if den(c) > 0 else 0.0) for c in seen) / len(seen) if seen else 0.0
        return {"loss": float(loss_sum) / batches if batches > 0 else 0.0,
                "accuracy": correct / samples if samples > 0 else 0.0,
                "precision": macro(lambda c: tp[c], lambda c: pred[c]),
                "recall": macro(lambda c: tp[c], lambda c: true[c]),
                "f1": macro(lambda c: 2 * tp[c], lambda c: pred[c] + true[c]),
                "samples": int(samples), "batches": int(batches)}


class CrossEntropyLoss(nn.Module):
    """``nn.CrossEntropyLoss()`` as the reference builds it (generic_train.py:26: mean reduction, nothing else), on this project's kernels.
    ``metrics``: a ``ClassMetrics`` that every forward adds its batch to (training accuracy without a host read).  ``train_step`` takes it as
    ``criterion=``; ``GraphedStep`` refuses it (recording these launches into a HIP graph is not supported yet)."""

    def __init__(self, weight=None, size_average=None, ignore_index: int = -100, reduce=None, reduction: str = "mean",
                 label_smoothing: float = 0.0, metrics: Optional[ClassMetrics] = None):
        super().__init__()
        unsupported = [name for name, off in (("weight", weight is None), ("size_average", size_average is None),
                                              ("ignore_index", ignore_index == -100), ("reduce", reduce is None),
                                              ("reduction", reduction == "mean"), ("label_smoothing", label_smoothing == 0.0)) if not off]
        if unsupported:
            raise NotImplementedError(f"CrossEntropyLoss: {', '.join(unsupported)} not supported (mean reduction over all rows only, as the "
                                      "reference uses it)")
        self.metrics = metrics

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return ops.cross_entropy(input, target, self.metrics)

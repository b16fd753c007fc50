"""Training-step harness around the hot path -- SURVEY.md section 8(f) rank 4.

Mirrors the reference's loop: ``optim.AdamW(lr, weight_decay)`` + ``ExponentialLR(gamma)`` + ``CrossEntropyLoss``
(generic_train.py:24-26), one ``zero_grad / forward / loss / backward / step`` per batch (evaluations.py:41-72) and one
scheduler step per epoch (evaluations.py: train_and_test_models), with the optimizer replaced by ``FusedAdamW`` and, under
``torch.distributed``, the gradient mean taken by ``BucketedGradReducer`` between backward and step.  Everything stays on
the launch stream: the only host synchronisation is the once-per-epoch read of the accumulated loss (the reference reads
``loss.item()`` every batch).  ``evaluate`` and ``train_and_test_models`` add the second half of that loop (evaluations.py:81-247: test loss,
accuracy, macro precision / recall / F1 after every epoch) under the same rule: the loss and the counting run in the kernels of
csrc/kan_loss.hip and the counters are read once per evaluation.  Datasets, checkpoints, early stopping and plots stay out of scope
(section 8: control plane).
"""
from __future__ import annotations

import contextlib
import warnings
from typing import Iterable, List, Optional, Tuple

import torch
import torch.nn as nn

from .optim import FusedAdamW


def train_step(model: nn.Module, data: torch.Tensor, target: torch.Tensor, optimizer: torch.optim.Optimizer,
               criterion: Optional[nn.Module] = None, reducer=None, split_precision: bool = False) -> torch.Tensor:
    """One batch: returns the (detached, device-resident) loss.  ``split_precision``: OPT-IN, the forward and backward of this step run inside
    ``ops.split_precision_training()`` (the conv launches of the layers in its scope in split precision; everything else exact).
    With ``optimizer.accumulate_steps = k > 1`` (``FusedAdamW``) the call is a micro-step: the gradients are still zeroed and recomputed per call --
    the optimizer accumulates them itself -- and only every k-th call updates; the loss returned is the micro-batch's.  Folding the reducer's
    ``no_sync()`` into this is not built: with a reducer every micro-step still all-reduces, which is correct (the mean of means) but wasteful."""
    criterion = criterion if criterion is not None else nn.CrossEntropyLoss()
    optimizer.zero_grad()
    with _split_context(split_precision):
        loss = criterion(model(data), target)
        loss.backward()
    if reducer is not None:
        reducer.finish()
    optimizer.step()
    return loss.detach()


def _split_context(on: bool):
    from . import ops
    return ops.split_precision_training() if on else contextlib.nullcontext()


class GraphedStep:
    """zero_grad / forward / loss / backward of ``model`` on fixed shapes -- and, with ``optimizer=``, the optimizer step -- recorded ONCE into a HIP
    graph and replayed per batch.

    Every launch of the hot path goes through ctypes onto torch's current stream, so ``torch.cuda.graph`` captures the conv-KAN kernels next to
    torch's own; a replay costs one graph launch instead of the host's per-kernel work.  That pays where the step is launch-bound -- small models and
    single layers (BASELINE config 2: 0.23 ms replayed against 0.43-0.48 ms eager, bit-identical); KAN-VGG11 at bs 256 keeps the GPU busy either way.
    The weight packs are recorded unconditionally (``ops.always_pack``): the replay reads the weights as they are at replay time, so an optimizer may
    update them in place between replays.  ``split_precision=True`` (OPT-IN) warms up and records inside ``ops.split_precision_training()``.
    Do not call ``zero_grad`` between replays: the recorded backward assigns ``p.grad`` (static tensors) rather than accumulating.  To accumulate,
    set ``optimizer.accumulate_steps = k`` before this object is built: the recorded ``step()`` is then a micro-step whose window counter lives on
    the device -- ONE graph, replayed per micro-batch, and every k-th replay updates; the warm-up's micro-steps are undone with the rest, so the
    first replay is micro-step 0 of a fresh window.  ``loss`` stays the micro-batch's loss.
    The criterion inside a recorded step is torch's: ``convkan_amd.CrossEntropyLoss`` (the device-side counters of ``ClassMetrics``) is refused here --
    recording it is not supported yet; ``train_step`` takes it.

    ``optimizer``: None, or a ``FusedAdamW(capturable=True)`` (anything else: ValueError).  Its ``step()`` is then the last thing of the recorded
    region -- it reads lr and the step counts from device memory, so replay k computes step k.  The warm-up runs full steps, optimizer included, and
    then the parameters, both moments and the step counts are put back to what they were: the first replay starts from the state the first eager
    step would.  Each call brings lr up to date (``optimizer.sync_hyper()``: nothing unless a scheduler moved it), replays, and bumps the version
    counter of every parameter the recorded step updates, so that a later eager forward (``evaluate``, a ragged last batch through ``train_step``)
    sees the new weights through the packed-weight cache.  Which parameters have a gradient, betas, eps and weight_decay are frozen at recording
    time.  Gradient clipping travels with the optimizer (``FusedAdamW(..., max_grad_norm=c)``): its norm kernels are part of the recorded step, and
    ``max_grad_norm`` itself is read from device memory at replay time, like lr.  So does the non-finite guard (``optimizer.skip_nonfinite = True``
    before this object is built: the decision is taken on the device at every replay, and the warm-up leaves the guard's counters where it found
    them); an ``AnomalyProbe`` attached to ``model`` before this object is built is recorded too, and every replay counts.  Not built: a recorded ``convkan_amd.CrossEntropyLoss``, and a DP
    reducer inside the graph.

        step = GraphedStep(model, example_data, example_target, optimizer=opt)       # opt = FusedAdamW(..., capturable=True)
        for data, target in batches:
            loss = step(data, target)          # device-resident, overwritten by the next call

    Without ``optimizer`` the caller steps after each call (any optimizer that updates the parameters in place).
    """

    def __init__(self, model: nn.Module, example_data: torch.Tensor, example_target: torch.Tensor, criterion: Optional[nn.Module] = None,
                 warmup: int = 3, split_precision: bool = False, optimizer=None):
        from . import ops
        from .loss import CrossEntropyLoss
        if isinstance(criterion, CrossEntropyLoss):
            raise NotImplementedError("GraphedStep does not record convkan_amd.CrossEntropyLoss yet: keep torch's criterion in a recorded step")
        if optimizer is not None and not (isinstance(optimizer, FusedAdamW) and optimizer.capturable):
            raise ValueError("GraphedStep(optimizer=...) records only a convkan_amd FusedAdamW(capturable=True); step any other optimizer after each call")
        if not example_data.is_cuda:
            raise ValueError("GraphedStep needs device tensors")
        self.model = model
        self.optimizer = optimizer
        self.criterion = criterion if criterion is not None else nn.CrossEntropyLoss()
        self.data, self.target = example_data.clone(), example_target.clone()
        saved = optimizer.snapshot() if optimizer is not None else None
        side = torch.cuda.Stream(device=example_data.device)
        side.wait_stream(torch.cuda.current_stream(example_data.device))
        with torch.cuda.stream(side), _split_context(split_precision):      # warm-up off the capture stream: plans, workspaces, torch's lazy initialisations
            for _ in range(max(1, warmup)):
                self._eager()
            if optimizer is not None:                      # (the warm-up uploaded lr; the recording below must find it on the device)
                optimizer.restore(saved)
        torch.cuda.current_stream(example_data.device).wait_stream(side)
        del saved
        self.graph = torch.cuda.CUDAGraph()
        self.model.zero_grad(set_to_none=True)             # recorded backward then ASSIGNS the gradients (tensors of the graph's pool)
        with _split_context(split_precision), ops.always_pack(), torch.cuda.graph(self.graph):
            self.loss = self._eager()
        self._captured = optimizer.captured_addresses() if optimizer is not None else None

    def _eager(self) -> torch.Tensor:
        self.model.zero_grad(set_to_none=True)
        loss = self.criterion(self.model(self.data), self.target)
        loss.backward()
        if self.optimizer is not None:
            self.optimizer.step()
        return loss.detach()

    def __call__(self, data: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if data.shape != self.data.shape or target.shape != self.target.shape:
            raise ValueError(f"GraphedStep was recorded for {tuple(self.data.shape)} / {tuple(self.target.shape)}, got {tuple(data.shape)} / {tuple(target.shape)}")
        self.data.copy_(data, non_blocking=True)
        self.target.copy_(target, non_blocking=True)
        if self.optimizer is not None:
            self.optimizer.sync_hyper()
        self.graph.replay()
        if self.optimizer is not None:
            self.optimizer.after_replay(self._captured)
        return self.loss


class _BatchRunner:
    """One training batch for the drivers below: ``train_step``, or -- ``graphed`` -- ONE ``GraphedStep(optimizer=...)`` recorded on the first batch
    (taken as the full-size one) and replayed for every batch of that shape; any other shape (the ragged last batch) goes through eager
    ``train_step`` with the same optimizer."""

    def __init__(self, model, optimizer, criterion, reducer, split_precision, graphed):
        if graphed:
            if not (isinstance(optimizer, FusedAdamW) and optimizer.capturable):
                raise ValueError("graphed=True needs a convkan_amd FusedAdamW(capturable=True)")
            if reducer is not None:
                raise ValueError("graphed=True: a reducer inside a recorded step is not built")
        self.model, self.optimizer, self.criterion, self.reducer, self.split, self.graphed = model, optimizer, criterion, reducer, split_precision, graphed
        self.step = None

    def __call__(self, data: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self.graphed:
            if self.step is None:
                self.step = GraphedStep(self.model, data, target, self.criterion, split_precision=self.split, optimizer=self.optimizer)
            if data.shape == self.step.data.shape and target.shape == self.step.target.shape:
                return self.step(data, target)
        return train_step(self.model, data, target, self.optimizer, self.criterion, self.reducer, self.split)


def train_model_generic(model: nn.Module, train_batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], device="cuda",
                        learning_rate: float = 1e-3, weight_decay: float = 1e-4, gamma: float = 0.8, epochs: int = 15,
                        reducer=None, split_precision: bool = False, graphed: bool = False, max_grad_norm=None,
                        skip_nonfinite: bool = False, accumulate_steps: int = 1) -> List[float]:
    """generic_train.py:19-30 without the dataset / metric / checkpoint plumbing; returns the average loss per epoch.
    ``train_batches`` is re-iterated every epoch (a list of (data, target) pairs or a DataLoader).  ``split_precision``: handed to every ``train_step``.
    ``graphed``: the optimizer is a capturable ``FusedAdamW`` and the whole step of every full-size batch is one graph replay (``_BatchRunner``).
    ``max_grad_norm``: None (off), or the global-norm clip the reference asks for at evaluations.py:33, done inside the optimizer step.
    ``skip_nonfinite``: sets ``FusedAdamW.skip_nonfinite`` (needs ``graphed=True``: ValueError otherwise) -- a step whose gradients hold an inf or a
    NaN changes nothing; the guard's counters are read with the epoch's loss, and an epoch that skipped steps issues ONE ``warnings.warn`` with the
    count and the parameter indices.
    ``accumulate_steps``: sets ``FusedAdamW.accumulate_steps`` before anything is recorded -- every batch is a micro-batch and every k-th one
    updates with the mean gradient, graphed or not.  The losses averaged per epoch stay the micro-batches' losses; a window left open at the end of
    an epoch carries into the next one (the scheduler moves lr between its micro-steps, and the update uses the lr of its boundary call); one left
    open at the very end is dropped with the optimizer.  With a ``reducer`` every micro-step still all-reduces: correct, but wasteful."""
    if skip_nonfinite and not graphed:
        raise ValueError("skip_nonfinite=True needs graphed=True (a capturable FusedAdamW)")
    model.to(device).train()
    optimizer = FusedAdamW(model.parameters(), lr=learning_rate, weight_decay=weight_decay, capturable=graphed, max_grad_norm=max_grad_norm)
    optimizer.skip_nonfinite = bool(skip_nonfinite)
    optimizer.accumulate_steps = accumulate_steps
    scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=gamma)
    criterion = nn.CrossEntropyLoss()
    run = _BatchRunner(model, optimizer, criterion, reducer, split_precision, graphed)
    history, skipped_before = [], 0
    for epoch in range(epochs):
        total, n = torch.zeros((), device=device), 0
        for data, target in train_batches:
            total += run(data.to(device), target.to(device))
            n += 1
        history.append(float(total) / max(n, 1))
        if skip_nonfinite:
            report = optimizer.guard_report()
            if report["skipped_steps"] > skipped_before:
                warnings.warn(f"epoch {epoch}: {report['skipped_steps'] - skipped_before} of {n} optimizer steps were skipped for non-finite "
                              f"gradients (last one: step {report['last_skipped']}, parameters {report['nonfinite_params']})", RuntimeWarning)
            skipped_before = report["skipped_steps"]
        scheduler.step()
    return history


def evaluate(model: nn.Module, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], device="cuda", metrics=None) -> dict:
    """evaluations.py:81-153 (``test``) without its per-batch host reads: the model in ``eval()`` mode under ``no_grad``, one
    ``ops.cross_entropy(model(data), target, metrics)`` per batch -- loss, torch.max's prediction and the per-class counts stay on the device --
    and ONE read at the end.  Returns ``ClassMetrics.result()``: loss (the mean of the batch means, evaluations.py:150), accuracy, macro
    precision / recall / f1 (scikit-learn's, ``zero_division=0``), samples, batches.  ``metrics``: a ``ClassMetrics`` to reuse (it is reset
    first); by default one is made for the width of the first batch's logits.  The model's training mode is restored.  Inference timing is not
    carried over."""
    from . import ops
    from .loss import ClassMetrics
    was_training = model.training
    model.eval()
    if metrics is not None:
        metrics.reset()
    try:
        with torch.no_grad():
            for data, target in batches:
                out = model(data.to(device))
                if metrics is None:
                    metrics = ClassMetrics(out.shape[1], out.device)
                ops.cross_entropy(out, target.to(device), metrics)
    finally:
        model.train(was_training)
    if metrics is None:
        raise ValueError("evaluate: no batches")
    return metrics.result()


def train_and_test_models(model: nn.Module, train_batches: Iterable[Tuple[torch.Tensor, torch.Tensor]],
                          test_batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], optimizer: torch.optim.Optimizer, scheduler=None,
                          epochs: int = 15, reducer=None, split_precision: bool = False, criterion: Optional[nn.Module] = None,
                          graphed: bool = False):
    """evaluations.py:156-247: per epoch the ``train_step`` loop (one read of the accumulated loss), then ``evaluate`` (one read of the
    counters), then ``scheduler.step()``.  Runs on the device the model is on.  Returns the first seven lists of evaluations.py:247: train loss,
    test loss, accuracy, precision, recall, F1 and the learning rate each epoch started with.  Checkpoints (``torch.save``), early stopping
    (``patience``), plots and timing are not carried over.  ``graphed``: ``optimizer`` must be a ``FusedAdamW(capturable=True)``; every full-size
    training batch is then one replay of a recorded step, optimizer included (``_BatchRunner``), the evaluation stays eager.  The optimizer is the
    caller's: set ``optimizer.skip_nonfinite = True`` before the call for guarded steps, and read ``optimizer.guard_report()`` after it; set
    ``optimizer.accumulate_steps = k`` before the call for accumulation (a window left open at the end of an epoch carries into the next)."""
    device = next(model.parameters()).device
    run = _BatchRunner(model, optimizer, criterion, reducer, split_precision, graphed)
    train_loss, test_loss, accuracy, precision, recall, f1, rates = [], [], [], [], [], [], []
    for _ in range(epochs):
        rates.append(optimizer.param_groups[0]["lr"])
        model.train()
        total, n = torch.zeros((), device=device), 0
        for data, target in train_batches:
            total += run(data.to(device), target.to(device))
            n += 1
        train_loss.append(float(total) / max(n, 1))
        r = evaluate(model, test_batches, device)
        for history, key in ((test_loss, "loss"), (accuracy, "accuracy"), (precision, "precision"), (recall, "recall"), (f1, "f1")):
            history.append(r[key])
        if scheduler is not None:
            scheduler.step()
    return train_loss, test_loss, accuracy, precision, recall, f1, rates

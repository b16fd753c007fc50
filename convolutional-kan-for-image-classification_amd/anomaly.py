"""Device-side anomaly mode: which layer first produced a NaN or an inf -- SURVEY.md section 5 ("NaN-checks kernel outputs").

The reference trains under ``torch.autograd.set_detect_anomaly(True)`` (train.py:431), which names the op that first produced a NaN by checking
every backward output on the HOST.  Here the training loop runs without a host read per step (``DeviceBatches`` -> ``GraphedStep(optimizer=...)``),
so the check is a counter in device memory: ``AnomalyProbe`` hangs one ``ops.count_nonfinite`` launch (csrc/kan_guard.hip, HBM-bound, one read of
the tensor) behind the output of every HIP layer and behind the gradient of that output, all adding to ONE int64 buffer, and ``report()`` reads that
buffer once, when asked.  Attached before ``GraphedStep(...)`` is built, the launches are recorded with the step and every replay counts.

It only reads.  Outputs are seen by forward hooks, their gradients by ``Tensor.register_hook`` on those outputs -- no node enters the autograd
graph, ``needs_input_grad``, ``ops.GRAD_SINKS`` and the first layer's skipped input gradient stay as they are, and loss, logits and gradients are
bit for bit those of the model without a probe.  OPT-IN: a model without a probe launches nothing of this.

    probe = AnomalyProbe(model)                        # before GraphedStep(...) is built
    step = GraphedStep(model, data, target, optimizer=opt)
    probe.reset()                                      # forget the warm-up: the next forward is tick 1
    for data, target in batches:
        step(data, target)
    for e in probe.report():                           # ONE host read; entry 0 is where the trouble was born
        print(e["name"], e["direction"], e["elements"], e["first_tick"], e["last_tick"])

The guard that keeps such a step from poisoning the parameters is ``FusedAdamW.skip_nonfinite``.  BatchNorm running statistics are updated in the
forward, before any probe or guard can know: a non-finite batch still poisons them, as in torch.
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn

from . import _lib as L
from . import ops

ROOT_NAME = "<output>"       # the slot pair of the root module's output
_EXTRA = 16                  # named slots ``check()`` may add: the buffer is allocated once, so that a recorded launch keeps its address


def _hip_layer_types():
    from .layers.conv_layers import _HipLayer
    from .layers.head_layers import _CoeffKANLayer
    from .layers.mlp_layers import KANLayer
    return (_HipLayer, KANLayer, _CoeffKANLayer)


def _first_tensor(out):
    if isinstance(out, torch.Tensor):
        return out
    if isinstance(out, (tuple, list)):
        for o in out:
            if isinstance(o, torch.Tensor):
                return o
    return None


class AnomalyProbe:
    """Counts non-finite values behind every HIP layer of ``model`` (every ``_HipLayer`` subclass, ``KANLayer``, the ``_CoeffKANLayer`` heads; in
    ``named_modules()`` order) and behind the model's own output (``"<output>"``): a "forward" slot for the output and -- ``backward=True`` -- a
    "backward" slot for the gradient that reaches that output.  A tick counts the forwards of the root module (a forward pre-hook adds 1 on the
    device, recordable); each slot keeps its element count and the first and last tick at which it saw something.

    ``slots``     the (name, direction) pairs, in buffer order
    ``check(t, name)``  count ``t`` into a named "forward" slot of its own (the loss, for instance); at most 16 names
    ``report()``  the ONLY host read: the slots with a non-zero count as dicts (name, direction, elements, first_tick, last_tick), sorted by
                  first_tick; within a tick forward slots come first, in module order, then backward slots in REVERSE module order -- the order
                  in which a step runs them -- so entry 0 is where the first non-finite value appeared
    ``reset()``   zero the tick and every record (after the warm-up of a ``GraphedStep``, for instance)
    ``remove()``  take the hooks off; also the exit of ``with AnomalyProbe(model) as probe:``
    A ``no_grad`` forward registers no gradient hook.  The buffer lives on the device of the model's first parameter."""

    def __init__(self, model: nn.Module, backward: bool = True):
        self.model, self.backward = model, bool(backward)
        kinds = _hip_layer_types()
        layers = [(name, m) for name, m in model.named_modules() if isinstance(m, kinds) and name != ""] + [(ROOT_NAME, model)]
        self.slots: List[tuple] = []
        self._order = {}                                       # slot index -> position of its module in forward order
        for pos, (name, _) in enumerate(layers):
            for direction in ("forward", "backward"):
                self._order[len(self.slots)] = pos
                self.slots.append((name, direction))
        self._fixed, self._named = len(self.slots), {}
        first = next(model.parameters(), None)
        self.buffer = torch.zeros(1 + 3 * (self._fixed + _EXTRA), dtype=torch.int64, device=first.device if first is not None else "cpu")
        self._handles = [model.register_forward_pre_hook(self._advance)]
        for pos, (_, m) in enumerate(layers):
            self._handles.append(m.register_forward_hook(self._make_hook(2 * pos)))

    # ------------------------------------------------------------------ the buffer: [tick, then 3 words per slot]
    @property
    def tick(self) -> torch.Tensor:
        return self.buffer[0:1]

    def _record(self, slot: int) -> torch.Tensor:
        return self.buffer[1 + 3 * slot:4 + 3 * slot]

    def _count(self, t: torch.Tensor, slot: int) -> None:
        if t.device != self.buffer.device and t.is_cuda:
            raise L.KanConvError(f"AnomalyProbe: its buffer is on {self.buffer.device}, the tensor on {t.device}; build the probe after model.to(device)")
        ops.count_nonfinite(t, self._record(slot), self.tick)

    # ------------------------------------------------------------------ hooks
    def _advance(self, module, args):
        self.tick.add_(1)                                      # one small launch on the current stream: recorded with the step

    def _make_hook(self, slot: int):
        def hook(module, args, out):
            t = _first_tensor(out)
            if t is None:
                return
            self._count(t, slot)
            if self.backward and torch.is_grad_enabled() and t.requires_grad:
                t.register_hook(lambda g: self._count(g, slot + 1))      # returns None: the gradient goes on unchanged
        return hook

    # ------------------------------------------------------------------ the public surface
    def check(self, tensor: torch.Tensor, name: str) -> None:
        """Count ``tensor`` into the "forward" slot called ``name`` (made at the first call with that name)."""
        slot = self._named.get(name)
        if slot is None:
            if len(self._named) == _EXTRA:
                raise L.KanConvError(f"AnomalyProbe.check: at most {_EXTRA} named slots")
            slot = self._named[name] = len(self.slots)
            self._order[slot] = slot                           # behind every module, in the order of their first call
            self.slots.append((name, "forward"))
        self._count(tensor, slot)

    def report(self) -> List[dict]:
        words = self.buffer.tolist()                           # the one host read
        found = []
        for slot, (name, direction) in enumerate(self.slots):
            elements, first, last = words[1 + 3 * slot:4 + 3 * slot]
            if elements:
                fwd = direction == "forward"
                found.append(((first, 0 if fwd else 1, self._order[slot] if fwd else -self._order[slot]),
                              dict(name=name, direction=direction, elements=elements, first_tick=first, last_tick=last)))
        return [entry for _, entry in sorted(found, key=lambda f: f[0])]

    def reset(self) -> None:
        self.buffer.zero_()

    def remove(self) -> None:
        for h in self._handles:
            h.remove()
        self._handles = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.remove()
        return False

"""Fused AdamW step over flat parameter blocks -- SURVEY.md section 8(f) rank 4 (the step right after the hot path).

The reference trains with ``optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)`` + ``ExponentialLR``
(generic_train.py:24-25), stepped once per batch (evaluations.py: train()).  torch walks the parameter list; here every
parameter group lives in ONE flat fp32 block (parameters, exp_avg, exp_avg_sq; the parameters are views into it) and a
step is one launch of ``kan_adamw_step_segments`` per group, which reads every gradient where autograd -- or the DP
reducer's all-reduce bucket -- left it (a device table of gradient addresses, re-uploaded only when an address changes).
Nothing is copied, zeroed or accumulated per step: 28 bytes of HBM traffic per element, 2.3 GB = ~0.3 ms at the HBM
roofline for KAN-VGG11's 83 M parameters.

It is a ``torch.optim.Optimizer``: ``param_groups`` / ``lr`` schedulers (ExponentialLR), ``state_dict`` /
``load_state_dict`` (per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq`` entries, as torch's AdamW stores them) and
``zero_grad`` (torch's own: gradients set to None) work as usual.  The update itself has no CPU path: ``step()`` on CPU parameters raises.

``capturable=True`` keeps what changes between steps on the DEVICE -- ``lr`` (a float64 scalar per group) and one int32 step count per
parameter -- so that ``step()`` may be recorded into a HIP graph (``train.GraphedStep(..., optimizer=opt)``) and a replay computes the next
step, as ``torch.optim.AdamW(capturable=True)`` does.  A step is then two launches per group, ``kan_adamw_advance`` (the counts of the
parameters that have a gradient) and ``kan_adamw_step_segments_dev``; the host keeps no count and reads the device ones only for
``state_dict()`` / ``sync_steps()``.  See ``FusedAdamW.step`` for what a recording freezes.

``max_grad_norm=c`` (default None: off) clips by the global gradient norm inside the step -- what the reference asks for at evaluations.py:33
(``clip_grad_norm_(model.parameters(), max_norm=1.0)``) -- without a host walk or an in-place rescaling pass: ``kan_grad_sqnorm_chunks`` per group
and one ``kan_grad_norm_finish`` leave the norm and ``min(1, c / (norm + 1e-6))`` in device memory, and the ``_clip`` step kernels multiply by that
coefficient as they read each gradient (32 bytes per element instead of 28; ``p.grad`` itself is not modified).  ``opt.grad_norm``,
``opt.clip_scale`` and ``opt.grad_norms()`` (the per-parameter norms of evaluations.py:66-71) are device reads.  It works in both modes and inside
a recorded step.

``opt.skip_nonfinite = True`` (default False; ``capturable=True`` only) guards the step: the same statistics pass runs, with or without clipping,
and one ``kan_adamw_guard`` launch decides ON THE DEVICE whether any gradient holds an inf or a NaN; if so the step kernels are handed an
all-zero address table and touch no parameter, no moment and no step count.  ``opt.last_step_skipped`` / ``opt.skipped_steps`` are device views,
``opt.guard_report()`` is one read.  The watchdog the reference keeps on the host (train.py:431); ``AnomalyProbe`` says where the value was born.

``opt.accumulate_steps = k`` (default 1: nothing changes) makes every ``step()`` call a MICRO-step of a window of k: ``kan_grad_accumulate`` per group
adds the gradients into a flat fp32 accumulator row (the first call of a window overwrites it, the last one turns the sum into the mean), one
``kan_accum_gate`` moves the window's counter, and the unchanged statistics / guard / advance / step kernels read a GATED address table -- the
accumulator addresses on the k-th call, zeros otherwise.  ``capturable=True`` keeps the counter on the device, so a recorded step is ONE graph
replayed per micro-batch and every k-th replay updates; the classic mode counts on the host.  The reference's loop (evaluations.py:44-72) has no
accumulation; k micro-batches give the update k data-parallel ranks compute (mean of the shard gradients, one step).
"""
from __future__ import annotations

import ctypes as C
from typing import List

import torch

from . import _lib as L

_ALIGN = 64          # elements: every parameter starts on a 256-byte boundary of the flat block
_CHUNK = 8192        # elements per workgroup of the segment kernel (256 threads x 8 float4)


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, capturable: bool = False,
                 max_grad_norm=None):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid AdamW hyper-parameters")
        self.capturable = bool(capturable)           # not a param_groups entry: a state_dict must load into torch.optim.AdamW on any device
        self._captured = None
        self._max_grad_norm = self._check_max_norm(max_grad_norm)     # like capturable, not a param_groups entry
        self._clip = None
        self._skip_nonfinite = False                 # a settable attribute, not a keyword: see skip_nonfinite
        self._guard = None
        self._accum_k = 1                            # a settable attribute, not a keyword: see accumulate_steps
        self._accum = None
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._flat = []
        for group in self.param_groups:
            self._flat.append(self._flatten(group))
        if self._max_grad_norm is not None:
            self._clip = self._build_clip()

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_flat"):                   # groups added after construction get their own flat block
            self._flat.append(self._flatten(self.param_groups[-1]))
            if self._clip is not None:               # a new layout: the statistics buffer is rebuilt with it
                self._clip = self._build_clip()
            if self._guard is not None:              # and the guard's tables; the counters carry over
                self._guard = self._build_guard(self._guard)
            if self._accum is not None:              # and the accumulators: a new layout starts a fresh window
                self._accum = self._build_accum(self._accum_k)

    # ------------------------------------------------------------------ layout
    @staticmethod
    def _flatten(group):
        ps: List[torch.nn.Parameter] = [p for p in group["params"] if p.requires_grad]
        if not ps:
            return None
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or p.device != dev:
                raise L.KanConvError("FusedAdamW needs float32 parameters on one device per group")
        offs, n = [], 0
        for p in ps:
            offs.append(n)
            n += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        blk = torch.zeros((3, n), dtype=torch.float32, device=dev)          # rows: parameters, exp_avg, exp_avg_sq
        views = []
        with torch.no_grad():
            for p, o in zip(ps, offs):
                pv, mv, vv = (blk[r, o:o + p.numel()].view_as(p) for r in range(3))
                pv.copy_(p.data)
                p.data = pv
                views.append((pv, mv, vv))
        # chunk table of kan_adamw_step_segments: workgroup b -> (segment, first element); built once per layout
        seg, start = [], []
        for i, p in enumerate(ps):
            for s0 in range(0, p.numel(), _CHUNK):
                seg.append(i); start.append(s0)
        tab = dict(seg_off=torch.tensor(offs, dtype=torch.int64, device=dev), seg_n=torch.tensor([p.numel() for p in ps], dtype=torch.int32, device=dev),
                   chunk_seg=torch.tensor(seg, dtype=torch.int32, device=dev), chunk_start=torch.tensor(start, dtype=torch.int32, device=dev),
                   seg_grad=torch.zeros(len(ps), dtype=torch.int64, device=dev), grad_ptrs=None,
                   seg_bias=torch.zeros((len(ps), 2), dtype=torch.float32, device=dev),
                   seg_step=torch.zeros(len(ps), dtype=torch.int32, device=dev))           # capturable: the step counts live here
        group.setdefault("step", 0)
        return dict(params=ps, block=blk, views=views, n=n, tab=tab, steps=[0] * len(ps), index={id(p): i for i, p in enumerate(ps)},
                    lr_dev=torch.zeros(1, dtype=torch.float64, device=dev), lr_host=None)  # capturable: lr on the device, and what it holds

    def _link_state(self, group, flat):
        for p, (_, mv, vv) in zip(flat["params"], flat["views"]):
            st = self.state[p]
            st["step"] = torch.tensor(float(flat["steps"][flat["index"][id(p)]]))
            st["exp_avg"], st["exp_avg_sq"] = mv, vv

    # ------------------------------------------------------------------ clipping: the statistics buffer
    @staticmethod
    def _check_max_norm(value):
        if value is None:
            return None
        value = float(value)
        if not value >= 0.0:                                              # negative or NaN
            raise ValueError(f"max_grad_norm must be None or a float >= 0 (inf allowed), got {value}")
        return value

    @property
    def max_grad_norm(self):
        """None (no clipping: the step is the plain one) or the ``max_norm`` of ``clip_grad_norm_``.  Settable; the device copy follows like lr."""
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        self._max_grad_norm = self._check_max_norm(value)
        if self._max_grad_norm is not None and self._clip is None and hasattr(self, "_flat"):
            self._clip = self._build_clip()

    def _build_clip(self):
        """ONE buffer for everything the norm kernels write, built with the layout tables: partial (double, one per chunk over all groups), seg_sq
        (double, one per parameter), seg_first_chunk (int32, one per parameter + 1) and three floats (norm, scale, max_norm)."""
        flats = [f for f in self._flat if f is not None]
        dev = flats[0]["block"].device if flats else torch.device("cpu")
        if any(f["block"].device != dev for f in flats):
            raise L.KanConvError("FusedAdamW(max_grad_norm=...): one global norm needs every parameter group on one device")
        first, chunk0 = [0], []
        for f in self._flat:
            chunk0.append(first[-1])
            for p in (f["params"] if f is not None else ()):
                first.append(first[-1] + (p.numel() + _CHUNK - 1) // _CHUNK)
        nc, ns = first[-1], len(first) - 1
        words = (ns + 2) // 2                                              # 8-byte words holding the ns + 1 int32
        buf = torch.zeros(nc + ns + words + 2, dtype=torch.float64, device=dev)
        ints = buf[nc + ns:nc + ns + words].view(torch.int32)[:ns + 1]
        ints.copy_(torch.tensor(first, dtype=torch.int32))
        return dict(buf=buf, partial=buf[:nc], seg_sq=buf[nc:nc + ns], seg_first_chunk=ints, out=buf[nc + ns + words:].view(torch.float32)[:3],
                    chunk0=chunk0, host=None)                              # host: what out[2], the device copy of max_grad_norm, holds

    def _need_clip(self, what):
        if self._max_grad_norm is None or self._clip is None:
            raise L.KanConvError(f"FusedAdamW.{what} belongs to max_grad_norm=...: this optimizer does not clip (max_grad_norm=None)")
        return self._clip

    @property
    def grad_norm(self):
        """0-dim float32 DEVICE tensor: the global norm, before clipping, of the gradients the last step (or replay) consumed.  A view of the
        statistics buffer: no host read, and the next step overwrites it (like ``GraphedStep.loss``)."""
        return self._need_clip("grad_norm")["out"][0]

    @property
    def clip_scale(self):
        """0-dim float32 DEVICE tensor: min(1, max_grad_norm / (grad_norm + 1e-6)), what the last step multiplied every gradient by."""
        return self._need_clip("clip_scale")["out"][1]

    def grad_norms(self):
        """float32 DEVICE vector: the gradient norm of every parameter that has ``requires_grad``, in ``param_groups`` order, as of the last step;
        0 where there was no gradient.  No host read."""
        return self._need_clip("grad_norms()")["seg_sq"].sqrt().float()

    def _sync_max_norm(self, clip):
        if clip["host"] != self._max_grad_norm:
            if torch.cuda.is_current_stream_capturing():
                raise L.KanConvError(f"FusedAdamW(max_grad_norm=...): the device copy of max_grad_norm holds {clip['host']}, the attribute is "
                                     f"{self._max_grad_norm}; nothing may be uploaded while the stream is capturing -- run one eager step, or call "
                                     "sync_hyper(), before recording")
            clip["out"][2:3].fill_(self._max_grad_norm)                    # a fill launch carrying the value: no host memory is read later
            clip["host"] = self._max_grad_norm

    def _launch_norm(self, lib, clip, work, src=None):
        """The first pass of a clipping (or guarded) step: every group's address table, one chunk launch per group, one finish.  ``src``: None, or
        per group the table to read instead of ``seg_grad`` (the gated tables of an accumulating step, which filled ``seg_grad`` already)."""
        if self.capturable:
            for _, group, flat, _, _ in work:                              # refuse a stale lr before anything is launched
                self._sync_lr(group, flat)
        if clip is self._clip:                                             # (the guard's own statistics buffer holds max_norm = inf for good)
            self._sync_max_norm(clip)
        dev = clip["buf"].device
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            for _, _, flat, ptrs, _ in work:
                if src is None:
                    self._fill_table(lib, flat, ptrs)
            if len(work) != sum(f is not None for f in self._flat):        # a group without any gradient launches nothing: its partials are 0
                clip["partial"].zero_()
            for gi, _, flat, _, _ in work:
                tab, c0 = flat["tab"], clip["chunk0"][gi]
                L.check(lib.kan_grad_sqnorm_chunks(C.c_void_p((tab["seg_grad"] if src is None else src[gi]).data_ptr()), C.c_void_p(tab["seg_n"].data_ptr()),
                                                   C.c_void_p(tab["chunk_seg"].data_ptr()), C.c_void_p(tab["chunk_start"].data_ptr()),
                                                   tab["chunk_seg"].numel(), _CHUNK, C.c_void_p(clip["partial"].data_ptr() + 8 * c0), stream),
                        "kan_grad_sqnorm_chunks")
            L.check(lib.kan_grad_norm_finish(C.c_void_p(clip["partial"].data_ptr()), C.c_void_p(clip["seg_first_chunk"].data_ptr()),
                                             clip["seg_sq"].numel(), C.c_void_p(clip["out"].data_ptr() + 8), C.c_void_p(clip["seg_sq"].data_ptr()),
                                             C.c_void_p(clip["out"].data_ptr()), stream), "kan_grad_norm_finish")

    # ------------------------------------------------------------------ the non-finite guard
    @property
    def skip_nonfinite(self):
        """False (default: an inf or NaN gradient poisons what torch's ``error_if_nonfinite=False`` path poisons, and the launches are the ones
        described under ``step``) or True: a step whose gradients hold an inf or a NaN leaves every parameter, both moments and every step count
        alone.  Settable, like ``max_grad_norm``; needs ``capturable=True`` (the classic mode counts steps on the host and could not know about a
        skip without a read: ValueError) and every parameter group on one device.  A recorded step freezes whether it is on."""
        return self._skip_nonfinite

    @skip_nonfinite.setter
    def skip_nonfinite(self, value):
        value = bool(value)
        if value and not self.capturable:
            raise ValueError("FusedAdamW.skip_nonfinite needs capturable=True: the classic step counts on the host and cannot skip without a read")
        if value and self._guard is None:
            self._guard = self._build_guard()
        self._skip_nonfinite = value

    def _build_guard(self, old=None):
        """Everything the guard owns, apart from ``_clip`` and the flat blocks (whose layouts stay as they are): a statistics buffer of its own for
        the steps that do not clip (``_build_clip``'s, with max_norm = inf), and ONE int64 buffer holding the five counters, one flag per
        parameter, the group descriptors of ``kan_adamw_guard`` and a masked copy of every group's gradient address table."""
        stats = self._build_clip()                                         # (refuses groups on several devices)
        dev = stats["buf"].device
        stats["out"][2:3].fill_(float("inf"))
        stats["host"] = float("inf")
        ns, live = stats["seg_sq"].numel(), [f for f in self._flat if f is not None]
        buf = torch.zeros(5 + ns + 3 * len(live) + ns, dtype=torch.int64, device=dev)
        at, desc, masked = 5 + ns + 3 * len(live), [], []
        for f in self._flat:
            if f is None:
                masked.append(None)
                continue
            n = len(f["params"])
            masked.append(buf[at:at + n])
            desc += [f["tab"]["seg_grad"].data_ptr(), masked[-1].data_ptr(), n]
            at += n
        groups = buf[5 + ns:5 + ns + 3 * len(live)]
        if desc:
            groups.copy_(torch.tensor(desc, dtype=torch.int64))
        if old is not None:
            buf[:5].copy_(old["counters"])
        return dict(stats=stats, buf=buf, counters=buf[:5], flags=buf[5:5 + ns], groups=groups, masked=masked, n_groups=len(live))

    def _need_guard(self, what):
        if self._guard is None:
            raise L.KanConvError(f"FusedAdamW.{what} belongs to skip_nonfinite = True: this optimizer has never been guarded")
        return self._guard

    @property
    def last_step_skipped(self):
        """0-dim int64 DEVICE view: 1 if the last guarded step (or replay) was skipped, else 0.  No host read."""
        return self._need_guard("last_step_skipped")["counters"][4]

    @property
    def skipped_steps(self):
        """0-dim int64 DEVICE view: how many guarded steps were skipped since the counters were last cleared.  No host read."""
        return self._need_guard("skipped_steps")["counters"][1]

    def guard_report(self):
        """ONE host read of the guard's counters: ``guarded_steps``, ``skipped_steps``, ``first_skipped`` / ``last_skipped`` (the ordinal, counting
        guarded steps from 1, of the first / last skipped one; None if none) and ``nonfinite_params``: the parameters whose gradient held an inf
        or a NaN in the LAST skipped step, as indices into the parameters that have ``requires_grad``, in ``param_groups`` order (the indexing of
        ``grad_norms()``)."""
        g = self._need_guard("guard_report()")
        words = g["buf"][:5 + g["flags"].numel()].tolist()
        guarded, skipped, first, last = words[:4]
        return dict(guarded_steps=guarded, skipped_steps=skipped, first_skipped=first if skipped else None, last_skipped=last if skipped else None,
                    nonfinite_params=[i for i, f in enumerate(words[5:]) if f] if skipped else [])

    def reset_guard(self):
        """Clear the guard's counters and flags (one small launch)."""
        g = self._need_guard("reset_guard()")
        g["buf"][:5 + g["flags"].numel()].zero_()

    def _launch_guard(self, lib, stats, groups=None):
        """``groups``: None, or the descriptors to use instead of the guard's own (an accumulating step: the gated tables are the source it masks)."""
        g = self._guard
        with torch.cuda.device(g["buf"].device):
            L.check(lib.kan_adamw_guard(C.c_void_p(stats["seg_sq"].data_ptr()), stats["seg_sq"].numel(),
                                        C.c_void_p((g["groups"] if groups is None else groups).data_ptr()),
                                        g["n_groups"], C.c_void_p(g["counters"].data_ptr()), C.c_void_p(g["flags"].data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream(g["buf"].device).cuda_stream)), "kan_adamw_guard")

    # ------------------------------------------------------------------ gradient accumulation
    @property
    def accumulate_steps(self):
        """1 (default: every ``step()`` call is a step, nothing is allocated and the launches are the ones described under ``step``) or k > 1: every
        ``step()`` call is micro-step m of a window of k, and only the k-th applies an update -- ONE AdamW step with the MEAN of the k gradients.
        Settable, like ``skip_nonfinite``; not a constructor keyword and not a ``param_groups`` entry (a ``state_dict`` keeps loading into
        ``torch.optim.AdamW``).  Anything but an int >= 1: ValueError.  Changing it inside an open window (``micro_step != 0``; see
        ``reset_accumulation()``) or while the stream is capturing: ``KanConvError``.  k is a kernel argument: a recorded step freezes it.

        Inside a window ``max_grad_norm`` clips by the norm of the MEAN (``grad_norm`` reads 0 and ``clip_scale`` 1 after a call that is no
        boundary; ``p.grad`` is never modified), the guard skips the window's update if ANY micro-gradient was non-finite (the first call of the
        next window overwrites the accumulator: nothing leaks), a parameter without a gradient in the whole window is skipped as torch skips it, and
        step counts advance once per window.  ``state_dict()`` is unchanged: an OPEN WINDOW IS NOT CHECKPOINTED -- save on a boundary, or the
        micro-steps of the open window are lost on resume.  ``snapshot()`` / ``restore()`` do cover it."""
        return self._accum_k

    @accumulate_steps.setter
    def accumulate_steps(self, value):
        if isinstance(value, bool) or not isinstance(value, int) or value < 1:
            raise ValueError(f"FusedAdamW.accumulate_steps must be an int >= 1, got {value!r}")
        if value == self._accum_k:
            return
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise L.KanConvError("FusedAdamW.accumulate_steps cannot change while the stream is capturing: set it before recording")
        if self.micro_step != 0:
            raise L.KanConvError(f"FusedAdamW.accumulate_steps cannot change inside an open window (micro_step = {self.micro_step} of "
                                 f"{self._accum_k}): finish the window or call reset_accumulation()")
        self._accum = self._build_accum(value) if value > 1 and hasattr(self, "_flat") else None
        self._accum_k = value

    def _build_accum(self, k):
        """Everything accumulation owns (the flat blocks and their tables stay as they are): per group ONE fp32 accumulator row with the layout of
        the flat block, and ONE int64 buffer holding the window's state -- the counter (int32, word 0) and one int32 ``seen`` flag per parameter --,
        then the group descriptors of ``kan_accum_gate``, per group the table of accumulator addresses and the gated table."""
        live = [f for f in self._flat if f is not None]
        dev = live[0]["block"].device if live else torch.device("cpu")
        if any(f["block"].device != dev for f in live):
            raise L.KanConvError("FusedAdamW.accumulate_steps: one window counter needs every parameter group on one device")
        ns = [0 if f is None else len(f["params"]) for f in self._flat]
        seen_words = [(n + 1) // 2 for n in ns]                            # int32 flags in 8-byte words: every table stays 8-byte aligned
        n_state = 1 + sum(seen_words)
        buf = torch.zeros(n_state + 4 * len(live) + 2 * sum(ns), dtype=torch.int64, device=dev)
        rows, seen, addr, gated, desc, addr_host = [], [], [], [], [], []
        at_seen, at = 1, n_state + 4 * len(live)
        for f, n, w in zip(self._flat, ns, seen_words):
            if f is None:
                rows.append(None); seen.append(None); addr.append(None); gated.append(None); addr_host.append(None)
                continue
            rows.append(torch.zeros(f["n"], dtype=torch.float32, device=dev))
            seen.append(buf[at_seen:at_seen + w].view(torch.int32)[:n])
            addr.append(buf[at:at + n]); gated.append(buf[at + n:at + 2 * n])
            addr_host.append([rows[-1].data_ptr() + 4 * o for o in f["tab"]["seg_off"].tolist()])       # (one read, at build time)
            addr[-1].copy_(torch.tensor(addr_host[-1], dtype=torch.int64))
            desc += [addr[-1].data_ptr(), gated[-1].data_ptr(), seen[-1].data_ptr(), n]
            at_seen, at = at_seen + w, at + 2 * n
        groups = buf[n_state:n_state + 4 * len(live)]
        if desc:
            groups.copy_(torch.tensor(desc, dtype=torch.int64))
        return dict(k=k, buf=buf, state=buf[:n_state], micro=buf[:1].view(torch.int32)[:1], rows=rows, seen=seen, addr=addr, gated=gated,
                    groups=groups, n_groups=len(live), addr_host=addr_host, micro_host=0, seen_host=[[False] * n for n in ns], gated_host=[None] * len(ns),
                    guard_groups=None)

    @property
    def micro_step(self):
        """The index m of the NEXT ``step()`` call within its window, an int in [0, accumulate_steps); 0 = no window is open.  ``capturable=True``:
        ONE device read (the counter lives on the device); it is never read on the step path."""
        if self._accum is None:
            return 0
        return int(self._accum["micro"].item()) if self.capturable else self._accum["micro_host"]

    def reset_accumulation(self):
        """Drop an open window: the next ``step()`` call is micro-step 0 and overwrites the accumulators.  Never while the stream is capturing."""
        if self._accum is None:
            return
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise L.KanConvError("FusedAdamW.reset_accumulation() while the stream is capturing: call it before recording")
        a = self._accum
        a["state"].zero_()
        a["micro_host"], a["seen_host"] = 0, [[False] * len(s) for s in a["seen_host"]]

    def _guard_groups(self, acc):
        """The guard's group descriptors with the gated tables as the source it masks (built once per guard layout)."""
        g = self._guard
        if acc["guard_groups"] is None or acc["guard_groups"][0] is not g:
            desc = []
            for gated, masked in zip(acc["gated"], g["masked"]):
                if gated is not None:
                    desc += [gated.data_ptr(), masked.data_ptr(), gated.numel()]
            acc["guard_groups"] = (g, torch.tensor(desc, dtype=torch.int64).to(g["buf"].device))
        return acc["guard_groups"][1]

    def _launch_accumulate(self, lib, acc, work, micro_dev, m):
        for gi, _, flat, ptrs, _ in work:
            tab = flat["tab"]
            with torch.cuda.device(flat["block"].device):
                self._fill_table(lib, flat, ptrs)
                L.check(lib.kan_grad_accumulate(C.c_void_p(acc["rows"][gi].data_ptr()), C.c_void_p(tab["seg_grad"].data_ptr()),
                                                C.c_void_p(tab["seg_off"].data_ptr()), C.c_void_p(tab["seg_n"].data_ptr()),
                                                C.c_void_p(tab["chunk_seg"].data_ptr()), C.c_void_p(tab["chunk_start"].data_ptr()),
                                                tab["chunk_seg"].numel(), _CHUNK, micro_dev, m, acc["k"], C.c_void_p(acc["seen"][gi].data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream(flat["block"].device).cuda_stream)), "kan_grad_accumulate")

    def _accumulate_capturable(self, lib, acc, work, guard):
        """Micro-step of the capturable mode: the accumulate launch of every group, then the gate.  The device decides what the launches behind it see."""
        for _, group, flat, _, _ in work:                                  # refuse a stale lr before anything is launched
            self._sync_lr(group, flat)
        if guard is not None:
            self._guard_groups(acc)                                        # (an upload: never between recorded launches)
        self._launch_accumulate(lib, acc, work, C.c_void_p(acc["micro"].data_ptr()), 0)
        dev = acc["buf"].device
        with torch.cuda.device(dev):
            L.check(lib.kan_accum_gate(C.c_void_p(acc["groups"].data_ptr()), acc["n_groups"], C.c_void_p(acc["micro"].data_ptr()), acc["k"],
                                       C.c_void_p(guard["counters"].data_ptr() if guard is not None else 0),
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "kan_accum_gate")

    def _accumulate_classic(self, lib, acc, work):
        """Micro-step of the classic mode: the host counts.  Inside a window only the accumulate kernel is launched (returns []); on the boundary
        the ordinary step is handed the accumulator addresses of the parameters the window saw, through the gated tables."""
        m, k = acc["micro_host"], acc["k"]
        self._launch_accumulate(lib, acc, work, None, m)
        for gi, _, _, ptrs, _ in work:
            acc["seen_host"][gi] = [s or bool(a) for s, a in zip(acc["seen_host"][gi], ptrs)]
        if m + 1 < k:
            acc["micro_host"] = m + 1
            return []
        out = []
        for gi, group, flat, _, keep in work:
            ptrs = [a if s else 0 for a, s in zip(acc["addr_host"][gi], acc["seen_host"][gi])]
            if ptrs != acc["gated_host"][gi]:                              # (the same parameters window after window: usually nothing)
                acc["gated"][gi].copy_(torch.tensor(ptrs, dtype=torch.int64), non_blocking=False)
                acc["gated_host"][gi] = ptrs
            if any(ptrs):
                out.append((gi, group, flat, ptrs, keep))
        acc["state"].zero_()                                               # the kernel's seen flags: the host keeps its own
        acc["micro_host"], acc["seen_host"] = 0, [[False] * len(s) for s in acc["seen_host"]]
        return out

    # ------------------------------------------------------------------ torch.optim surface
    @torch.no_grad()
    def step(self, closure=None):
        """One launch per parameter group; gradients are read where autograd (or the DP reducer's bucket) left them.

        ``capturable=True``: two launches per group and nothing read from or written to host memory on the way, so the call may run while the
        current stream is capturing.  A RECORDED step freezes (a) which parameters have a gradient and where those gradients live -- the addresses
        go into the graph through ``kan_set_u64_table`` nodes -- and (b) betas, eps and weight_decay, which are kernel arguments: changing one of
        them, or the set of parameters with a gradient, means recording again.  ``lr`` and the step counts are NOT frozen: they are read from
        device memory at replay time.  ``lr`` must already be on the device when recording starts (one eager step, or ``sync_hyper()``,
        after the last change of ``group["lr"]``); between replays call ``sync_hyper()`` -- ``GraphedStep`` does.

        ``max_grad_norm=c`` (default None: off, and the launches are the ones above): global-norm clipping as
        ``torch.nn.utils.clip_grad_norm_(params, c)`` in front of the step computes it, in two passes over the groups -- one
        ``kan_grad_sqnorm_chunks`` per group and ONE ``kan_grad_norm_finish`` (the norm is global, over all groups), then per group the ``_clip``
        variant of the step, which multiplies every gradient by the coefficient as it reads it.  Unlike ``clip_grad_norm_``, ``p.grad`` is NOT
        modified: the scale exists only inside the step.  ``opt.grad_norm``, ``opt.clip_scale`` and ``opt.grad_norms()`` are device reads of what
        the step computed.  Under DP the step runs after ``reducer.finish()``, so the norm is that of the REDUCED gradients (every rank computes
        the same one).  A recorded step freezes that clipping is on; the VALUE of ``max_grad_norm`` is NOT frozen -- it is read from device memory
        at replay time and brought up to date like ``lr``, by the eager step or by ``sync_hyper()``.  If no parameter has a gradient, nothing launches.

        ``skip_nonfinite = True`` (default False, and the launches are the ones above; capturable only): the two norm launches run whether or not
        the step clips, then ONE ``kan_adamw_guard`` -- it tests the exact double sum of squares of every parameter's gradient (non-finite exactly
        when the gradient holds an inf or a NaN; a finite gradient whose float32 norm overflows does NOT skip), counts, and writes per group a masked
        copy of the address table, zeros if the step is to be skipped -- and ``kan_adamw_advance`` and the step kernels read that copy: a skipped
        step changes no parameter, no moment and no step count.  One decision per step over all groups, taken from device memory: a recorded
        step decides anew at every replay.  On a skipped step ``grad_norm`` / ``clip_scale`` / ``grad_norms()`` show the non-finite values that
        caused it.  Version counters are bumped either way.  Under DP every rank sees the reduced gradients and decides alike.

        ``accumulate_steps = k`` (default 1, and the launches are the ones above): the call is a micro-step.  The address tables are filled as
        always, then ONE ``kan_grad_accumulate`` per group and -- capturable -- ONE ``kan_accum_gate``, and everything above runs unchanged on the
        GATED tables: the accumulator addresses on the k-th call, zeros (no parameter, moment or step count touched; ``grad_norm`` 0,
        ``clip_scale`` 1; neither a guarded nor a skipped step) on the others.  The classic mode counts on the host and launches only the
        accumulate kernel inside a window.  See ``accumulate_steps``."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.load()
        work = []
        for gi, (group, flat) in enumerate(zip(self.param_groups, self._flat)):
            if flat is None:
                continue
            blk = flat["block"]
            if not blk.is_cuda:
                raise L.KanConvError(f"FusedAdamW.step: parameters are on {blk.device}; the fused step runs only on a ROCm device "
                                     "(there is no CPU fallback)")
            ptrs, keep = [], []
            for p, (pv, _, _) in zip(flat["params"], flat["views"]):
                if p.data_ptr() != pv.data_ptr():
                    raise L.KanConvError("a parameter was re-allocated after FusedAdamW flattened it (call .to()/.cuda() before "
                                         "building the optimizer)")
                g = p.grad
                if g is None:
                    ptrs.append(0)                                         # torch skips parameters without a gradient
                    continue
                if g.dtype != torch.float32 or g.device != blk.device or not g.is_contiguous():
                    g = g.to(device=blk.device, dtype=torch.float32).contiguous()
                    keep.append(g)
                ptrs.append(g.data_ptr())
            if any(ptrs) or self._accum is not None:                       # an accumulating call runs every group: the window may hold its gradient
                work.append((gi, group, flat, ptrs, keep))
        clip = self._clip if self._max_grad_norm is not None else None
        guard = self._guard if self._skip_nonfinite and self.capturable else None
        acc = self._accum if work else None
        if acc is not None and not self.capturable:
            work = self._accumulate_classic(lib, acc, work)                # the boundary's work (accumulator addresses), or [] inside a window
            if not work and clip is not None:                              # no step: the statistics read what the capturable mode computes there,
                clip["out"][0:1].zero_()                                   # norm 0 and coefficient 1 (two fill launches, only when clipping)
                clip["out"][1:2].fill_(1.0)
        elif acc is not None:
            self._accumulate_capturable(lib, acc, work, guard)
        src = acc["gated"] if acc is not None else None                    # what everything below reads where it read seg_grad
        if guard is not None and work:
            stats = clip if clip is not None else guard["stats"]           # the statistics pass runs with or without clipping
            self._launch_norm(lib, stats, work, src)
            self._launch_guard(lib, stats, self._guard_groups(acc) if acc is not None else None)
        elif clip is not None and work:
            self._launch_norm(lib, clip, work, src)
        scale = C.c_void_p(clip["out"].data_ptr() + 4) if clip is not None else None
        for gi, group, flat, ptrs, _ in work:
            with torch.cuda.device(flat["block"].device):
                if self.capturable:
                    self._step_capturable(lib, group, flat, ptrs, scale, guard["masked"][gi] if guard is not None else src[gi] if acc is not None else None)
                else:
                    self._step_classic(lib, group, flat, ptrs, scale, src[gi] if acc is not None else None)
            for p, a in zip(flat["params"], ptrs):                         # the kernel wrote through raw pointers: tell autograd (and the packed-
                if a or (acc is not None and self.capturable):             # weight cache of ops.py) that the values changed.  Host-only, legal
                    torch.autograd.graph.increment_version(p)              # under capture; a replay bumps them in after_replay().  (A capturable
        del work                                                           # accumulating call does not know the boundary: it bumps every time.)
        return loss

    def _fill_table(self, lib, flat, ptrs):
        """The group's device table of gradient addresses: a copy when an address changed (the caching allocator hands back the same blocks step
        after step: usually nothing), or -- capturing, where no host-to-device copy is allowed -- by value, 64 per launch, as part of the graph."""
        tab = flat["tab"]
        if self.capturable and torch.cuda.is_current_stream_capturing():
            seg_grad, stream = C.c_void_p(tab["seg_grad"].data_ptr()), C.c_void_p(torch.cuda.current_stream(flat["block"].device).cuda_stream)
            vals = (C.c_ulonglong * 64)()
            for first in range(0, len(ptrs), 64):
                part = ptrs[first:first + 64]
                vals[:len(part)] = part
                L.check(lib.kan_set_u64_table(seg_grad, first, vals, len(part), stream), "kan_set_u64_table")
            tab["grad_ptrs"] = None                                        # the table holds these addresses only after a replay: after_replay()
            flat["captured_ptrs"] = list(ptrs)
        elif ptrs != tab["grad_ptrs"]:
            tab["seg_grad"].copy_(torch.tensor(ptrs, dtype=torch.int64), non_blocking=False)
            tab["grad_ptrs"] = ptrs

    def _step_classic(self, lib, group, flat, ptrs, scale, table=None):
        """``table``: None, or the device table that already holds ``ptrs`` (an accumulating step's gated table), read instead of ``seg_grad``."""
        blk, tab = flat["block"], flat["tab"]
        if scale is None and table is None:
            self._fill_table(lib, flat, ptrs)                              # (a clipping step filled every table in its first pass)
        b1, b2 = group["betas"]
        steps = flat["steps"]                                              # torch counts steps per parameter
        for i, a in enumerate(ptrs):
            steps[i] += 1 if a else 0
        group["step"] = max(steps)
        bias = None
        if any(a and st != group["step"] for a, st in zip(ptrs, steps)):   # rare: some parameter skipped earlier steps
            bias = tab["seg_bias"]
            bias.copy_(torch.tensor([[-group["lr"] / (1.0 - b1 ** max(st, 1)), 1.0 / (1.0 - b2 ** max(st, 1)) ** 0.5] for st in steps],
                                    dtype=torch.float32))
        row = lambda r: C.c_void_p(blk.data_ptr() + 4 * r * flat["n"])
        fn, name = (lib.kan_adamw_step_segments, "kan_adamw_step_segments") if scale is None else \
                   (lib.kan_adamw_step_segments_clip, "kan_adamw_step_segments_clip")
        L.check(fn(row(0), row(1), row(2), C.c_void_p((tab["seg_grad"] if table is None else table).data_ptr()), C.c_void_p(tab["seg_off"].data_ptr()),
                   C.c_void_p(tab["seg_n"].data_ptr()), C.c_void_p(tab["chunk_seg"].data_ptr()), C.c_void_p(tab["chunk_start"].data_ptr()),
                   C.c_void_p(bias.data_ptr() if bias is not None else 0), tab["chunk_seg"].numel(), _CHUNK, group["lr"], b1, b2, group["eps"],
                   group["weight_decay"], group["step"], 1.0 if scale is None else scale,
                   C.c_void_p(torch.cuda.current_stream(blk.device).cuda_stream)), name)

    # ------------------------------------------------------------------ the capturable step
    def _sync_lr(self, group, flat):
        if flat["lr_host"] != group["lr"]:
            if torch.cuda.is_current_stream_capturing():
                raise L.KanConvError(f"FusedAdamW(capturable=True): the device copy of lr holds {flat['lr_host']}, group['lr'] is {group['lr']}; nothing "
                                     "may be uploaded while the stream is capturing -- run one eager step, or call sync_hyper(), before recording")
            self._upload_lr(group, flat)

    def _step_capturable(self, lib, group, flat, ptrs, scale, masked=None):
        """``masked``: None, or the guard's copy of the group's address table (all zeros on a skipped step) -- or, accumulating without a guard, the
        gated table --, which both launches then read instead of ``seg_grad``."""
        blk, tab = flat["block"], flat["tab"]
        self._sync_lr(group, flat)
        if scale is None and masked is None:                               # (the statistics pass of a clipping or guarded step filled every table)
            self._fill_table(lib, flat, ptrs)
        b1, b2 = group["betas"]
        stream = C.c_void_p(torch.cuda.current_stream(blk.device).cuda_stream)
        seg_grad = C.c_void_p((tab["seg_grad"] if masked is None else masked).data_ptr())
        row = lambda r: C.c_void_p(blk.data_ptr() + 4 * r * flat["n"])
        fn, name = (lib.kan_adamw_step_segments_dev, "kan_adamw_step_segments_dev") if scale is None else \
                   (lib.kan_adamw_step_segments_dev_clip, "kan_adamw_step_segments_dev_clip")
        L.check(lib.kan_adamw_advance(C.c_void_p(tab["seg_step"].data_ptr()), seg_grad, len(ptrs), stream), "kan_adamw_advance")
        L.check(fn(row(0), row(1), row(2), seg_grad, C.c_void_p(tab["seg_off"].data_ptr()), C.c_void_p(tab["seg_n"].data_ptr()),
                   C.c_void_p(tab["chunk_seg"].data_ptr()), C.c_void_p(tab["chunk_start"].data_ptr()), C.c_void_p(flat["lr_dev"].data_ptr()),
                   C.c_void_p(tab["seg_step"].data_ptr()), tab["chunk_seg"].numel(), _CHUNK, b1, b2, group["eps"], group["weight_decay"],
                   1.0 if scale is None else scale, stream), name)

    @staticmethod
    def _upload_lr(group, flat):
        flat["lr_dev"].fill_(float(group["lr"]))                           # a fill launch carrying the double: no host memory is read later
        flat["lr_host"] = group["lr"]

    def _need_capturable(self, what):
        if not self.capturable:
            raise L.KanConvError(f"FusedAdamW.{what} belongs to capturable=True")

    def sync_hyper(self):
        """Bring the device copy of every group's ``lr`` up to date with ``group["lr"]`` (one small launch per group whose lr a scheduler moved;
        nothing otherwise), and that of ``max_grad_norm`` likewise.  Call it before recording and between replays -- never while the stream is
        capturing."""
        self._need_capturable("sync_hyper()")
        if self._max_grad_norm is not None and self._clip["buf"].is_cuda:
            self._sync_max_norm(self._clip)
        for group, flat in zip(self.param_groups, self._flat):
            if flat is not None and flat["block"].is_cuda and flat["lr_host"] != group["lr"]:
                if torch.cuda.is_current_stream_capturing():
                    raise L.KanConvError("FusedAdamW.sync_hyper() while the stream is capturing: call it before recording")
                self._upload_lr(group, flat)

    def sync_steps(self):
        """Read the device step counts into the host view (``flat["steps"]``, ``group["step"]``): ONE device read per group, for checkpoints and
        inspection -- never on the step path.  ``state_dict()`` calls it."""
        self._need_capturable("sync_steps()")
        for group, flat in zip(self.param_groups, self._flat):
            if flat is not None:
                flat["steps"] = [int(s) for s in flat["tab"]["seg_step"].tolist()]
                group["step"] = max(flat["steps"])

    def captured_addresses(self):
        """What the last recorded ``step()`` froze: per group, the gradient address of every parameter (0 = none), or None."""
        return [None if flat is None else flat.get("captured_ptrs") for flat in self._flat]

    def after_replay(self, captured):
        """Host-side bookkeeping after a graph holding a recorded ``step()`` was replayed (``captured``: ``captured_addresses()`` as of its
        recording): the device address table now holds the recorded addresses, and every parameter the recorded step updates gets its version
        counter bumped, so that a later eager forward re-packs the weights the replay wrote through raw pointers."""
        self._need_capturable("after_replay()")
        for flat, ptrs in zip(self._flat, captured):
            if flat is None or ptrs is None:
                continue
            flat["tab"]["grad_ptrs"] = list(ptrs)
            for p, a in zip(flat["params"], ptrs):
                if a:
                    torch.autograd.graph.increment_version(p)

    def snapshot(self):
        """Copies of everything a step changes on the device (parameters, both moments, the step counts; behind them, once the optimizer has been
        guarded, the guard's counters and flags; behind those, with ``accumulate_steps > 1``, a dict holding the accumulator rows and the window's
        counter and ``seen`` flags) -- ``restore()`` puts them back.  With ``accumulate_steps == 1`` the list is what it always was."""
        self._need_capturable("snapshot()")
        saved = [None if flat is None else (flat["block"].clone(), flat["tab"]["seg_step"].clone()) for flat in self._flat]
        if self._guard is not None:
            saved.append(self._guard["buf"][:5 + self._guard["flags"].numel()].clone())
        if self._accum is not None:
            saved.append(dict(accum_rows=[None if r is None else r.clone() for r in self._accum["rows"]], accum_state=self._accum["state"].clone()))
        return saved

    @torch.no_grad()
    def restore(self, saved):
        if saved and isinstance(saved[-1], dict):                          # the window of an accumulating optimizer
            saved, window = saved[:-1], saved[-1]
            if self._accum is not None and window["accum_state"].numel() == self._accum["state"].numel():
                self._accum["state"].copy_(window["accum_state"])
                for row, r in zip(self._accum["rows"], window["accum_rows"]):
                    if row is not None:
                        row.copy_(r)
        if self._guard is not None and len(saved) > len(self._flat):
            self._guard["buf"][:saved[-1].numel()].copy_(saved[-1])
        for flat, s in zip(self._flat, saved):
            if flat is None:
                continue
            flat["block"].copy_(s[0]); flat["tab"]["seg_step"].copy_(s[1])
            for p in flat["params"]:                                       # written behind autograd's back: the packed-weight cache must notice
                torch.autograd.graph.increment_version(p)

    def state_dict(self):
        if self.capturable:
            self.sync_steps()
        for group, flat in zip(self.param_groups, self._flat):
            if flat is not None:
                self._link_state(group, flat)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group, flat in zip(self.param_groups, self._flat):
            if flat is None:
                continue
            steps_seen = 0                          # one step count per group (torch keeps one per parameter; they agree)
            with torch.no_grad():
                for p, (_, mv, vv) in zip(flat["params"], flat["views"]):
                    st = self.state.get(p, {})
                    if "exp_avg" in st:
                        mv.copy_(st["exp_avg"]); vv.copy_(st["exp_avg_sq"])
                        flat["steps"][flat["index"][id(p)]] = int(st.get("step", 0))
                        group["step"] = max(int(st.get("step", 0)), steps_seen)
                        steps_seen = group["step"]
                if self.capturable:                 # the counts the kernels read: one small upload per group at resume time
                    flat["tab"]["seg_step"].copy_(torch.tensor(flat["steps"], dtype=torch.int32))
            self._link_state(group, flat)

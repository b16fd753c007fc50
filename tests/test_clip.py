"""FusedAdamW(max_grad_norm=...) as far as it goes without a GPU: the keyword and its validation, what stays unchanged with the default
(None), the layout of the statistics buffer for a hand-written two-group case, the refusals, and the C ABI of the four new entry points
(declared, bound, exported, and refusing bad arguments on the host).  The kernels run in tests/test_gpu_clip.py."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch
import torch.nn as nn

import convkan_amd as K
from convkan_amd import _lib as L
from convkan_amd import optim as O
from convkan_amd import train as T
from convkan_amd.optim import FusedAdamW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"kan_grad_sqnorm_chunks", "kan_grad_norm_finish", "kan_adamw_step_segments_clip", "kan_adamw_step_segments_dev_clip"}


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(7, 5), nn.PReLU(), nn.Linear(5, 3, bias=False))


def test_clip_exports_are_declared_bound_and_exported():
    K.build_library()
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "kanconv.h")).read()
    declared = set(re.findall(r"\b(kan_[a-z0-9_]+)\s*\(", header))
    assert NEW <= declared
    assert NEW <= set(L.SIGNATURES)                                       # no digit in a name: the plain table
    assert declared == set(L.SIGNATURES) | set(L.SIGNATURES_DIGIT_NAMES)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, name
    for line in ("evaluations.py:33", "evaluations.py:66-71", "generic_train.py:24-25"):      # the reference lines the entry points stand in for
        assert line in header[header.index("Global-norm gradient clipping"):], line


def test_clip_entry_points_refuse_bad_arguments_on_the_host():
    """Host-side returns: nothing is launched (the pointers are never dereferenced, no device is needed)."""
    K.build_library()
    lib = L.load()
    ok, odd, null = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4), ctypes.c_void_p(0)

    def refused(rc, what):
        assert rc != 0 and lib.kan_last_error(), what

    def chunks(**kw):
        a = dict(seg_grad=ok, seg_n=ok, chunk_seg=ok, chunk_start=ok, n_chunks=1, chunk=8192, partial=ok, st=null) | kw
        return lib.kan_grad_sqnorm_chunks(*a.values())

    def finish(**kw):
        a = dict(partial=ok, first=ok, n_seg=1, max_norm=ok, seg_sq=ok, out=ok, st=null) | kw
        return lib.kan_grad_norm_finish(*a.values())

    def classic(**kw):
        a = dict(p=ok, m=ok, v=ok, seg_grad=ok, seg_off=ok, seg_n=ok, chunk_seg=ok, chunk_start=ok, bias=null, n_chunks=1, chunk=8192, lr=1e-3, b1=0.9,
                 b2=0.999, eps=1e-8, wd=1e-2, step=1, scale=ok, st=null) | kw
        return lib.kan_adamw_step_segments_clip(*a.values())

    def dev(**kw):
        a = dict(p=ok, m=ok, v=ok, seg_grad=ok, seg_off=ok, seg_n=ok, chunk_seg=ok, chunk_start=ok, lr_dev=ok, seg_step=ok, n_chunks=1, chunk=8192,
                 b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, scale=ok, st=null) | kw
        return lib.kan_adamw_step_segments_dev_clip(*a.values())

    for k in ("seg_grad", "seg_n", "chunk_seg", "chunk_start", "partial"):
        refused(chunks(**{k: null}), f"chunks: null {k}")
    for k in ("partial", "first", "max_norm", "seg_sq", "out"):
        refused(finish(**{k: null}), f"finish: null {k}")
    for k in ("p", "m", "v", "seg_grad", "seg_off", "seg_n", "chunk_seg", "chunk_start", "scale"):
        refused(classic(**{k: null}), f"segments_clip: null {k}")
    for k in ("p", "m", "v", "seg_grad", "seg_off", "seg_n", "chunk_seg", "chunk_start", "lr_dev", "seg_step", "scale"):
        refused(dev(**{k: null}), f"segments_dev_clip: null {k}")
    for fn, name in ((chunks, "chunks"), (classic, "segments_clip"), (dev, "segments_dev_clip")):
        for bad in (dict(n_chunks=0), dict(n_chunks=-1), dict(chunk=0), dict(chunk=6), dict(chunk=-4)):
            refused(fn(**bad), f"{name}: {bad}")
    refused(finish(n_seg=0), "finish: n_seg 0")
    refused(finish(n_seg=-1), "finish: negative n_seg")
    refused(chunks(partial=odd), "chunks: misaligned partial")
    refused(finish(seg_sq=odd), "finish: misaligned seg_sq")
    refused(classic(step=0), "segments_clip: step 0")
    refused(classic(p=odd), "segments_clip: misaligned p")
    refused(dev(lr_dev=odd), "segments_dev_clip: misaligned lr_dev")
    refused(dev(b1=1.0), "segments_dev_clip: beta1 = 1")


def test_keyword_default_and_validation():
    assert inspect.signature(FusedAdamW.__init__).parameters["max_grad_norm"].default is None
    assert list(inspect.signature(FusedAdamW.__init__).parameters)[-1] == "max_grad_norm"        # a new keyword AFTER the existing ones
    assert inspect.signature(T.train_model_generic).parameters["max_grad_norm"].default is None
    assert FusedAdamW(_net().parameters()).max_grad_norm is None
    for good in (0, 0.0, 1.0, 1e-3, float("inf")):
        opt = FusedAdamW(_net().parameters(), max_grad_norm=good)
        assert opt.max_grad_norm == float(good) and isinstance(opt.max_grad_norm, float)
    for bad in (-1.0, -1e-30, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdamW(_net().parameters(), max_grad_norm=bad)
    opt = FusedAdamW(_net().parameters(), max_grad_norm=1.0)
    opt.max_grad_norm = 0.25                                               # a settable attribute, validated the same way
    assert opt.max_grad_norm == 0.25
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.max_grad_norm = -2.0
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.max_grad_norm = float("nan")
    assert opt.max_grad_norm == 0.25


@pytest.mark.parametrize("capturable", [False, True])
def test_off_by_default_nothing_changes(capturable):
    plain = FusedAdamW(_net().parameters(), capturable=capturable)
    off = FusedAdamW(_net().parameters(), capturable=capturable, max_grad_norm=None)
    on = FusedAdamW(_net().parameters(), capturable=capturable, max_grad_norm=1.0)
    assert off._clip is None and plain._clip is None                      # no statistics buffer unless asked for
    for a in (off, on):
        assert [sorted(g) for g in a.param_groups] == [sorted(g) for g in plain.param_groups]
        assert "max_grad_norm" not in a.param_groups[0]
        sa, sp = a.state_dict(), plain.state_dict()
        assert sorted(sa) == sorted(sp) and [sorted(g) for g in sa["param_groups"]] == [sorted(g) for g in sp["param_groups"]]
        assert {k: sorted(v) for k, v in sa["state"].items()} == {k: sorted(v) for k, v in sp["state"].items()}
        assert set(a._flat[0]) == set(plain._flat[0]) and set(a._flat[0]["tab"]) == set(plain._flat[0]["tab"])


def test_state_dict_of_a_clipping_optimizer_loads_into_torch_adamw():
    opt = FusedAdamW(_net().parameters(), lr=3e-3, weight_decay=0.02, max_grad_norm=0.5)
    opt._flat[0]["steps"][:] = [4, 4, 1, 4]
    sd = opt.state_dict()
    ref = torch.optim.AdamW(_net().parameters(), foreach=False)
    ref.load_state_dict(sd)
    assert [int(ref.state_dict()["state"][i]["step"]) for i in range(4)] == [4, 4, 1, 4]
    assert ref.param_groups[0]["lr"] == 3e-3 and ref.param_groups[0]["weight_decay"] == 0.02
    back = FusedAdamW(_net().parameters(), max_grad_norm=2.0)
    back.load_state_dict(ref.state_dict())
    assert back._flat[0]["steps"] == [4, 4, 1, 4] and back.max_grad_norm == 2.0       # not part of the state: the constructor's value stays


def test_statistics_buffer_of_a_two_group_layout():
    """Group 0: 1, 8192, 8193 and 20000 elements (1 + 1 + 2 + 3 chunks) and a frozen parameter in between; group 1: 5 and 16385 elements
    (1 + 3 chunks).  seg_first_chunk is the running sum over BOTH groups; each group's chunk launch starts at its own offset."""
    assert O._CHUNK == 8192
    mk = lambda n: nn.Parameter(torch.zeros(n))
    frozen = nn.Parameter(torch.zeros(9), requires_grad=False)
    g0, g1 = [mk(1), mk(8192), frozen, mk(8193), mk(20000)], [mk(5), mk(16385)]
    opt = FusedAdamW([dict(params=g0), dict(params=g1, lr=1e-2)], max_grad_norm=1.0)
    clip = opt._clip
    assert clip["seg_first_chunk"].dtype == torch.int32 and clip["seg_first_chunk"].tolist() == [0, 1, 2, 4, 7, 8, 11]
    assert clip["chunk0"] == [0, 7]
    assert [f["tab"]["chunk_seg"].numel() for f in opt._flat] == [7, 4]                  # the step kernel's own chunk tables
    assert clip["partial"].dtype == torch.float64 and clip["partial"].numel() == 11
    assert clip["seg_sq"].dtype == torch.float64 and clip["seg_sq"].numel() == 6
    assert clip["out"].dtype == torch.float32 and clip["out"].numel() == 3
    buf = clip["buf"]                                                      # ONE allocation: every view lies inside it, none overlaps another
    spans = sorted((t.data_ptr() - buf.data_ptr(), t.data_ptr() - buf.data_ptr() + t.numel() * t.element_size())
                   for t in (clip["partial"], clip["seg_sq"], clip["seg_first_chunk"], clip["out"]))
    assert spans == [(0, 88), (88, 136), (136, 164), (168, 180)]
    assert buf.numel() * buf.element_size() == 184 and buf.data_ptr() % 8 == 0
    assert opt.grad_norms().shape == (6,) and opt.grad_norm.shape == () and opt.clip_scale.shape == ()
    assert opt.grad_norm.dtype == opt.clip_scale.dtype == opt.grad_norms().dtype == torch.float32
    assert opt.grad_norm.data_ptr() == clip["out"].data_ptr() and opt.clip_scale.data_ptr() == clip["out"].data_ptr() + 4      # views, not copies
    before = buf.data_ptr()
    opt.max_grad_norm = 3.0                                                # a new value is not a new buffer
    assert opt._clip["buf"].data_ptr() == before
    opt.add_param_group(dict(params=[mk(8200)]))                           # a new layout is
    assert opt._clip["seg_first_chunk"].tolist() == [0, 1, 2, 4, 7, 8, 11, 13] and opt._clip["chunk0"] == [0, 7, 11]


def test_statistics_reads_raise_when_clipping_is_off():
    opt = FusedAdamW(_net().parameters())
    for read in (lambda: opt.grad_norm, lambda: opt.clip_scale, opt.grad_norms):
        with pytest.raises(L.KanConvError, match="max_grad_norm"):
            read()
    on = FusedAdamW(_net().parameters(), max_grad_norm=1.0)
    on.max_grad_norm = None                                                # switched off: the reads refuse again
    with pytest.raises(L.KanConvError, match="max_grad_norm"):
        on.grad_norm
    late = FusedAdamW(_net().parameters())
    late.max_grad_norm = 1.0                                               # switched on after construction: the buffer is built then
    assert late.grad_norms().tolist() == [0.0] * 4 and math.isfinite(float(late.grad_norm))


@pytest.mark.parametrize("capturable", [False, True])
def test_step_on_cpu_parameters_still_raises(capturable):
    net = _net()
    opt = FusedAdamW(net.parameters(), capturable=capturable, max_grad_norm=1.0)
    net(torch.randn(2, 7)).sum().backward()
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        opt.step()
    if capturable:
        opt.sync_hyper()                                                   # nothing to do on CPU parameters, and no error

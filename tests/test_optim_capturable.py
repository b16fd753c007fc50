"""FusedAdamW(capturable=True) and GraphedStep(optimizer=...) as far as they go without a GPU: the new keywords and their defaults, the
device-state layout of a capturable optimizer on CPU parameters, the refusals, and the C ABI of the capturable step (the export whose name
holds a digit is bound from _lib.SIGNATURES_DIGIT_NAMES: tests/test_host.py's header scan reads lower-case names only).  The kernels run in
tests/test_gpu_optim_capturable.py."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn as nn

import convkan_amd as K
from convkan_amd import _lib as L
from convkan_amd import train as T
from convkan_amd.optim import FusedAdamW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAB_KEYS = {"seg_off", "seg_n", "chunk_seg", "chunk_start", "seg_grad", "grad_ptrs", "seg_bias"}        # what flat["tab"] held before seg_step


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(7, 5), nn.PReLU(), nn.Linear(5, 3, bias=False))


def test_new_keywords_and_their_defaults():
    assert inspect.signature(FusedAdamW.__init__).parameters["capturable"].default is False
    gs = inspect.signature(T.GraphedStep.__init__).parameters
    assert gs["optimizer"].default is None and gs["criterion"].default is None and gs["split_precision"].default is False
    assert list(gs)[-1] == "optimizer"                                   # a new keyword AFTER the existing ones
    for fn in (T.train_model_generic, T.train_and_test_models):
        assert inspect.signature(fn).parameters["graphed"].default is False
    assert FusedAdamW(_net().parameters()).capturable is False


def test_capturable_layout_on_cpu_parameters():
    net = _net()
    before = [p.detach().clone() for p in net.parameters()]
    opt = FusedAdamW(net.parameters(), lr=1e-3, capturable=True)
    flat = opt._flat[0]
    tab = flat["tab"]
    assert tab["seg_step"].dtype == torch.int32 and tab["seg_step"].tolist() == [0, 0, 0, 0]
    assert flat["lr_dev"].dtype == torch.float64 and flat["lr_dev"].shape == (1,)
    assert TAB_KEYS <= set(tab) and set(tab) - TAB_KEYS == {"seg_step"}
    classic = FusedAdamW(_net().parameters())._flat[0]
    assert set(classic["tab"]) == set(tab) and set(classic) == set(flat)            # one layout for both modes
    assert all(torch.equal(p, b) for p, b in zip(net.parameters(), before))
    assert "capturable" not in opt.param_groups[0]                       # a state_dict must load into torch.optim.AdamW as it is
    sd = opt.state_dict()                                                # the host view is read from seg_step
    assert [int(sd["state"][i]["step"]) for i in range(4)] == [0, 0, 0, 0]


def test_step_on_cpu_parameters_raises():
    net = _net()
    opt = FusedAdamW(net.parameters(), capturable=True)
    net(torch.randn(2, 7)).sum().backward()
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        opt.step()
    opt.sync_hyper()                                                     # nothing to do on CPU parameters, and no error


def test_host_bookkeeping_belongs_to_capturable():
    opt = FusedAdamW(_net().parameters())
    for call in (opt.sync_hyper, opt.sync_steps, opt.snapshot, lambda: opt.after_replay([None])):
        with pytest.raises(L.KanConvError, match="capturable=True"):
            call()


def test_state_dict_round_trip_carries_step_counts_on_cpu():
    """capturable <-> classic <-> torch.optim.AdamW, without a step: the counts travel through seg_step in both directions."""
    net = _net()
    cap = FusedAdamW(net.parameters(), capturable=True)
    cap._flat[0]["tab"]["seg_step"].copy_(torch.tensor([5, 5, 2, 0], dtype=torch.int32))
    sd = cap.state_dict()
    assert [int(sd["state"][i]["step"]) for i in range(4)] == [5, 5, 2, 0] and cap.param_groups[0]["step"] == 5
    classic = FusedAdamW(_net().parameters())
    classic.load_state_dict(sd)
    assert classic._flat[0]["steps"] == [5, 5, 2, 0]
    ref = torch.optim.AdamW(_net().parameters(), foreach=False)
    ref.load_state_dict(sd)
    assert [int(ref.state_dict()["state"][i]["step"]) for i in range(4)] == [5, 5, 2, 0]
    back = FusedAdamW(_net().parameters(), capturable=True)
    back.load_state_dict(ref.state_dict())
    assert back._flat[0]["tab"]["seg_step"].tolist() == [5, 5, 2, 0]
    back.load_state_dict(classic.state_dict())
    assert back._flat[0]["tab"]["seg_step"].tolist() == [5, 5, 2, 0]


def test_graphed_step_refuses_other_optimizers():
    net = _net()
    x, t = torch.randn(4, 7), torch.randint(0, 3, (4,))
    with pytest.raises(ValueError, match="capturable"):
        T.GraphedStep(net, x, t, optimizer=torch.optim.AdamW(net.parameters()))
    with pytest.raises(ValueError, match="capturable"):
        T.GraphedStep(net, x, t, optimizer=FusedAdamW(net.parameters()))


def test_graphed_drivers_refuse_what_is_not_built():
    net = _net()
    with pytest.raises(ValueError, match="capturable"):
        T.train_and_test_models(net, [], [], FusedAdamW(net.parameters()), epochs=1, graphed=True)
    with pytest.raises(ValueError, match="capturable"):
        T.train_and_test_models(net, [], [], torch.optim.AdamW(net.parameters()), epochs=1, graphed=True)
    with pytest.raises(ValueError, match="reducer"):
        T.train_and_test_models(net, [], [], FusedAdamW(net.parameters(), capturable=True), epochs=1, graphed=True, reducer=object())


def test_capturable_exports_are_declared_bound_and_exported():
    K.build_library()
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "kanconv.h")).read()
    new = {"kan_adamw_step_segments_dev", "kan_adamw_advance", "kan_adamw_dev_args", "kan_set_u64_table"}
    declared = set(re.findall(r"\b(kan_[a-z0-9_]+)\s*\(", header))
    assert new <= declared
    assert declared == set(L.SIGNATURES) | set(L.SIGNATURES_DIGIT_NAMES)
    assert not set(L.SIGNATURES) & set(L.SIGNATURES_DIGIT_NAMES)
    assert all(re.search(r"\d", n) for n in L.SIGNATURES_DIGIT_NAMES)    # only names the lower-case scan cannot see live there
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in new:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, name


def test_capturable_entry_points_refuse_bad_arguments_on_the_host():
    """Host-side returns: nothing is launched (the pointers are never dereferenced, no device is needed)."""
    K.build_library()
    lib = L.load()
    ok, odd, null = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4), ctypes.c_void_p(0)

    def refused(rc, what):
        assert rc != 0 and lib.kan_last_error(), what

    def segm(**kw):
        a = dict(p=ok, m=ok, v=ok, seg_grad=ok, seg_off=ok, seg_n=ok, chunk_seg=ok, chunk_start=ok, lr_dev=ok, seg_step=ok, n_chunks=1, chunk=8192,
                 b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, gs=1.0, st=null) | kw
        return lib.kan_adamw_step_segments_dev(*a.values())

    for k in ("p", "m", "v", "seg_grad", "seg_off", "seg_n", "chunk_seg", "chunk_start", "lr_dev", "seg_step"):
        refused(segm(**{k: null}), f"segments_dev: null {k}")
    for k in ("p", "m", "v", "lr_dev"):
        refused(segm(**{k: odd}), f"segments_dev: misaligned {k}")
    for bad in (dict(chunk=0), dict(chunk=6), dict(n_chunks=-1), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0), dict(wd=-1.0)):
        refused(segm(**bad), f"segments_dev: {bad}")
    assert segm(n_chunks=0) == 0
    refused(lib.kan_adamw_advance(null, ok, 1, null), "advance: null seg_step")
    refused(lib.kan_adamw_advance(ok, null, 1, null), "advance: null seg_grad")
    refused(lib.kan_adamw_advance(ok, ok, -1, null), "advance: negative n_seg")
    assert lib.kan_adamw_advance(ok, ok, 0, null) == 0
    vals = (ctypes.c_ulonglong * 65)()
    refused(lib.kan_set_u64_table(null, 0, vals, 1, null), "set_u64_table: null table")
    refused(lib.kan_set_u64_table(ok, 0, null, 1, null), "set_u64_table: null values")
    refused(lib.kan_set_u64_table(ok, 0, vals, 65, null), "set_u64_table: more than 64")
    refused(lib.kan_set_u64_table(ok, -1, vals, 1, null), "set_u64_table: negative first")
    refused(lib.kan_set_u64_table(odd, 0, vals, 1, null), "set_u64_table: misaligned table")
    assert lib.kan_set_u64_table(ok, 0, vals, 0, null) == 0
    refused(lib.kan_adamw_dev_args(null, ok, 0.9, 0.999, 1e-8, 1e-2, 1.0, ok, null), "dev_args: null lr")
    refused(lib.kan_adamw_dev_args(ok, ok, 0.9, 0.999, 1e-8, 1e-2, 1.0, null, null), "dev_args: null out")

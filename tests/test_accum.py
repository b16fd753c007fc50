"""Gradient accumulation as far as it goes without a GPU: the C ABI of kan_grad_accumulate and kan_accum_gate (declared, bound, exported, refusing
bad arguments on the host), FusedAdamW.accumulate_steps as a switch (default, validation, what stays unchanged when it is 1, the layout of its
buffers when it is not), the driver keyword, and the numpy model of tests/accum_cells.py against plain arithmetic.  The kernels run in
tests/test_gpu_accum.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import accum_cells as A
import convkan_amd as K
from convkan_amd import _lib as L
from convkan_amd import train as T
from convkan_amd.optim import FusedAdamW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"kan_grad_accumulate", "kan_accum_gate"}


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(7, 5), nn.PReLU(), nn.Linear(5, 3, bias=False))


def test_accum_exports_are_declared_bound_and_exported():
    K.build_library()
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "kanconv.h")).read()
    declared = set(re.findall(r"\b(kan_[a-z0-9_]+)\s*\(", header))
    assert NEW <= declared and NEW <= set(L.SIGNATURES)
    assert declared == set(L.SIGNATURES) | set(L.SIGNATURES_DIGIT_NAMES)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, name
    section = header[header.index("Gradient accumulation decided on the device"):header.index("cross-entropy loss and test metrics")]
    assert "evaluations.py:44-72" in section and "NO accumulation" in section          # the loop it extends, and that the reference has none
    assert os.path.exists(os.path.join(os.path.dirname(L.__file__), "csrc", "kan_accum.hip"))


def test_accum_entry_points_refuse_bad_arguments_on_the_host():
    """Host-side returns: nothing is launched (the pointers are never dereferenced, no device is needed)."""
    K.build_library()
    lib = L.load()
    ok, odd4, odd8, odd2, null = (ctypes.c_void_p(v) for v in (4096, 4096 + 4, 4096 + 8, 4096 + 2, 0))

    def refused(rc, what):
        assert rc != 0 and lib.kan_last_error(), what

    def accumulate(**kw):
        a = dict(acc=ok, seg_grad=ok, seg_off=ok, seg_n=ok, chunk_seg=ok, chunk_start=ok, n_chunks=1, chunk_elems=8192, micro_dev=ok, m=0, k=2,
                 seen=ok, st=null) | kw
        return lib.kan_grad_accumulate(*a.values())

    def gate(**kw):
        a = dict(groups=ok, n_groups=1, micro=ok, k=2, guard_counters=null, st=null) | kw
        return lib.kan_accum_gate(*a.values())

    for name in ("acc", "seg_grad", "seg_off", "seg_n", "chunk_seg", "chunk_start", "seen"):
        refused(accumulate(**{name: null}), f"accumulate: null {name}")
    for name in ("acc", "seg_grad", "seg_off"):
        refused(accumulate(**{name: odd4}), f"accumulate: {name} 4 bytes off")
    refused(accumulate(acc=odd8), "accumulate: acc 8 bytes off (float4 stores)")
    for name in ("seg_n", "chunk_seg", "chunk_start", "micro_dev", "seen"):
        refused(accumulate(**{name: odd2}), f"accumulate: {name} 2 bytes off")
    for bad in (dict(n_chunks=0), dict(n_chunks=-1), dict(chunk_elems=0), dict(chunk_elems=-4), dict(chunk_elems=6), dict(k=0), dict(k=-2)):
        refused(accumulate(**bad), f"accumulate: {bad}")
    for bad in (dict(m=-1), dict(m=2), dict(m=7)):                          # m by value must lie in the window
        refused(accumulate(micro_dev=null, **bad), f"accumulate: micro_dev NULL, {bad}")
    for name in ("groups", "micro"):
        refused(gate(**{name: null}), f"gate: null {name}")
    refused(gate(groups=odd4), "gate: misaligned groups")
    refused(gate(micro=odd2), "gate: misaligned micro")
    refused(gate(guard_counters=odd4), "gate: misaligned guard_counters")
    for bad in (dict(n_groups=0), dict(n_groups=-1), dict(k=0), dict(k=-1)):
        refused(gate(**bad), f"gate: {bad}")


def test_switch_default_signature_and_validation():
    assert "accumulate_steps" not in inspect.signature(FusedAdamW.__init__).parameters     # an attribute, not a keyword
    assert list(inspect.signature(FusedAdamW.__init__).parameters)[-1] == "max_grad_norm"
    assert "accumulate_steps" not in inspect.signature(T.GraphedStep.__init__).parameters
    names = list(inspect.signature(T.train_model_generic).parameters)
    assert names[-1] == "accumulate_steps" and names[-2] == "skip_nonfinite"
    assert inspect.signature(T.train_model_generic).parameters["accumulate_steps"].default == 1
    assert "accumulate_steps" not in inspect.signature(T.train_and_test_models).parameters  # the optimizer is the caller's
    for capturable in (False, True):
        opt = FusedAdamW(_net().parameters(), capturable=capturable)
        assert opt.accumulate_steps == 1 and opt._accum is None and opt.micro_step == 0
        opt.reset_accumulation()                                           # nothing to drop: allowed
        for bad in (0, -1, -7, 1.0, 2.0, 1.5, "2", None, True, False, [2]):
            with pytest.raises(ValueError, match="accumulate_steps"):
                opt.accumulate_steps = bad
            assert opt.accumulate_steps == 1 and opt._accum is None
        opt.accumulate_steps = 4
        assert opt.accumulate_steps == 4 and opt._accum is not None and opt._accum["k"] == 4 and opt.micro_step == 0
        opt.accumulate_steps = 1                                           # back: everything is released
        assert opt.accumulate_steps == 1 and opt._accum is None
    with pytest.raises(ValueError, match="accumulate_steps"):
        T.train_model_generic(_net(), [], device="cpu", epochs=1, accumulate_steps=0)


@pytest.mark.parametrize("capturable", [False, True])
def test_an_open_window_refuses_a_new_k(capturable):
    opt = FusedAdamW(_net().parameters(), capturable=capturable)
    opt.accumulate_steps = 3
    if capturable:
        opt._accum["micro"].fill_(2)                                       # what two micro-steps leave in the counter
    else:
        opt._accum["micro_host"] = 2
    assert opt.micro_step == 2
    for k in (1, 2, 5):
        with pytest.raises(L.KanConvError, match="open window"):
            opt.accumulate_steps = k
    opt.accumulate_steps = 3                                               # the same value is no change
    assert opt.accumulate_steps == 3 and opt.micro_step == 2
    opt.reset_accumulation()
    assert opt.micro_step == 0
    opt.accumulate_steps = 2
    assert opt.accumulate_steps == 2 and opt._accum["k"] == 2


@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
def test_k_equal_one_nothing_changes(max_grad_norm):
    plain = FusedAdamW(_net().parameters(), capturable=True, max_grad_norm=max_grad_norm)
    was_on = FusedAdamW(_net().parameters(), capturable=True, max_grad_norm=max_grad_norm)
    was_on.accumulate_steps = 3
    on_keys = (set(was_on._flat[0]), set(was_on._flat[0]["tab"]), [sorted(g) for g in was_on.param_groups])
    on_sd = was_on.state_dict()
    assert len(was_on.snapshot()) == 2 and isinstance(was_on.snapshot()[-1], dict)         # the window travels behind the blocks
    was_on.accumulate_steps = 1
    for a in (plain, was_on):
        assert a._accum is None and a._guard is None
        assert set(a._flat[0]) == {"params", "block", "views", "n", "tab", "steps", "index", "lr_dev", "lr_host"}
        assert set(a._flat[0]["tab"]) == {"seg_off", "seg_n", "chunk_seg", "chunk_start", "seg_grad", "grad_ptrs", "seg_bias", "seg_step"}
        assert set(a.param_groups[0]) == {"params", "lr", "betas", "eps", "weight_decay", "step"}
        snap = a.snapshot()                                                # exactly what it was: one (block, counts) pair per group
        assert len(snap) == 1 and isinstance(snap[0], tuple) and len(snap[0]) == 2
        sd = a.state_dict()
        assert sorted(sd) == ["param_groups", "state"]
        assert all(sorted(v) == ["exp_avg", "exp_avg_sq", "step"] for v in sd["state"].values())
    assert on_keys == (set(plain._flat[0]), set(plain._flat[0]["tab"]), [sorted(g) for g in plain.param_groups])      # nor does k > 1 add a key
    assert sorted(on_sd) == ["param_groups", "state"] and all(sorted(v) == ["exp_avg", "exp_avg_sq", "step"] for v in on_sd["state"].values())
    assert "accumulate_steps" not in on_sd["param_groups"][0]
    ref = torch.optim.AdamW(_net().parameters(), foreach=False)
    ref.load_state_dict(on_sd)                                             # still torch's format, with a window configured


def test_accum_buffers_of_a_two_group_layout():
    mk = lambda n: nn.Parameter(torch.zeros(n))
    frozen = nn.Parameter(torch.zeros(9), requires_grad=False)
    g0, g1 = [mk(1), mk(8192), frozen, mk(8193)], [mk(5), mk(16385)]
    opt = FusedAdamW([dict(params=g0), dict(params=g1, lr=1e-2)], capturable=True)
    opt.accumulate_steps = 4
    a = opt._accum
    assert a["k"] == 4 and a["n_groups"] == 2
    assert [r.numel() for r in a["rows"]] == [f["n"] for f in opt._flat] == [64 + 8192 + 8256, 64 + 16448]
    assert all(r.dtype == torch.float32 and r.data_ptr() % 16 == 0 and not r.any() for r in a["rows"])
    assert [s.numel() for s in a["seen"]] == [3, 2] and all(s.dtype == torch.int32 for s in a["seen"])
    assert [t.numel() for t in a["gated"]] == [3, 2] and [t.numel() for t in a["addr"]] == [3, 2]
    for gi, f in enumerate(opt._flat):                                     # the accumulator address of a segment: its row + seg_off
        assert a["addr"][gi].tolist() == [a["rows"][gi].data_ptr() + 4 * o for o in f["tab"]["seg_off"].tolist()] == a["addr_host"][gi]
    assert a["groups"].tolist() == [a["addr"][0].data_ptr(), a["gated"][0].data_ptr(), a["seen"][0].data_ptr(), 3,
                                    a["addr"][1].data_ptr(), a["gated"][1].data_ptr(), a["seen"][1].data_ptr(), 2]
    assert a["micro"].dtype == torch.int32 and a["micro"].data_ptr() == a["buf"].data_ptr() and a["buf"].data_ptr() % 8 == 0
    assert all(t.data_ptr() % 8 == 0 for t in (*a["addr"], *a["gated"], *a["seen"], a["groups"]))
    assert a["state"].numel() == 1 + 2 + 1                                 # the counter's word, then the seen flags in whole 8-byte words
    spans = sorted((t.data_ptr() - a["buf"].data_ptr(), t.data_ptr() - a["buf"].data_ptr() + t.element_size() * t.numel())
                   for t in (a["micro"], *a["seen"], a["groups"], *a["addr"], *a["gated"]))
    assert all(hi <= lo2 for (_, hi), (lo2, _) in zip(spans, spans[1:])) and spans[-1][1] <= 8 * a["buf"].numel()     # nothing overlaps
    # snapshot / restore cover the rows, the flags and the counter
    a["rows"][1][5] = 3.0
    a["seen"][0][2] = 1
    a["micro"].fill_(3)
    saved = opt.snapshot()
    opt.reset_accumulation()
    a["rows"][1].zero_()
    assert opt.micro_step == 0 and not a["seen"][0].any()
    opt.restore(saved)
    assert opt.micro_step == 3 and a["seen"][0].tolist() == [0, 0, 1] and float(a["rows"][1][5]) == 3.0
    opt.reset_accumulation()
    opt.add_param_group(dict(params=[mk(8200)]))                           # a new layout: new buffers, a fresh window
    assert opt._accum["n_groups"] == 3 and [t.numel() for t in opt._accum["gated"]] == [3, 2, 1] and opt._accum["k"] == 4
    opt.skip_nonfinite = True                                              # the guard masks the gated tables of an accumulating step
    assert opt._guard_groups(opt._accum).tolist() == [v for g, m in zip(opt._accum["gated"], opt._guard["masked"])
                                                      for v in (g.data_ptr(), m.data_ptr(), g.numel())]


def test_step_on_cpu_parameters_still_raises():
    for capturable in (False, True):
        net = _net()
        opt = FusedAdamW(net.parameters(), capturable=capturable)
        opt.accumulate_steps = 2
        net(torch.randn(2, 7)).sum().backward()
        with pytest.raises(L.KanConvError, match="no CPU fallback"):
            opt.step()
        assert opt.micro_step == 0


def test_the_numpy_model_of_the_window():
    rng = np.random.default_rng(0)
    g = [rng.standard_normal(9).astype(np.float32) for _ in range(4)]
    g[0][3] = -0.0
    junk = np.full(9, np.nan, dtype=np.float32)
    first = A.micro_step(junk, g[0], 0, 3)
    assert first.view(np.int32).tolist() == g[0].view(np.int32).tolist() and np.signbit(first[3])       # a copy: -0.0 survives, the junk is gone
    assert not A.micro_step(junk, None, 0, 3).any()                         # zero-filled
    mid = A.micro_step(first, g[1], 1, 3)
    assert mid.dtype == np.float32 and np.array_equal(mid, g[0] + g[1]) and A.micro_step(mid, None, 1, 3) is mid
    last = A.micro_step(mid, g[2], 2, 3)
    assert last.dtype == np.float32 and np.array_equal(last, ((g[0] + g[1]) + g[2]) * np.float32(1.0 / 3.0))
    assert np.array_equal(A.micro_step(mid, None, 2, 3), mid * np.float32(1.0 / 3.0))
    assert np.array_equal(A.window_mean(g[:3]), last) and A.window_mean([None, None]) is None
    assert np.array_equal(A.window_mean([None, g[1], None]), g[1] * np.float32(1.0 / 3.0))              # a gradient in one micro-step of three: g / 3
    assert np.array_equal(A.window_mean([g[0]]), g[0])                      # k == 1: the copy alone
    exact = sum(x.astype(np.float64) for x in g) / 4
    assert np.abs(A.window_mean(g) - exact).max() <= 5 * 2.0 ** -24 * sum(np.abs(x).max() for x in g)       # three adds, s and one multiply, each half an ulp of at most sum max|g|
    lay = A.flat_layout([n for n, _ in A.KERNEL_LAYOUT])
    assert all(o % A.ALIGN == 0 for o in lay["seg_off"]) and lay["n"] % A.ALIGN == 0
    assert len(lay["chunk_seg"]) == 1 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3 and lay["chunk_start"][-3:] == [0, 8192, 16384]
    assert int(A.padding_mask(lay).sum()) == lay["n"] - sum(lay["seg_n"]) > 0
    opt = FusedAdamW([nn.Parameter(torch.zeros(n)) for n, _ in A.KERNEL_LAYOUT])                         # the optimizer's own layout agrees
    tab = opt._flat[0]["tab"]
    assert (tab["seg_off"].tolist(), tab["seg_n"].tolist(), tab["chunk_seg"].tolist(), tab["chunk_start"].tolist(), opt._flat[0]["n"]) == \
           (lay["seg_off"], lay["seg_n"], lay["chunk_seg"], lay["chunk_start"], lay["n"])
    assert A.gate_model(0, 1, [1, 0], [8, 16]) == ([8, 0], [0, 0], 0) and A.gate_model(0, 2, [1, 0], [8, 16]) == ([0, 0], [1, 0], 1)
    assert A.gate_model(1, 2, [0, 1], [8, 16]) == ([0, 16], [0, 0], 0)

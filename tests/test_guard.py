"""The device-side anomaly mode as far as it goes without a GPU: the C ABI of kan_nonfinite_count and kan_adamw_guard (declared, bound, exported,
refusing bad arguments on the host), FusedAdamW.skip_nonfinite as a switch (default, validation, what stays unchanged when it is off, the layout
of the guard's buffers), the slots AnomalyProbe lists for two models and its hooks, and the refusals on CPU tensors.  The kernels run in
tests/test_gpu_guard.py."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn as nn

import convkan_amd as K
from convkan_amd import _lib as L
from convkan_amd import ops
from convkan_amd import train as T
from convkan_amd.anomaly import ROOT_NAME
from convkan_amd.models import vggkan
from convkan_amd.optim import FusedAdamW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"kan_nonfinite_count", "kan_adamw_guard"}


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(7, 5), nn.PReLU(), nn.Linear(5, 3, bias=False))


def test_guard_exports_are_declared_bound_and_exported():
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
    section = header[header.index("Device-side anomaly mode"):header.index("cross-entropy loss and test metrics")]
    for line in ("train.py:431", "evaluations.py:33"):                     # the reference lines the entry points stand in for
        assert line in section, line
    assert os.path.exists(os.path.join(os.path.dirname(L.__file__), "csrc", "kan_guard.hip"))


def test_guard_entry_points_refuse_bad_arguments_on_the_host():
    """Host-side returns: nothing is launched (the pointers are never dereferenced, no device is needed)."""
    K.build_library()
    lib = L.load()
    ok, odd, odd2, null = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4), ctypes.c_void_p(4096 + 2), ctypes.c_void_p(0)

    def refused(rc, what):
        assert rc != 0 and lib.kan_last_error(), what

    def count(**kw):
        a = dict(x=ok, n=16, tick=ok, record=ok, st=null) | kw
        return lib.kan_nonfinite_count(*a.values())

    def guard(**kw):
        a = dict(seg_sq=ok, n_seg=1, groups=ok, n_groups=1, counters=ok, flags=ok, st=null) | kw
        return lib.kan_adamw_guard(*a.values())

    for k in ("x", "tick", "record"):
        refused(count(**{k: null}), f"count: null {k}")
    for bad in (-1, -2 ** 40):
        refused(count(n=bad), f"count: n = {bad}")
    refused(count(tick=odd), "count: misaligned tick")
    refused(count(record=odd), "count: misaligned record")
    refused(count(x=odd2), "count: misaligned x")
    refused(count(n=0, x=null), "count: n = 0 does not excuse a null pointer")
    assert count(n=0) == 0                                                 # n == 0: nothing is launched, and that is not an error
    assert count(n=0, x=odd) == 0                                          # 4-byte alignment is all the data needs
    for k in ("seg_sq", "groups", "counters", "flags"):
        refused(guard(**{k: null}), f"guard: null {k}")
        refused(guard(**{k: odd}), f"guard: misaligned {k}")
    for bad in (dict(n_seg=0), dict(n_seg=-1), dict(n_groups=0), dict(n_groups=-3)):
        refused(guard(**bad), f"guard: {bad}")


def test_switch_default_and_validation():
    assert "skip_nonfinite" not in inspect.signature(FusedAdamW.__init__).parameters      # an attribute, not a keyword
    assert "skip_nonfinite" not in inspect.signature(T.GraphedStep.__init__).parameters
    names = list(inspect.signature(T.train_model_generic).parameters)
    assert names.index("skip_nonfinite") == names.index("max_grad_norm") + 1
    assert inspect.signature(T.train_model_generic).parameters["skip_nonfinite"].default is False
    for capturable in (False, True):
        opt = FusedAdamW(_net().parameters(), capturable=capturable)
        assert opt.skip_nonfinite is False and opt._guard is None
    classic = FusedAdamW(_net().parameters())
    with pytest.raises(ValueError, match="capturable"):
        classic.skip_nonfinite = True
    assert classic.skip_nonfinite is False and classic._guard is None
    classic.skip_nonfinite = False                                         # switching it off is always allowed
    opt = FusedAdamW(_net().parameters(), capturable=True)
    opt.skip_nonfinite = True
    assert opt.skip_nonfinite is True
    with pytest.raises(ValueError, match="graphed"):
        T.train_model_generic(_net(), [], device="cpu", epochs=1, skip_nonfinite=True)
    for read in (lambda: classic.last_step_skipped, lambda: classic.skipped_steps, classic.guard_report, classic.reset_guard):
        with pytest.raises(L.KanConvError, match="skip_nonfinite"):
            read()


@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
def test_switch_off_nothing_changes(max_grad_norm):
    plain = FusedAdamW(_net().parameters(), capturable=True, max_grad_norm=max_grad_norm)
    was_on = FusedAdamW(_net().parameters(), capturable=True, max_grad_norm=max_grad_norm)
    was_on.skip_nonfinite = True
    on_keys = (set(was_on._flat[0]), set(was_on._flat[0]["tab"]))
    was_on.skip_nonfinite = False
    assert plain._guard is None
    assert (plain._clip is None) == (max_grad_norm is None) and (was_on._clip is None) == (max_grad_norm is None)
    for a in (plain, was_on):
        assert set(a._flat[0]) == {"params", "block", "views", "n", "tab", "steps", "index", "lr_dev", "lr_host"}
        assert set(a._flat[0]["tab"]) == {"seg_off", "seg_n", "chunk_seg", "chunk_start", "seg_grad", "grad_ptrs", "seg_bias", "seg_step"}
        assert set(a.param_groups[0]) == {"params", "lr", "betas", "eps", "weight_decay", "step"}
        assert "skip_nonfinite" not in a.param_groups[0]
        sd = a.state_dict()
        assert sorted(sd) == ["param_groups", "state"]
        assert all(sorted(v) == ["exp_avg", "exp_avg_sq", "step"] for v in sd["state"].values())
    assert on_keys == (set(plain._flat[0]), set(plain._flat[0]["tab"]))    # nor does the switch, when on, add a key to either
    assert [sorted(g) for g in was_on.param_groups] == [sorted(g) for g in plain.param_groups]
    if max_grad_norm is not None:
        assert set(was_on._clip) == set(plain._clip)
    ref = torch.optim.AdamW(_net().parameters(), foreach=False)
    ref.load_state_dict(was_on.state_dict())                               # still torch's format


def test_guard_buffers_of_a_two_group_layout():
    mk = lambda n: nn.Parameter(torch.zeros(n))
    frozen = nn.Parameter(torch.zeros(9), requires_grad=False)
    g0, g1 = [mk(1), mk(8192), frozen, mk(8193)], [mk(5), mk(16385)]
    opt = FusedAdamW([dict(params=g0), dict(params=g1, lr=1e-2)], capturable=True)
    opt.skip_nonfinite = True
    g = opt._guard
    assert opt._clip is None                                               # the guard's statistics are its own
    assert g["stats"]["seg_first_chunk"].tolist() == [0, 1, 2, 4, 5, 8] and g["stats"]["out"].tolist()[2] == float("inf")
    assert g["buf"].dtype == torch.int64 and g["buf"].numel() == 5 + 5 + 6 + 5 and g["buf"].data_ptr() % 8 == 0
    assert g["counters"].numel() == 5 and g["flags"].numel() == 5 and g["n_groups"] == 2
    assert [m.numel() for m in g["masked"]] == [3, 2]
    assert g["groups"].tolist() == [opt._flat[0]["tab"]["seg_grad"].data_ptr(), g["masked"][0].data_ptr(), 3,
                                    opt._flat[1]["tab"]["seg_grad"].data_ptr(), g["masked"][1].data_ptr(), 2]
    spans = sorted((t.data_ptr() - g["buf"].data_ptr(), t.data_ptr() - g["buf"].data_ptr() + 8 * t.numel())
                   for t in (g["counters"], g["flags"], g["groups"], *g["masked"]))
    assert spans == [(0, 40), (40, 80), (80, 128), (128, 152), (152, 168)]
    assert opt.last_step_skipped.shape == () and opt.skipped_steps.shape == () and opt.skipped_steps.dtype == torch.int64
    assert opt.last_step_skipped.data_ptr() == g["counters"].data_ptr() + 32 and opt.skipped_steps.data_ptr() == g["counters"].data_ptr() + 8
    assert opt.guard_report() == dict(guarded_steps=0, skipped_steps=0, first_skipped=None, last_skipped=None, nonfinite_params=[])
    g["counters"].copy_(torch.tensor([7, 2, 3, 6, 1]))
    g["flags"][3] = 1
    assert opt.guard_report() == dict(guarded_steps=7, skipped_steps=2, first_skipped=3, last_skipped=6, nonfinite_params=[3])
    saved = opt.snapshot()
    opt.reset_guard()
    assert opt.guard_report()["guarded_steps"] == 0 and int(opt.skipped_steps) == 0
    opt.restore(saved)                                                     # the counters are part of what a snapshot holds
    assert opt.guard_report() == dict(guarded_steps=7, skipped_steps=2, first_skipped=3, last_skipped=6, nonfinite_params=[3])
    opt.add_param_group(dict(params=[mk(8200)]))                           # a new layout: new tables, the counters carry over
    assert opt._guard["n_groups"] == 3 and [m.numel() for m in opt._guard["masked"]] == [3, 2, 1]
    assert opt._guard["counters"].tolist() == [7, 2, 3, 6, 1] and opt._guard["flags"].numel() == 6
    opt.max_grad_norm = 1.0                                                # clipping switched on later: the guard keeps its own buffers
    assert opt._clip is not None and opt._clip["buf"].data_ptr() != opt._guard["stats"]["buf"].data_ptr()


def test_step_on_cpu_parameters_still_raises():
    net = _net()
    opt = FusedAdamW(net.parameters(), capturable=True)
    opt.skip_nonfinite = True
    net(torch.randn(2, 7)).sum().backward()
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        opt.step()


def test_count_nonfinite_refuses_cpu_tensors_and_bad_records():
    rec, tick = torch.zeros(3, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        ops.count_nonfinite(torch.zeros(4), rec, tick)
    with pytest.raises(L.KanConvError, match="tensor"):
        ops.count_nonfinite([0.0], rec, tick)
    assert rec.tolist() == [0, 0, 0]


def _hip_names(model):
    from convkan_amd.layers.conv_layers import _HipLayer
    from convkan_amd.layers.head_layers import _CoeffKANLayer
    from convkan_amd.layers.mlp_layers import KANLayer
    return [n for n, m in model.named_modules() if isinstance(m, (_HipLayer, KANLayer, _CoeffKANLayer))]


@pytest.mark.parametrize("head", [dict(classifier_type="Linear"), dict(classifier_type="KAN", kan_classifier="KAN"),
                                  dict(classifier_type="HiddenKAN", kan_classifier="ChebyKAN")], ids=["linear", "kan", "chebykan"])
def test_probe_slots_and_hooks_on_a_cpu_model(head):
    torch.manual_seed(0)
    model = vggkan(3, 10, arch="VGG11", kan_conv="KAN", **head)
    names = _hip_names(model)
    convs = [f"features.{i}" for i, m in enumerate(model.features) if not isinstance(m, nn.MaxPool2d)]
    assert names[:8] == convs and len(convs) == 8                          # VGG11: eight conv layers, in forward order
    assert (len(names) > 8) == (head["classifier_type"] != "Linear")       # a KAN head adds its layers behind them
    before = {k: v.clone() for k, v in model.state_dict().items()}
    hooks_before = sum(len(m._forward_hooks) + len(m._forward_pre_hooks) for m in model.modules())
    probe = K.AnomalyProbe(model)
    assert probe.slots == [(n, d) for n in names + [ROOT_NAME] for d in ("forward", "backward")]
    assert probe.buffer.dtype == torch.int64 and probe.buffer.device.type == "cpu" and probe.buffer.numel() >= 1 + 3 * len(probe.slots)
    assert probe.tick.data_ptr() == probe.buffer.data_ptr() and probe.report() == []
    assert sum(len(m._forward_hooks) for m in model.modules()) == len(names) + 1 and len(model._forward_pre_hooks) == 1
    assert all(len(m._forward_hooks) == (1 if n in names or n == "" else 0) for n, m in model.named_modules())
    # the order report() promises: by first tick; forward slots in module order, then backward slots in reverse module order
    last = len(probe.slots) // 2 - 1
    for slot, (elements, first) in {0: (4, 2), 1: (1, 2), 2: (9, 2), 3: (2, 2), 2 * last: (5, 1), 2 * last + 1: (6, 2)}.items():
        probe.buffer[1 + 3 * slot:4 + 3 * slot] = torch.tensor([elements, first, first + 1])
    got = [(e["name"], e["direction"], e["elements"], e["first_tick"], e["last_tick"]) for e in probe.report()]
    assert got == [(ROOT_NAME, "forward", 5, 1, 2), (names[0], "forward", 4, 2, 3), (names[1], "forward", 9, 2, 3),
                   (ROOT_NAME, "backward", 6, 2, 3), (names[1], "backward", 2, 2, 3), (names[0], "backward", 1, 2, 3)]
    probe.reset()
    assert probe.report() == [] and int(probe.tick) == 0
    probe.remove()
    assert sum(len(m._forward_hooks) + len(m._forward_pre_hooks) for m in model.modules()) == hooks_before
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    with K.AnomalyProbe(model, backward=False) as p2:                      # a context manager; forward slots are listed either way
        assert len(model._forward_pre_hooks) == 1 and p2.backward is False
    assert sum(len(m._forward_hooks) + len(m._forward_pre_hooks) for m in model.modules()) == hooks_before

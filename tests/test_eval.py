"""The evaluation half of the training loop, off the device: the C ABI of the loss kernels is declared, bound and refuses bad arguments by
host arithmetic; the Python names exist and refuse what they do not implement; and ``ClassMetrics.summarize`` turns integer counters into
the figures the REFERENCE's ``evaluations.test`` returned for the fixtures of tests/golden/eval/ (make_golden_eval.py): both sides are fp64
arithmetic on the same integers, hence the 1e-12."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import convkan_amd as K
from convkan_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL = os.path.join(ROOT, "tests", "golden", "eval")
FIXTURES = sorted(f[:-4] for f in os.listdir(EVAL) if f.endswith(".npz")) if os.path.isdir(EVAL) else []
ENTRY_POINTS = ("kan_xent_workspace_bytes", "kan_xent_metrics_bytes", "kan_xent_fwd", "kan_xent_bwd")


def load_eval(name):
    return dict(np.load(os.path.join(EVAL, name + ".npz")))


def counters(logits, targets):
    """tp / pred / true per class and the correct count, in numpy; the prediction is the lowest index among the maxima (np.argmax, torch.max)."""
    Cn = logits.shape[1]
    pred = np.argmax(logits, axis=1)
    hit = pred == targets
    return (np.bincount(targets[hit], minlength=Cn), np.bincount(pred, minlength=Cn), np.bincount(targets, minlength=Cn), int(hit.sum()))


def test_fixture_set():
    assert len(FIXTURES) >= 3
    d = load_eval("c10_n37_b8")
    assert d["logits"].shape == (37, 10) and d["logits"].dtype == np.float32 and d["targets"].dtype == np.int64 and int(d["batch_size"]) == 8
    d = load_eval("c100_n50_b16")
    tp, pred, true, _ = counters(d["logits"], d["targets"])
    assert ((pred + true) == 0).any() and ((pred > 0) & (true == 0)).any() and ((pred == 0) & (true > 0)).any()
    d = load_eval("ties_c6_n20_b7")
    assert ((d["logits"] == d["logits"].max(1, keepdims=True)).sum(1) > 1).any()


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "kanconv.h")).read()
    declared = set(re.findall(r"\b(kan_[a-z_]+)\s*\(", header))
    for name in ENTRY_POINTS:
        assert name in declared and name in L.SIGNATURES, name
    K.build_library()
    lib = L.load()
    raw = C.CDLL(L.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), name
    assert lib.kan_xent_workspace_bytes(5) >= 5 * 4 and lib.kan_xent_workspace_bytes(0) == 0
    assert lib.kan_xent_metrics_bytes(10) == 8 * (L.XENT_HEADER_WORDS + 30) and lib.kan_xent_metrics_bytes(0) == 0
    for name in ("CrossEntropyLoss", "ClassMetrics", "evaluate", "train_and_test_models"):
        assert hasattr(K, name), name
    assert callable(K.ops.cross_entropy)
    assert list(inspect.signature(K.evaluate).parameters) == ["model", "batches", "device", "metrics"]
    assert list(inspect.signature(K.train_and_test_models).parameters)[:8] == [
        "model", "train_batches", "test_batches", "optimizer", "scheduler", "epochs", "reducer", "split_precision"]


def test_launchers_refuse_bad_arguments_without_a_device():
    K.build_library()
    lib = L.load()
    p, null, st = C.c_void_p(64), C.c_void_p(0), C.c_void_p(0)           # never dereferenced: every call below is refused before a launch

    def refused(rc, word):
        assert rc < 0
        msg = lib.kan_last_error().decode()
        assert word in msg, msg
    for i in (0, 1, 4, 5, 7):                                            # logits, target, loss, lse, workspace (metrics, index 6, may be null)
        args = [p, p, 4, 3, p, p, null, p, st]
        args[i] = null
        refused(lib.kan_xent_fwd(*args), "kan_xent_fwd: null pointer")
    refused(lib.kan_xent_fwd(p, p, 0, 3, p, p, null, p, st), "kan_xent_fwd: B and C")
    refused(lib.kan_xent_fwd(p, p, 4, 0, p, p, null, p, st), "kan_xent_fwd: B and C")
    for i in range(5):
        args = [p, p, p, p, p, 4, 3, st]
        args[i] = null
        refused(lib.kan_xent_bwd(*args), "kan_xent_bwd: null pointer")
    refused(lib.kan_xent_bwd(p, p, p, p, p, 0, 3, st), "kan_xent_bwd: B and C")
    refused(lib.kan_xent_bwd(p, p, p, p, p, 4, 0, st), "kan_xent_bwd: B and C")


@pytest.mark.parametrize("kwargs", [dict(label_smoothing=0.1), dict(weight=torch.ones(3)), dict(ignore_index=0), dict(reduction="sum"),
                                    dict(reduction="none"), dict(size_average=True), dict(reduce=False)],
                         ids=lambda k: next(iter(k)) + "=" + str(next(iter(k.values()))).replace(" ", ""))
def test_criterion_refuses_what_it_does_not_implement(kwargs):
    with pytest.raises(NotImplementedError):
        K.CrossEntropyLoss(**kwargs)


def test_criterion_and_op_have_no_cpu_fallback():
    crit = K.CrossEntropyLoss()
    assert crit.metrics is None and isinstance(crit, torch.nn.Module)
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        crit(torch.randn(4, 3), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        K.ops.cross_entropy(torch.randn(4, 3), torch.zeros(4, dtype=torch.int64))


def test_graphed_step_refuses_the_criterion():
    """Recording the loss kernels into a HIP graph is not supported: refused by name before anything runs, torch's criterion stays the default."""
    with pytest.raises(NotImplementedError, match="CrossEntropyLoss"):
        K.GraphedStep(torch.nn.Identity(), torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), criterion=K.CrossEntropyLoss())
    assert inspect.signature(K.GraphedStep.__init__).parameters["criterion"].default is None
    assert inspect.signature(K.train_step).parameters["criterion"].default is None


@pytest.mark.parametrize("name", FIXTURES)
def test_summarize_reproduces_the_reference(name):
    d = load_eval(name)
    logits, targets, bs = d["logits"], d["targets"], int(d["batch_size"])
    tp, pred, true, correct = counters(logits, targets)
    n = len(targets)
    batches = -(-n // bs)
    r = K.ClassMetrics.summarize(tp, pred, true, correct, n, batches, float(d["loss"]) * batches)
    for key in ("accuracy", "precision", "recall", "f1"):
        print(name, key, r[key], float(d[key]))
        assert abs(r[key] - float(d[key])) <= 1e-12, (key, r[key], float(d[key]))
    assert abs(r["loss"] - float(d["loss"])) <= 1e-12 and (r["samples"], r["batches"]) == (n, batches)
    # the same counters as torch tensors and as lists
    for conv in (lambda a: torch.from_numpy(a), lambda a: a.tolist()):
        assert K.ClassMetrics.summarize(conv(tp), conv(pred), conv(true), correct, n, batches, float(d["loss"]) * batches) == r


def test_summarize_macro_rule():
    """An absent class, a class that is only predicted and a class that is only a target: scikit-learn averages over the labels that occur
    in either vector (3 of 4 here), with 0 for a 0 / 0."""
    # targets [0, 0, 2, 0], predictions [0, 1, 0, 0]; class 3 absent
    r = K.ClassMetrics.summarize([2, 0, 0, 0], [3, 1, 0, 0], [3, 0, 1, 0], 2, 4, 1, 0.5)
    assert abs(r["precision"] - (2 / 3 + 0 + 0) / 3) <= 1e-15 and abs(r["recall"] - (2 / 3 + 0 + 0) / 3) <= 1e-15
    assert abs(r["f1"] - (4 / 6 + 0 + 0) / 3) <= 1e-15 and r["accuracy"] == 0.5 and r["loss"] == 0.5
    empty = K.ClassMetrics.summarize([0], [0], [0], 0, 0, 0, 0.0)
    assert empty["f1"] == 0.0 and empty["loss"] == 0.0 and empty["accuracy"] == 0.0

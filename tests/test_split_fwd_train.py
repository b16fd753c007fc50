"""CPU: the host side of the OPT-IN split-precision training forward (ops.split_precision_forward / split_precision_training) -- the
`split_precision` argument of the training harness (the switch and its contexts: tests/test_split_host.py)."""
import inspect

import pytest

import convkan_amd as K


@pytest.mark.parametrize("fn", [K.train_step, K.train_model_generic, K.GraphedStep], ids=lambda f: f.__name__)
def test_harness_takes_split_precision_off_by_default(fn):
    p = inspect.signature(fn).parameters["split_precision"]
    assert p.default is False

"""CPU: the host side of the OPT-IN split-precision training forward (ops.split_precision_forward / split_precision_training) -- the
flag and its two context managers, and the `split_precision` argument of the training harness."""
import inspect

import pytest

import convkan_amd as K
from convkan_amd import ops


def _flags():
    return ops._SPLIT_FWD, ops._SPLIT_BWD_DATA, ops._SPLIT_BWD_WEIGHT


def test_forward_context_sets_restores_and_nests():
    assert ops._SPLIT_FWD is False and ops._SPLIT_INFERENCE is False
    with ops.split_precision_forward():
        assert _flags() == (True, False, False) and ops._SPLIT_INFERENCE is False
        with ops.split_precision_forward():
            assert ops._SPLIT_FWD is True
        assert ops._SPLIT_FWD is True
    assert ops._SPLIT_FWD is False
    with pytest.raises(RuntimeError):
        with ops.split_precision_forward():
            raise RuntimeError("x")
    assert ops._SPLIT_FWD is False and ops._SPLIT_INFERENCE is False


def test_training_context_is_the_three_and_restores_what_it_found():
    assert _flags() == (False, False, False)
    with ops.split_precision_training():
        assert _flags() == (True, True, True) and ops._SPLIT_INFERENCE is False
        with ops.split_precision_training():
            assert _flags() == (True, True, True)
        assert _flags() == (True, True, True)
    assert _flags() == (False, False, False)
    with ops.split_precision_backward_data():                 # restores what it found, not False
        with pytest.raises(RuntimeError):
            with ops.split_precision_training():
                assert _flags() == (True, True, True)
                raise RuntimeError("x")
        assert _flags() == (False, True, False)
    assert _flags() == (False, False, False)
    with ops.split_precision_inference():                     # a switch of its own: neither set nor cleared
        with ops.split_precision_training():
            assert ops._SPLIT_INFERENCE is True
        assert ops._SPLIT_INFERENCE is True and _flags() == (False, False, False)
    assert ops._SPLIT_INFERENCE is False


@pytest.mark.parametrize("fn", [K.train_step, K.train_model_generic, K.GraphedStep], ids=lambda f: f.__name__)
def test_harness_takes_split_precision_off_by_default(fn):
    p = inspect.signature(fn).parameters["split_precision"]
    assert p.default is False

"""CPU: the host plumbing the three opt-in split-precision launches share (ops.py, section "opt-in split precision") -- the one switch
record and the six public contexts over it, the one scope rule against the library's three byte-count exports, the cut-weight cache class on stub functions,
and the per-stage decision with every switch off.  No device: the scope rule reads shapes, the cache is driven with CPU tensors."""
import ctypes as C
import dataclasses
import gc

import pytest
import torch

from convkan_amd import _lib as L
from convkan_amd import ops
from split_cells import OUT_OF_SCOPE, geom_basis, stage_spec

OFF = ops.SplitMode()
CONTEXTS = {"split_precision_inference": dict(inference=True),
            "split_precision_forward": dict(fwd=True),
            "split_precision_backward_data": dict(bwd_data=True),
            "split_precision_backward_weight": dict(bwd_weight=True),
            "split_precision_backward": dict(bwd_data=True, bwd_weight=True),
            "split_precision_training": dict(fwd=True, bwd_data=True, bwd_weight=True)}


# ------------------------------------------------------------------------------------------ the switch
def test_the_record_is_off_by_default_and_immutable():
    assert ops._SPLIT == OFF == ops.SplitMode(inference=False, fwd=False, bwd_data=False, bwd_weight=False)
    with pytest.raises(dataclasses.FrozenInstanceError):
        ops._SPLIT.fwd = True


@pytest.mark.parametrize("name", CONTEXTS)
def test_context_sets_its_fields_only_nests_and_restores_after_an_exception(name):
    ctx, want = getattr(ops, name), dataclasses.replace(OFF, **CONTEXTS[name])
    assert ops._SPLIT == OFF
    with ctx():
        assert ops._SPLIT == want                                 # its fields, and no other
        with ctx():
            assert ops._SPLIT == want
        assert ops._SPLIT == want
    assert ops._SPLIT == OFF
    with pytest.raises(RuntimeError):
        with ctx():
            assert ops._SPLIT == want
            raise RuntimeError("x")
    assert ops._SPLIT == OFF


@pytest.mark.parametrize("name", CONTEXTS)
@pytest.mark.parametrize("outer", CONTEXTS)
def test_context_restores_what_it_found_not_false(outer, name):
    """Every context inside every other: inside, the union of the two -- no context clears a field, so split_precision_training neither sets nor clears
    `inference` and split_precision_inference leaves the training fields alone --; afterwards what the outer one set, on a clean exit and on an exception."""
    found = dataclasses.replace(OFF, **CONTEXTS[outer])
    both = dataclasses.replace(found, **CONTEXTS[name])
    with getattr(ops, outer)():
        with getattr(ops, name)():
            assert ops._SPLIT == both
        assert ops._SPLIT == found
        with pytest.raises(RuntimeError):
            with getattr(ops, name)():
                assert ops._SPLIT == both
                raise RuntimeError("x")
        assert ops._SPLIT == found
    assert ops._SPLIT == OFF


# ------------------------------------------------------------------------------------------ the scope rule
def _byte_counts(geom, basis):
    lib = L.load()
    return tuple(getattr(lib, n)(C.byref(geom), C.byref(basis)) for n in
                 ("kan_split_weight_bytes", "kan_split_bwd_data_weight_bytes", "kan_split_bwd_weight_workspace_bytes"))


def test_scope_truth_table():
    """An in-scope stage (16 -> 128 channels, 8x8, B = 2, default B-spline spec with SiLU), then each host condition and each library condition flipped in turn:
    `_split_scope` refuses every one, and the three byte counts are nonzero exactly when it does not."""
    x, O_ = torch.empty(2, 16, 8, 8), 128                          # the rule reads shapes only
    scope = ops._split_scope(stage_spec(), x, None, None, O_)
    assert scope is not None and all(n > 0 for n in _byte_counts(*scope)), scope
    host = {"groups 2": (stage_spec(groups=2), x, None, None),
            "no base branch": (stage_spec(act="none"), x, None, None),
            "a second input": (stage_spec(), x, torch.empty_like(x), None),
            "a phase table": (stage_spec(), x, None, torch.empty(16, 2, 8)),
            "a 5-D x": (stage_spec(), torch.empty(2, 16, 8, 8, 8), None, None),
            "a plane window": (stage_spec(first=1), x, None, None),
            "W_IOD": (stage_spec(w_layout=ops.W_IOD), x, None, None)}
    for why, args in host.items():
        assert ops._split_scope(*args, O_) is None, why
    for kw in OUT_OF_SCOPE:
        kw = dict(dict(B=2, nb=8, act="silu"), **kw)
        assert ops._split_scope(stage_spec(kw["nb"], kw["act"]), torch.empty(kw["B"], kw["C_"], kw["H"], kw["H"]), None, None, kw["O_"]) is None, kw
        assert _byte_counts(*geom_basis(**kw)) == (0, 0, 0), kw


def test_public_entry_points_refuse_with_the_one_scope_sentence(monkeypatch):
    """The three refusals are one sentence (`_SPLIT_SCOPE`) behind the launch's name; KanConvError, "split-precision" in the message.  (`_require` is stepped
    over: it asks for device tensors, the refusal is host arithmetic.)"""
    monkeypatch.setattr(ops, "_require", lambda t, name: t)
    spec, x, dz = stage_spec(), torch.empty(3, 16, 8, 8), torch.empty(3, 128, 8, 8)      # odd batch on 8x8
    w = torch.empty(128, 16, 3, 3)
    for call, which in ((lambda: ops.kan_conv_fwd_split(spec, x, w, w), "forward"), (lambda: ops.kan_conv_bwd_data_split(spec, x, dz, w, w), "bwd-data"),
                        (lambda: ops.kan_conv_bwd_weight_split(spec, x, dz), "bwd-weight")):
        with pytest.raises(L.KanConvError) as e:
            call()
        assert str(e.value) == f"split-precision {which}: {ops._SPLIT_SCOPE} only"
    x = torch.empty(2, 16, 8, 8)                                   # their other refusals that need no device: the dz shape, NCHW
    for call in (lambda dz: ops.kan_conv_bwd_data_split(spec, x, dz, w, w), lambda dz: ops.kan_conv_bwd_weight_split(spec, x, dz)):
        with pytest.raises(L.KanConvError, match=r"split-precision bwd-\w+: dz \(2, 128, 8, 4\) != \(2, 128, 8, 8\)"):
            call(torch.empty(2, 128, 8, 4))
        with pytest.raises(L.KanConvError, match=r"split-precision bwd-\w+: NCHW x and dz"):
            call(torch.empty(128, 8, 8))


# ------------------------------------------------------------------------------------------ the cut-weight cache
def _stub_cache(size):
    packs = []
    return ops.CutWeightCache(lambda geom, basis: size[0], lambda geom, basis, wb, ws, buf: packs.append(buf.data_ptr())), packs


def test_cut_weight_cache_recuts_in_place_only_when_something_moved():
    size = [64]
    cache, packs = _stub_cache(size)
    wb, ws = torch.zeros(4), torch.zeros(8)
    get = lambda: cache.get(None, None, wb, ws)
    a = get()
    assert a.dtype == torch.uint8 and a.numel() == 64 and packs == [a.data_ptr()]
    assert get() is a and len(packs) == 1                          # nothing moved: no second cut
    ws.add_(1.0)                                                   # a version stamp moved: cut again, into the same buffer
    assert get() is a and packs == [a.data_ptr()] * 2
    ops.weights_changed()                                          # the epoch moved
    assert get() is a and len(packs) == 3
    assert get() is a and len(packs) == 3
    with ops.always_pack():                                        # a recorded step: every call cuts
        assert get() is a and get() is a and len(packs) == 5
    assert get() is a and packs == [a.data_ptr()] * 5
    size[0] = 128                                                  # another byte count: a new buffer, cut once
    b = get()
    assert b is not a and b.numel() == 128 and len(packs) == 6 and get() is b and len(packs) == 6
    assert len(cache.entries) == 1
    size[0] = 0                                                    # the launch does not take the stage
    assert get() is None and len(packs) == 6


def test_cut_weight_cache_is_lru_bounded_at_16_and_entries_die_with_their_weights():
    cache, packs = _stub_cache([16])
    assert cache.bound == 16 and ops._CUT_FWD.bound == 16 and ops._CUT_BWD_DATA.bound == 16 and ops._CUT_FWD is not ops._CUT_BWD_DATA
    pairs = [(torch.zeros(4), torch.zeros(4)) for _ in range(18)]
    key = lambda p: (p[0].data_ptr(), p[1].data_ptr(), None)       # (addresses, device index)
    for p in pairs[:16]:
        cache.get(None, None, *p)
    assert [k for k in cache.entries] == [key(p) for p in pairs[:16]]
    cache.get(None, None, *pairs[0])                               # used again: now the newest
    cache.get(None, None, *pairs[16])                              # the 17th pair evicts the oldest, which is pair 1
    assert len(cache.entries) == 16 and key(pairs[1]) not in cache.entries and key(pairs[0]) in cache.entries and key(pairs[16]) in cache.entries
    cache.get(None, None, *pairs[17])
    assert len(cache.entries) == 16 and key(pairs[2]) not in cache.entries and key(pairs[0]) in cache.entries
    assert len(packs) == 18                                        # the second use of pair 0 cut nothing
    gone = key(pairs[5])
    assert gone in cache.entries
    del pairs[5]
    gc.collect()
    assert gone not in cache.entries and len(cache.entries) == 15


# ------------------------------------------------------------------------------------------ the decision
def test_switches_off_decide_nothing_without_a_plan_lookup_or_a_library_call(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("a plan lookup or a library call")
    monkeypatch.setattr(ops, "_plan_cached", touched)
    monkeypatch.setattr(L, "load", touched)
    spec, x = stage_spec(), torch.empty(2, 16, 8, 8)
    w_base, w_basis = [torch.empty(128, 16, 3, 3)], [torch.empty(128, 128, 3, 3)]
    nothing = ops.SplitStage(z=None, wcd=None, dw_split=False)
    assert ops._SPLIT == OFF
    assert ops._split_decision(spec, x, None, None, w_base, w_basis, False, True, True) == nothing
    with ops.split_precision_inference():                          # the caller turns this one into want_fwd, under no_grad only
        assert ops._split_decision(spec, x, None, None, w_base, w_basis, False, True, True) == nothing
    with ops.split_precision_backward():                           # on, but no gradient to compute
        assert ops._split_decision(spec, x, None, None, w_base, w_basis, False, False, False) == nothing
        with pytest.raises(AssertionError, match="a plan lookup"):                      # (the traps do catch a decision that goes on)
            ops._split_decision(spec, x, None, None, w_base, w_basis, False, True, False)
    with pytest.raises(AssertionError, match="a plan lookup"):
        ops._split_decision(spec, x, None, None, w_base, w_basis, True, False, False)

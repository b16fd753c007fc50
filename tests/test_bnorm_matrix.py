"""CPU: what the BatchNorm tail (csrc/kan_bnorm.hip) rests on before any GPU runs.

(a) every row of tests/bnorm_cells.py keeps the share of outputs its conditioning masks under MASK_CAP, from the fp64 reference alone;
(b) the header, the ctypes signatures and the built library all carry the three kan_batchnorm* entry points, and the host-side
    argument checks of the two launchers refuse what they must before anything is launched;
(c) `_fusable_batchnorm` accepts exactly the module configurations the kernels implement: plain BatchNorm1d/2d/3d with a numeric
    momentum, all groups alike -- and leaves momentum=None and every other norm class to torch."""
import ctypes
import os
import re

import pytest
import torch.nn as nn

import convkan_amd as K
from bnorm_cells import BNORM_CASES, MASK_CAP, case_id, mask_share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("kan_batchnorm_workspace_bytes", "kan_batchnorm_prelu_fwd", "kan_batchnorm_prelu_bwd")


@pytest.mark.parametrize("case", BNORM_CASES, ids=case_id)
def test_mask_share_under_cap(case):
    share, count, total = mask_share(case)
    print(f"[bnorm mask] {case_id(case)}: {count} of {total} outputs masked")
    assert share <= MASK_CAP, f"{case}: {share:.3%} of the outputs are masked (cap {MASK_CAP:.0%}): give the row another seed"


def test_rows_are_the_specified_shapes():
    shapes = [(c["B"], c["C"], c["H"], c["W"], c["S"], c["groups"], c["pool"], c["training"]) for c in BNORM_CASES]
    assert shapes == [(3, 7, 1, 1, 1, 1, None, True), (5, 6, 2, 2, 1, 2, None, True), (3, 9, 3, 3, 2, 3, None, True), (3, 7, 5, 13, 5, 1, None, True),
                      (70, 3, 2, 2, 1, 1, None, True), (2, 5, 33, 35, 3, 1, None, True), (3, 7, 2, 2, 4, 1, (2, 2), True),
                      (5, 6, 4, 4, 1, 2, (2, 2), True), (3, 9, 6, 6, 1, 3, (2, 2), True), (2, 5, 34, 36, 2, 1, (2, 2), True),
                      (3, 7, 4, 4, 1, 1, None, False), (3, 7, 6, 6, 2, 1, (2, 2), False), (2, 130, 8, 8, 1, 1, (2, 2), True)]
    assert {c["affine"] for c in BNORM_CASES} == {"", "gb", "GB"} and {c["slope"] for c in BNORM_CASES} == {"", "+", "-"}
    assert any(not c["track"] for c in BNORM_CASES) and sum(c["kind"] == "unaligned" for c in BNORM_CASES) == 1


def test_entry_points_in_header_signatures_and_library():
    from convkan_amd import _lib as L
    K.build_library()
    header = open(os.path.join(ROOT, "include", "kanconv.h")).read()
    declared = set(re.findall(r"\b(kan_[a-z_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared and name in L.SIGNATURES and hasattr(raw, name), name
    for name in ENTRY_POINTS[1:]:                                         # each declaration's comment cites the reference lines it replaces
        comment = header[header.rindex("/*", 0, header.index("int " + name)):header.index("int " + name)]
        assert "kan_layers.py:241-243" in comment and "norm_layer=BatchNorm2d" in comment and "train.py:67-68" in comment, name


def test_workspace_and_argument_checks():
    """Host arithmetic only: every call below is refused before a launch (no GPU is touched)."""
    from convkan_amd import _lib as L
    K.build_library()
    lib = L.load()
    assert lib.kan_batchnorm_workspace_bytes(0, 4) == 0
    assert lib.kan_batchnorm_workspace_bytes(3, 7) >= 3 * 7 * 5 * 8          # five doubles per (b, channel) plane
    p = ctypes.c_void_p(4096)                                             # never dereferenced: the checks fail first
    null = ctypes.c_void_p(0)
    fwd = lambda **kw: lib.kan_batchnorm_prelu_fwd(*(dict(z=p, n_slabs=1, slab=0, z_out=p, gamma=null, beta=null, a=null, y=p, pidx=null, mean=p, rstd=p,
                                                          rm=null, rv=null, ws=p, B=2, Cn=4, H=4, W=4, bs=64, eps=1e-5, mom=0.1, span=0, training=1, st=null) | kw).values())
    bwd = lambda **kw: lib.kan_batchnorm_prelu_bwd(*(dict(dy=p, pidx=null, z=p, mean=p, rstd=p, gamma=null, beta=null, a=null, dz=p, dg=null, db=null, dp=null,
                                                          ws=p, B=2, Cn=4, H=4, W=4, bs=64, span=0, training=1, st=null) | kw).values())
    for bad in (dict(ws=null), dict(z=null), dict(n_slabs=0), dict(B=0), dict(bs=63), dict(pidx=p, H=3), dict(rm=p), dict(span=3),
                dict(B=1, H=1, W=1, bs=4)):
        assert fwd(**bad) != 0, bad
        assert lib.kan_last_error()
    for bad in (dict(ws=null), dict(dz=null), dict(Cn=0), dict(bs=63), dict(pidx=p, W=5), dict(span=3), dict(dp=p)):
        assert bwd(**bad) != 0, bad


def _mods(cls, n=2, ch=4, **kw):
    return nn.ModuleList([cls(ch, **kw) for _ in range(n)])


def test_fusable_batchnorm_accepts_and_refuses():
    from convkan_amd.layers.conv_layers import _fusable_batchnorm, _fusable_instnorm
    for cls in (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d):
        assert _fusable_batchnorm(_mods(cls))
        assert _fusable_batchnorm(_mods(cls, n=1, affine=False, track_running_stats=False, momentum=0.3, eps=1e-3))
        assert not _fusable_instnorm(_mods(cls))
    assert not _fusable_batchnorm(_mods(nn.BatchNorm2d, momentum=None)), "the cumulative average stays with torch"
    for other in (_mods(nn.InstanceNorm2d), _mods(nn.SyncBatchNorm), nn.ModuleList([nn.GroupNorm(2, 4)]), nn.ModuleList([nn.LayerNorm(4)]),
                  nn.ModuleList([nn.LazyBatchNorm2d()])):
        assert not _fusable_batchnorm(other), type(other[0]).__name__

    class MyNorm(nn.BatchNorm2d):
        pass
    assert not _fusable_batchnorm(_mods(MyNorm)), "a subclass may override forward: the caller's own module"
    for attr, value in (("eps", 1e-3), ("momentum", 0.2), ("affine", False), ("track_running_stats", False)):
        mixed = nn.ModuleList([nn.BatchNorm2d(4), nn.BatchNorm2d(4, **{attr: value})])
        assert not _fusable_batchnorm(mixed), f"groups differ in {attr}"
    stripped = _mods(nn.BatchNorm2d, n=1)
    stripped[0].running_mean = stripped[0].running_var = None                # flag and buffers disagree: torch decides
    assert not _fusable_batchnorm(stripped)

"""The persistent packed weights on the GPU, bit for bit (tests/pack_cells.py; the CPU half is tests/test_pack_cache.py).

Through the C ABI, with the ring, both layouts and the weights between sentinel words: (4) the fingerprint k_fingerprint leaves in the ring against the
numpy reference, over ragged, tiny, many-block and grid-stride sizes and four sample strides; (5) the early exit of k_pack and of k_pack_bwd_data -- an
unchanged call writes no word of wp or wd, a 1-ulp change re-packs both; (6) the claim of ops._layout_key that input shapes of one key share their
packed bytes.  Through the layers: (7) after every kind of weight write -- those the host stamps see, those only the fingerprint sees, and raw writes
under a verification cadence -- the step equals the same layer's step with the cache off, and the cached layouts equal a fresh pack."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from pack_cells import BIG_ROW, CLASS_ROWS, PACK_CASES, RAGGED_ROWS, counts, fingerprint_ref, fingerprint_ref_torch, ring_totals, structs
from route_cells import case_layer, route_key
from split_cells import same_but_slopes

pytestmark = pytest.mark.gpu

PAD = 64                                              # guard words on either side: a multiple of four, so the views stay 16-byte aligned
SENT = 0x5A5AA5A5
FILL_A, FILL_B = 0x7FC0A5A5, 0x7FC05A5A              # what a layout holds before a pack: two different NaNs, so equal results were written whole
SPECIALS = (0x80000000, 0x00000001, 0x7F800000, 0x7FC12345)       # -0.0, the smallest denormal, inf, a NaN with a payload
STRIDES = (1, 2, 3, 7)


# ------------------------------------------------------------------------------------------------ guarded buffers and the C ABI
def _i32(v):
    return v - (1 << 32) if v >= 1 << 31 else v


def _guarded(words, fill=SENT):
    """(buffer, view): `words` int32 words placed PAD words into a larger buffer; buffer and view start out as `SENT` / `fill`."""
    buf = torch.full((words + 2 * PAD,), _i32(SENT), dtype=torch.int32, device="cuda")
    view = buf[PAD:PAD + words]
    assert view.data_ptr() % 16 == 0
    if fill != SENT:
        view.fill_(_i32(fill))
    return buf, view


def _intact(*bufs):
    return all(bool((b[:PAD] == _i32(SENT)).all()) and bool((b[-PAD:] == _i32(SENT)).all()) for b in bufs)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Weights:
    """The two reference-layout weight tensors of a row as guarded int32 views (`a` None without a base branch), with a host copy of their bits."""

    def __init__(self, g, b, seed, specials=True, device_only=False):
        self.na, self.nb = counts(g, b)
        self.bufs, self.host = [], []
        rng = np.random.default_rng(seed)
        views = []
        for n in (self.na, self.nb):
            if n == 0:
                views.append(None)
                self.host.append(None)
                continue
            buf, view = _guarded(n)
            if device_only:                           # the one large row: drawn on the device, never copied to the host
                view.view(torch.float32).normal_(generator=torch.Generator(device="cuda").manual_seed(seed + n))
                bits = None
            else:
                bits = (rng.standard_normal(n) * 0.1).astype(np.float32).view(np.uint32)
            if specials:                              # spread over the tensor, first and last element included
                for k, s in enumerate(SPECIALS):
                    i = (k * (n - 1)) // (len(SPECIALS) - 1)
                    if bits is None:
                        view[i] = _i32(s)
                    else:
                        bits[i] = s
            if bits is not None:
                view.copy_(torch.from_numpy(bits.view(np.int32)))
            self.bufs.append(buf)
            views.append(view)
            self.host.append(bits)
        self.a, self.b = views

    def bump(self, which, i):
        """1 ulp on element i of the base (`which` 0) or the basis (1) tensor, on the device and in the host copy."""
        view = (self.a, self.b)[which]
        view[i] += 1
        if self.host[which] is not None:
            self.host[which][i] += np.uint32(1)

    def ref(self, stride):
        if self.host[1] is None:
            return fingerprint_ref_torch(self.a, self.b, stride)
        return fingerprint_ref(self.host[0], self.host[1], stride)


def _pack_fresh(lib, W, g, b, p, fill):
    """kan_pack_weights into guarded layouts that held `fill`: the (wp, wd) views."""
    from convkan_amd import _lib as L
    bwp, wp = _guarded(p.packed_weight_bytes // 4, fill)
    bwd, wd = _guarded(p.bwd_data_weight_bytes // 4, fill)
    L.check(lib.kan_pack_weights(_ptr(W.a), _ptr(W.b), _ptr(wp), _ptr(wd), C.byref(g), C.byref(b), _stream()), "kan_pack_weights")
    torch.cuda.synchronize()
    assert _intact(bwp, bwd, *W.bufs)
    return wp, wd


def _pack_cached(lib, W, wp, wd, g, b, ring, cur, force, stride=1):
    from convkan_amd import _lib as L
    L.check(lib.kan_pack_weights_cached(_ptr(W.a), _ptr(W.b), _ptr(wp), _ptr(wd), C.byref(g), C.byref(b), _ptr(ring), cur, force, stride, _stream()),
            "kan_pack_weights_cached")
    torch.cuda.synchronize()


def _ring():
    from convkan_amd import _lib as L
    buf, view = _guarded(2 * L.KAN_FP_WORDS, 0)
    return buf, view.view(torch.int64)


# ------------------------------------------------------------------------------------------------ (4) fingerprint values
FP_CASES = [(n, s) for n in PACK_CASES if n != BIG_ROW for s in STRIDES] + [(BIG_ROW, 1)]        # the grid-stride row at stride 1 only


@pytest.mark.parametrize("name,stride", FP_CASES, ids=[f"{n}-stride{s}" for n, s in FP_CASES])
def test_fingerprint_values(name, stride, gpu_lib):
    """The protocol of include/kanconv.h: ring zero before the first call, cur = 0, 1, 2, 0, 1.  After every call slot cur holds the reference's two
    sums, slot cur + 1 is zero in every word (so the second lap adds into clean slots), slot cur - 1 still holds the previous call's, and nothing
    next to the ring, the weights or wp was written.  One element moves by 1 ulp between calls: the first, the last, one of a ragged tail."""
    g, b, p = structs(name)
    W = Weights(g, b, seed=11, device_only=name == BIG_ROW)
    bring, ring = _ring()
    bwp, wp = _guarded(p.packed_weight_bytes // 4, FILL_A)
    moves = [None, (1, 0), (1, W.nb - 1), (0, W.na - 1) if W.na else (1, W.nb - 2), (1, W.nb // 2)]
    prev = None
    for call, cur in enumerate((0, 1, 2, 0, 1)):
        if moves[call] is not None:
            W.bump(*moves[call])
        _pack_cached(gpu_lib, W, wp, None, g, b, ring, cur, 0, stride)
        want = W.ref(stride)
        print(f"{name} stride {stride} call {call}: slot {cur} = {ring_totals(ring, cur)}, reference {want}")
        assert ring_totals(ring, cur) == want, f"call {call}, slot {cur}"
        assert not bool(ring[((cur + 1) % 3) * 64:((cur + 1) % 3 + 1) * 64].any()), f"call {call}: slot {(cur + 1) % 3} is not clear"
        if prev is not None:
            assert ring_totals(ring, (cur + 2) % 3) == prev, f"call {call}: slot {(cur + 2) % 3} moved"
        assert _intact(bring, bwp, *W.bufs), f"call {call}: a guard word was written"
        prev = want


# ------------------------------------------------------------------------------------------------ (5) the early exit of both pack kernels
def _bits_equal(x, y):
    return x.shape == y.shape and bool((x == y).all())


def _all(view, value):
    return bool((view == _i32(value)).all())


EXIT_ROWS = list(CLASS_ROWS) + list(RAGGED_ROWS)


@pytest.mark.parametrize("where", ["last_basis", "base"])
@pytest.mark.parametrize("name", EXIT_ROWS)
def test_unchanged_call_writes_nothing_and_one_ulp_repacks_both(name, where, gpu_lib):
    g, b, p = structs(name)
    W = Weights(g, b, seed=23, specials=False)
    bring, ring = _ring()
    bwp, wp = _guarded(p.packed_weight_bytes // 4, FILL_A)
    bwd, wd = _guarded(p.bwd_data_weight_bytes // 4, FILL_A)
    ok = lambda: _intact(bring, bwp, bwd, *W.bufs)

    _pack_cached(gpu_lib, W, wp, wd, g, b, ring, 0, 1)                               # call 1, forced
    wp0, wd0 = _pack_fresh(gpu_lib, W, g, b, p, FILL_B)
    assert _bits_equal(wp, wp0) and _bits_equal(wd, wd0) and ok(), "forced cached pack differs from kan_pack_weights"
    wp.fill_(_i32(SENT))
    wd.fill_(_i32(SENT))
    _pack_cached(gpu_lib, W, wp, wd, g, b, ring, 1, 0)                               # call 2, unchanged
    assert _all(wp, SENT) and ok(), "k_pack wrote although the weights are unchanged"
    assert _all(wd, SENT), "k_pack_bwd_data wrote although the weights are unchanged"
    if where == "base" and W.na:
        W.bump(0, W.na // 2)
    else:                                                                            # no base branch: the first basis element instead
        W.bump(1, W.nb - 1 if where == "last_basis" else 0)
    _pack_cached(gpu_lib, W, wp, wd, g, b, ring, 2, 0)                               # call 3: seen by the fingerprint alone
    wp1, wd1 = _pack_fresh(gpu_lib, W, g, b, p, FILL_B)
    assert not _bits_equal(wp1, wp0) and not _bits_equal(wd1, wd0)                   # the changed weight shows in both layouts
    assert _bits_equal(wp, wp1) and ok(), "wp was not re-packed after a 1-ulp change"
    assert _bits_equal(wd, wd1), "wd was not re-packed after a 1-ulp change"
    wp.fill_(_i32(SENT))
    wd.fill_(_i32(SENT))
    _pack_cached(gpu_lib, W, wp, wd, g, b, ring, 0, 0)                               # call 4, unchanged again (second lap of the ring)
    assert _all(wp, SENT) and _all(wd, SENT) and ok(), "an unchanged call on the ring's second lap wrote"


@pytest.mark.parametrize("name", ["halo", "tap", "kan_na594", "cheby_nb10"])
def test_bwd_data_layout_wanted_later_needs_force(name, gpu_lib):
    """wd = NULL, then a call that wants it: as the header says it must pass force -- an unforced call on unchanged weights leaves wd alone (both
    kernels exit), the forced one fills it; wp is right throughout."""
    g, b, p = structs(name)
    W = Weights(g, b, seed=29, specials=False)
    bring, ring = _ring()
    bwp, wp = _guarded(p.packed_weight_bytes // 4, FILL_A)
    bwd, wd = _guarded(p.bwd_data_weight_bytes // 4)
    wp0, wd0 = _pack_fresh(gpu_lib, W, g, b, p, FILL_B)
    _pack_cached(gpu_lib, W, wp, None, g, b, ring, 0, 1)
    assert _bits_equal(wp, wp0) and _all(wd, SENT)
    _pack_cached(gpu_lib, W, wp, wd, g, b, ring, 1, 0)
    assert _bits_equal(wp, wp0) and _all(wd, SENT)
    _pack_cached(gpu_lib, W, wp, wd, g, b, ring, 2, 1)
    assert _bits_equal(wp, wp0) and _bits_equal(wd, wd0) and _intact(bring, bwp, bwd, *W.bufs)


# ------------------------------------------------------------------------------------------------ (6) what the layout key leaves out
KEY_GRID = [(B, H, W) for B in (1, 2, 8, 16, 17, 32, 128) for H, W in ((2, 2), (3, 3), (4, 4), (8, 8), (16, 16), (4, 8))]


@pytest.mark.parametrize("name", list(CLASS_ROWS))
def test_input_shapes_of_one_layout_key_share_their_packed_bytes(name, gpu_lib):
    """ops._layout_key holds no batch size and no resolution: every (B, H, W) of the grid that plans to the same key -- whatever route it takes --
    must pack the same weights to the same bytes, wp and wd, or one cache entry could not serve them all."""
    from convkan_amd import _lib as L
    from convkan_amd import ops
    case = PACK_CASES[name]
    spec = case_layer(case).conv_spec()
    W = None
    groups = {}
    for B, H, Wd in KEY_GRID:
        try:
            g, b, p = ops._plan_cached(spec, B, case["C"], H, Wd, case["O"], case["C"], case["O"])
        except L.KanConvError:
            continue
        if not gpu_lib.kan_pack_cacheable(C.byref(g), C.byref(b)):
            continue                                  # never looked up in ops._PACKED
        W = W or Weights(g, b, seed=31, specials=False)
        groups.setdefault(ops._layout_key(spec, g, p), []).append(((B, H, Wd), route_key(g, b, p)[1], g, b, p))
    assert groups and max(len(v) for v in groups.values()) > 1, "no two shapes of the grid share a key: nothing was compared"
    for key, members in groups.items():
        first = None
        for shape, fwd, g, b, p in members:
            wp, wd = _pack_fresh(gpu_lib, W, g, b, p, FILL_A)
            if first is None:
                first = (shape, fwd, wp, wd)
                continue
            assert _bits_equal(wp, first[2]), f"wp of {shape} ({fwd}) differs from {first[0]} ({first[1]}) under one layout key"
            assert _bits_equal(wd, first[3]), f"wd of {shape} ({fwd}) differs from {first[0]} ({first[1]}) under one layout key"


def test_some_layer_has_more_than_one_layout_key(gpu_lib):
    """The grid is no single-key grid: the 128 -> 96 layer takes band order on 3x3 and 4x4 planes and tap-major order on 2x2 planes of 16 images."""
    from convkan_amd import ops
    case = PACK_CASES["band_1m"]
    spec = case_layer(case).conv_spec()
    keys = {ops._layout_key(spec, *ops._plan_cached(spec, B, 128, H, H, 96, 128, 96)[::2]) for B, H in ((16, 2), (16, 3), (16, 4))}
    assert len(keys) == 2


# ------------------------------------------------------------------------------------------------ (7) coherence through the layers
@pytest.fixture
def pack_ops(gpu_lib, monkeypatch):
    """ops with an empty cache, zeroed counters and the default knobs; everything as it was afterwards."""
    from convkan_amd import ops
    kept, stats = list(ops._PACKED.items()), dict(ops.PACK_STATS)
    ops._PACKED.clear()
    ops.PACK_STATS.update(calls=0, forced=0, skipped=0)
    for knob, value in (("_PACK_CACHE_MAX", 256), ("_PACK_CACHE_BYTES", 16 << 30), ("_PACK_SAMPLE", 1), ("_PACK_VERIFY_EVERY", 16), ("_ALWAYS_PACK", False)):
        monkeypatch.setattr(ops, knob, value)
    yield ops
    ops._PACKED.clear()
    ops._PACKED.update(kept)
    ops.PACK_STATS.update(stats)


@contextlib.contextmanager
def _cache_off(ops):
    keep, ops._PACK_CACHE_MAX = ops._PACK_CACHE_MAX, 0
    try:
        yield
    finally:
        ops._PACK_CACHE_MAX = keep


LAYER_ROWS = ["band_1m", "halo", "halo_cheby", "halo_rb", "expanded", "tap_pm", "tap", "conv1d"]


def _build(name, seed):
    """(layer, x, grad of the output) on the GPU.  conv1d: a KANConv1DLayer, whose weights reach ops as `weight.unsqueeze(2)` views."""
    import convkan_amd as K
    from convkan_amd import ops
    torch.manual_seed(seed)
    if name == "conv1d":
        layer, shape = K.KANConv1DLayer(4, 128, 3, padding=1).cuda(), (4, 4, 16)
    else:
        # plain InstanceNorm: the affine norm's dgamma / dbeta are float-atomic sums that differ in their last bits between any two runs
        # (DESIGN.md section 2), and the norm is no part of what is cached
        case = dict(PACK_CASES[name], affine=False)
        layer, shape = case_layer(case).cuda(), (case["B"], case["C"], case["H"], case["W"])
    x = torch.randn(shape, device="cuda")
    with torch.no_grad(), _cache_off(ops):
        go = torch.randn_like(layer(x))
    return layer, x, go


def _conv_weights(layer):
    return [p for p in layer.parameters() if p.dim() >= 3]


def _step(layer, x, go):
    layer.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    y = layer(xg)
    y.backward(go)
    torch.cuda.synchronize()
    return y.detach().clone(), xg.grad.clone(), {n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None}


def _poison(nbytes):
    """A layout that is never written must not be right by accident: torch.empty hands out the blocks freed last, which may hold this very layout
    from an earlier pack.  Take the free blocks of that size, fill them with NaNs and give them back."""
    blocks = [torch.full((n // 4,), float("nan"), device="cuda") for n in nbytes for _ in range(4)]
    torch.cuda.synchronize()
    del blocks


def _geometry(ops, layer, x):
    """(geom, basis, plan, layout key) of the layer's conv stage on input x, as ops plans it."""
    x4 = x.unsqueeze(2) if x.dim() == 3 else x
    spec, O = layer.conv_spec(), _conv_weights(layer)[-1].shape[0]
    g, b, p = ops._plan_cached(spec, x4.shape[0], x4.shape[1], x4.shape[2], x4.shape[3], O, x4.shape[1], O)
    return g, b, p, ops._layout_key(spec, g, p)


def _entry_is_current(ops, layer, xs, what):
    """The cache holds one entry per layout key of the inputs `xs`, and each one's layouts equal kan_pack_weights of the weights as they are now."""
    from convkan_amd import _lib as L
    lib = L.load()
    ws = _conv_weights(layer)
    wb, wbasis = (ws[0], ws[1]) if layer.conv_spec().has_base else (None, ws[0])
    assert wb is None or wbasis.shape[1] == wb.shape[1] * layer.conv_spec().n_basis
    geoms = {}
    for x in xs:
        g, b, p, key = _geometry(ops, layer, x)
        geoms.setdefault(key, (g, b, p))
    assert len(ops._PACKED) == len(geoms), f"{what}: {len(ops._PACKED)} cache entries for {len(geoms)} layout keys"
    for key, ent in ops._PACKED.items():
        g, b, p = geoms[key[0]]
        wp = torch.empty(p.packed_weight_bytes // 4, device="cuda")
        wd = torch.empty(p.bwd_data_weight_bytes // 4, device="cuda") if ent.wd is not None else None
        L.check(lib.kan_pack_weights(_ptr(wb), _ptr(wbasis), _ptr(wp), _ptr(wd), C.byref(g), C.byref(b), _stream()), "kan_pack_weights")
        torch.cuda.synchronize()
        assert _bits_equal(ent.wp.view(torch.int32), wp.view(torch.int32)), f"{what}: the cached wp is not a pack of the current weights"
        assert wd is None or _bits_equal(ent.wd.view(torch.int32), wd.view(torch.int32)), f"{what}: the cached wd is not a pack of the current weights"


def _check(ops, layer, x, go, what):
    """One cached step, then the same step with the cache off: y, dx and every gradient bit for bit (scalar PReLU slopes as same_but_slopes judges)."""
    got = _step(layer, x, go)
    if _aligned(layer):                               # (weights that are not 16-byte aligned are packed afresh on every call and leave the cache alone)
        _entry_is_current(ops, layer, [x], what)
    with _cache_off(ops):
        ref = _step(layer, x, go)
    assert torch.equal(got[0], ref[0]), f"{what}: y differs from the uncached layer"
    assert torch.equal(got[1], ref[1]), f"{what}: dx differs from the uncached layer"
    assert got[2].keys() == ref[2].keys()
    same_but_slopes(ref[2], got[2], list(ref[2]))
    return got


def _stats(ops):
    return tuple(ops.PACK_STATS[k] for k in ("calls", "forced", "skipped"))


def _aligned(layer):
    return all(p.data_ptr() % 16 == 0 for p in _conv_weights(layer))


def _plan_bytes(ops, layer, x):
    p = _geometry(ops, layer, x)[2]
    return p.packed_weight_bytes, p.bwd_data_weight_bytes


@pytest.mark.parametrize("name", LAYER_ROWS)
def test_writes_the_host_sees(name, pack_ops):
    import convkan_amd as K
    ops = pack_ops
    layer, x, go = _build(name, seed=41)
    ws = _conv_weights(layer)
    _poison(_plan_bytes(ops, layer, x))
    with torch.no_grad():
        layer(x)                                                                     # an entry without the bwd-data layout ...
    assert _stats(ops) == (1, 1, 0) and len(ops._PACKED) == 1
    _poison(_plan_bytes(ops, layer, x))
    last = _check(ops, layer, x, go, "first training step")                          # ... which the first training step wants: forced
    assert _stats(ops) == (2, 2, 0)
    _check(ops, layer, x, go, "unchanged")
    assert _stats(ops) == (2, 2, 1)                                                  # stamps unchanged, verified recently: no launch at all

    def inplace():
        with torch.no_grad():
            for w in ws:
                w.add_(0.02 * torch.randn_like(w))

    def sgd():
        torch.optim.SGD(layer.parameters(), lr=0.05).step()                          # the gradients of the last step

    def adamw():
        torch.optim.AdamW(layer.parameters(), lr=1e-2, foreach=True).step()

    def load():
        sd = {k: (v + 0.02 * torch.randn_like(v) if v.dim() >= 3 and v.is_floating_point() else v.clone()) for k, v in layer.state_dict().items()}
        layer.load_state_dict(sd)

    def swap():
        for w in ws:
            w.data = w.data + 0.02 * torch.randn_like(w)                             # new storage behind the same Parameter

    def vector():
        vec = torch.nn.utils.parameters_to_vector(layer.parameters())
        torch.nn.utils.vector_to_parameters(vec + 0.02 * torch.randn_like(vec), layer.parameters())      # views into one new vector

    fused = {}

    def fused_take():
        fused["opt"] = K.FusedAdamW(layer.parameters(), lr=1e-2)                     # parameters move into the optimizer's flat block

    def fused_step():
        fused["opt"].step()

    for what, write, changes in (("in-place op under no_grad", inplace, True), ("torch.optim.SGD", sgd, True), ("torch.optim.AdamW(foreach=True)", adamw, True),
                                 ("load_state_dict", load, True), ("p.data = other", swap, True), ("vector_to_parameters", vector, True),
                                 ("FusedAdamW takes the parameters", fused_take, False), ("FusedAdamW.step", fused_step, True)):
        write()
        before, was_aligned = _stats(ops), _aligned(layer)
        got = _check(ops, layer, x, go, what)
        if changes:
            assert not torch.equal(got[1], last[1]), f"{what}: the write did not change dx -- the comparison shows nothing"
        if was_aligned and _aligned(layer):                                          # (an unaligned view is packed afresh on every call, uncounted)
            assert _stats(ops) == (before[0] + 1, before[1] + 1, before[2]), f"{what}: {before} -> {_stats(ops)}, expected one forced pack"
        last = got


@pytest.mark.parametrize("name", LAYER_ROWS)
def test_writes_only_the_fingerprint_sees(name, pack_ops, monkeypatch):
    ops = pack_ops
    monkeypatch.setattr(ops, "_PACK_VERIFY_EVERY", 1)
    layer, x, go = _build(name, seed=43)
    ws = _conv_weights(layer)
    _poison(_plan_bytes(ops, layer, x))
    last = _check(ops, layer, x, go, "first step")
    assert _stats(ops) == (1, 1, 0)
    _check(ops, layer, x, go, "unchanged")
    assert _stats(ops) == (2, 1, 0)

    def mul2():
        for w in ws:
            w.data.mul_(2.0)

    def neg():
        for w in ws:
            w.data.neg_()

    def ulp():
        ws[-1].data.view(-1)[-1:].view(torch.int32).add_(1)

    def permute():
        for w in ws:
            w.data.copy_(w.data[torch.randperm(w.shape[0], device=w.device)])

    for what, write, visible in ((".data.mul_(2.0)", mul2, True), (".data.neg_()", neg, True), ("1 ulp on the last element", ulp, False),
                                 ("row permutation through .data.copy_", permute, True)):
        versions = [w._version for w in ws]
        write()
        assert [w._version for w in ws] == versions, f"{what}: the version counter moved -- not the write this test is about"
        before = _stats(ops)
        got = _check(ops, layer, x, go, what)
        assert _stats(ops) == (before[0] + 1, before[1], before[2]), f"{what}: {before} -> {_stats(ops)}: the host must have seen nothing"
        if visible:
            assert not torch.equal(got[1], last[1]), f"{what}: the write did not change dx"
        last = got


def test_cadence_with_two_entries_of_one_layer(pack_ops, monkeypatch):
    """Verification every 4th call; one layer, two input shapes with two layout keys, so two entries with a ring and a call count each."""
    ops = pack_ops
    monkeypatch.setattr(ops, "_PACK_VERIFY_EVERY", 4)
    layer, xa, _ = _build("band_1m", seed=47)                                        # 16 x 128 x 3 x 3: band order
    xb = torch.randn(16, 128, 2, 2, device="cuda")                                   # tap-major order
    ws = _conv_weights(layer)

    def run(x):
        with torch.no_grad():
            return layer(x).clone()

    def fresh(x):
        with _cache_off(ops):
            return run(x)
    _poison(_plan_bytes(ops, layer, xa)[:1])
    old = {0: run(xa), 1: run(xb)}
    assert len(ops._PACKED) == 2 and _stats(ops) == (2, 2, 0)
    for w in ws:
        w.data.add_(0.02 * torch.randn_like(w))                                      # raw write, not announced
    for i, x in ((0, xa), (1, xb)):                                                  # each entry within its own four calls, whatever the other did
        before = _stats(ops)
        outs = [run(x) for _ in range(4)]
        assert _stats(ops) == (before[0] + 1, before[1], before[2] + 3)
        assert all(torch.equal(o, old[i]) for o in outs[:3]), "a skipped call changed its result"
        assert torch.equal(outs[3], fresh(x)) and not torch.equal(outs[3], old[i]), f"entry {i}: the raw write was not picked up at the 4th call"
    _entry_is_current(ops, layer, [xa, xb], "after both verifications")
    old = {0: run(xa), 1: run(xb)}
    for w in ws:
        w.data.add_(0.02 * torch.randn_like(w))
    ops.weights_changed()                                                            # announced: each entry at once
    before = _stats(ops)
    for i, x in ((0, xa), (1, xb)):
        y = run(x)
        assert torch.equal(y, fresh(x)) and not torch.equal(y, old[i]), f"entry {i}: not picked up at once after weights_changed()"
    assert _stats(ops) == (before[0] + 2, before[1], before[2])
    _entry_is_current(ops, layer, [xa, xb], "after weights_changed()")


def test_shapes_of_one_key_share_one_entry(pack_ops):
    ops = pack_ops
    layer, x, go = _build("band_1m", seed=53)
    spec = layer.conv_spec()
    key = lambda B, H: ops._layout_key(spec, *ops._plan_cached(spec, B, 128, H, H, 96, 128, 96)[::2])
    shapes = [(B, H) for B, H in ((16, 3), (8, 4), (2, 8), (17, 3)) if key(B, H) == key(16, 3)]
    assert len(shapes) >= 3, shapes
    _poison(_plan_bytes(ops, layer, x))
    for n, (B, H) in enumerate(shapes):
        xs = torch.randn(B, 128, H, H, device="cuda")
        with torch.no_grad(), _cache_off(ops):
            gs = torch.randn_like(layer(xs))
        _check(ops, layer, xs, gs, f"input {B} x 128 x {H} x {H}")
        assert len(ops._PACKED) == 1 and _stats(ops) == (1, 1, n), (B, H, _stats(ops))


def test_entry_dies_with_its_layer_and_ids_can_be_reused(pack_ops):
    ops = pack_ops
    layer, x, go = _build("halo", seed=59)
    _check(ops, layer, x, go, "first layer")
    assert len(ops._PACKED) == 1
    del layer
    gc.collect()
    assert len(ops._PACKED) == 0, "the entry outlived its weights"
    for seed in (61, 67):                             # same shapes, other weights, very likely the ids and addresses just freed
        layer, x, go = _build("halo", seed=seed)
        _check(ops, layer, x, go, f"new layer, seed {seed}")
        del layer
        gc.collect()
        assert len(ops._PACKED) == 0

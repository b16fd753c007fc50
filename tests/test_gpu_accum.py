"""Gradient accumulation on the GPU: kan_grad_accumulate and kan_accum_gate against the numpy model of tests/accum_cells.py, and
FusedAdamW.accumulate_steps in both modes -- against a plain FusedAdamW stepped once with the model-computed mean, with clipping, with parameters
that have no gradient, under the non-finite guard, recorded into a GraphedStep, across snapshot / restore, and against one big batch.

Every comparison is bitwise (int32 views of the floats) except the last one, whose bound is the project's rule: relative L2 error against the fp64
gradient at most max(1e-6, 4 x the distance of torch's own fp32 big-batch gradient from that fp64 gradient).  Planting an inf in a batch is
ordinary floating-point data: nothing here provokes a fault."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import accum_cells as A

pytestmark = pytest.mark.gpu

PINF = float("inf")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _same_bits(a, b):
    return torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 5.1 the accumulate kernel against the model
@pytest.mark.parametrize("source", ["value", "device"])
@pytest.mark.parametrize("k", [2, 3])
def test_kernel_against_the_model(k, source, gpu_lib):
    """Two windows of k on KERNEL_LAYOUT, the accumulator and its padding prefilled with a NaN sentinel; after EVERY micro-step the row equals the
    model bit for bit, the padding still holds the sentinel and seen holds the segments that had a gradient so far.  m arrives by value
    (micro_dev NULL) or from a device int."""
    sizes, kinds = [n for n, _ in A.KERNEL_LAYOUT], [kind for _, kind in A.KERNEL_LAYOUT]
    lay = A.flat_layout(sizes)
    dev = lambda xs, dt: torch.tensor(xs, dtype=dt, device="cuda")
    seg_off, seg_n = dev(lay["seg_off"], torch.int64), dev(lay["seg_n"], torch.int32)
    chunk_seg, chunk_start = dev(lay["chunk_seg"], torch.int32), dev(lay["chunk_start"], torch.int32)
    acc = torch.full((lay["n"],), A.SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    assert acc.data_ptr() % 16 == 0
    seen, micro = torch.zeros(len(sizes), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    pad = A.padding_mask(lay)
    gen = torch.Generator().manual_seed(40 + k)
    stores, grads = [], []
    for n, kind in A.KERNEL_LAYOUT:                                         # the gradient buffers keep their addresses over both windows
        store = torch.zeros(n + 5, device="cuda")
        stores.append(store)
        grads.append(None if kind == "null" else store[1:1 + n] if kind == "view" else store[:n])
        if grads[-1] is not None:
            assert grads[-1].data_ptr() % 16 == (4 if kind == "view" else 0)
    seg_grad = dev([0 if g is None else g.data_ptr() for g in grads], torch.int64)
    model = [np.full(n, np.nan, dtype=np.float32) for n in sizes]
    for window in range(2):
        want_seen = [0] * len(sizes)
        for m in range(k):
            host = []
            for g, n in zip(grads, sizes):
                if g is None:
                    host.append(None)
                    continue
                h = torch.randn(n, generator=gen) * (1.0 + m)
                if m == 0:
                    h[0] = -0.0                                            # a copy keeps the sign of zero; 0.0 + -0.0 would not
                    h[n - 1] = -0.0
                g.copy_(h)
                host.append(h.numpy())
            micro.fill_(m)
            rc = gpu_lib.kan_grad_accumulate(_p(acc), _p(seg_grad), _p(seg_off), _p(seg_n), _p(chunk_seg), _p(chunk_start), len(lay["chunk_seg"]),
                                             A.CHUNK, _p(micro) if source == "device" else C.c_void_p(0), m if source == "value" else 0, k, _p(seen),
                                             _stream())
            assert rc == 0, gpu_lib.kan_last_error()
            got = _bits(acc)
            for s, (off, n) in enumerate(zip(lay["seg_off"], sizes)):
                model[s] = A.micro_step(model[s], host[s], m, k)
                want_seen[s] |= host[s] is not None
                assert np.array_equal(got[off:off + n], model[s].view(np.int32)), f"window {window} m {m} segment {s} ({sizes[s]}, {kinds[s]})"
            assert (got[pad] == A.SENTINEL_BITS).all(), f"window {window} m {m}: the padding was written"
            assert seen.tolist() == want_seen and int(micro) == m          # the kernel reads the counter, the gate moves it
            if m == 0:
                null = kinds.index("null")
                assert not got[lay["seg_off"][null]:lay["seg_off"][null] + sizes[null]].any()          # zero-filled: the sentinel is gone
                own = lay["seg_off"][kinds.index("own")]
                assert got[own] == np.int32(-2 ** 31)                      # -0.0
        assert not np.isnan(np.concatenate(model)).any()
        seen.zero_()                                                       # (the gate's job)


# ------------------------------------------------------------------------------------------------ 5.2 the gate
@pytest.mark.parametrize("with_guard", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_gate_counter_tables_and_seen(k, with_guard, gpu_lib):
    """Two groups, 2k + 1 calls.  The addresses are never dereferenced by the gate: any numbers do."""
    addr = [[0x1000 + 256 * i for i in range(5)], [0x9000 + 256 * i for i in range(300)]]                  # 300: more segments than threads
    n = [len(a) for a in addr]
    buf = torch.zeros(1 + 8 + 2 * sum(n) + sum((x + 1) // 2 for x in n), dtype=torch.int64, device="cuda")
    micro = buf[:1].view(torch.int32)[:1]
    at, addr_t, gated, seen, desc = 9, [], [], [], []
    for a in addr:
        addr_t.append(buf[at:at + len(a)]); gated.append(buf[at + len(a):at + 2 * len(a)])
        at += 2 * len(a)
    for a in addr:
        seen.append(buf[at:at + (len(a) + 1) // 2].view(torch.int32)[:len(a)])
        at += (len(a) + 1) // 2
    for a, t, g, s in zip(addr, addr_t, gated, seen):
        t.copy_(torch.tensor(a, dtype=torch.int64))
        g.fill_(-1)                                                        # stale: every call must overwrite all of it
        desc += [t.data_ptr(), g.data_ptr(), s.data_ptr(), len(a)]
    buf[1:9].copy_(torch.tensor(desc, dtype=torch.int64))
    counters = torch.tensor([10, 0, 0, 0, 0], dtype=torch.int64, device="cuda")
    gen = torch.Generator().manual_seed(k)
    m, model_seen = 0, [[0] * x for x in n]
    for call in range(2 * k + 1):
        for g in range(2):                                                 # what this call's accumulate launches would have seen
            new = (torch.rand(n[g], generator=gen) < 0.4).int().tolist()
            model_seen[g] = [a | b for a, b in zip(model_seen[g], new)]
            seen[g].copy_(torch.tensor(model_seen[g], dtype=torch.int32))
        rc = gpu_lib.kan_accum_gate(_p(buf[1:9]), 2, _p(micro), k, _p(counters) if with_guard else C.c_void_p(0), _stream())
        assert rc == 0, gpu_lib.kan_last_error()
        boundary = m + 1 == k
        for g in range(2):
            want_gated, want_seen, want_m = A.gate_model(m, k, model_seen[g], addr[g])
            assert gated[g].tolist() == want_gated, f"call {call} group {g}"
            assert seen[g].tolist() == want_seen, f"call {call} group {g}"
            if boundary and g == 1:
                assert any(want_gated) and not all(want_gated)             # (300 draws leave both kinds)
            model_seen[g] = want_seen
        m = want_m
        assert int(micro) == m == (call + 1) % k
        assert addr_t[0].tolist() == addr[0] and addr_t[1].tolist() == addr[1] and buf[1:9].tolist() == desc
    # the guard launch behind a call that is no step counts itself: the gate takes that one back in advance, and only that
    off_boundary = (2 * k + 1) - (2 * k + 1) // k
    assert counters.tolist() == [10 - (off_boundary if with_guard else 0), 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ rigs
def _model(norm_layer=None):
    import convkan_amd as K
    torch.manual_seed(3)
    extra = {} if norm_layer is None else dict(norm_layer=norm_layer)
    return nn.Sequential(K.KANConv2DLayer(3, 8, 3, padding=1, **extra), nn.Flatten(), nn.Linear(8 * 8 * 8, 10)).cuda().train()


def _batches(count, seed=5, bs=2):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(bs, 3, 8, 8, generator=gen).cuda(), torch.randint(0, 10, (bs,), generator=gen).cuda()) for _ in range(count)]


def _backward(model, data, target):
    model.zero_grad(set_to_none=True)
    loss = nn.functional.cross_entropy(model(data), target)
    loss.backward()
    return loss.detach()


def _state(opt):
    """Everything a step changes, whatever the mode: the flat blocks and the per-parameter step counts."""
    counts = [f["tab"]["seg_step"].tolist() if opt.capturable else list(f["steps"]) for f in opt._flat]
    return [f["block"].clone() for f in opt._flat], counts


def _same_state(a, b):
    return all(_same_bits(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]


def _mean_into(params, micro_grads):
    """p.grad of `params` = the model's window mean of the cloned micro-gradients (None where no micro-step had one)."""
    for i, p in enumerate(params):
        mean = A.window_mean([None if g[i] is None else g[i].cpu().numpy() for g in micro_grads])
        p.grad = None if mean is None else torch.from_numpy(mean).reshape(p.shape).cuda()


# ------------------------------------------------------------------------------------------------ 5.3 step equivalence, both modes
@pytest.mark.parametrize("max_grad_norm", [None, 1e-3], ids=["noclip", "clip"])
@pytest.mark.parametrize("capturable", [False, True], ids=["classic", "capturable"])
def test_window_of_three_equals_one_plain_step_with_the_mean(capturable, max_grad_norm, gpu_lib):
    import convkan_amd as K
    model = _model()
    twin = copy.deepcopy(model)
    opt = K.FusedAdamW(model.parameters(), lr=1e-2, weight_decay=1e-2, capturable=capturable, max_grad_norm=max_grad_norm)
    plain = K.FusedAdamW(twin.parameters(), lr=1e-2, weight_decay=1e-2, capturable=capturable, max_grad_norm=max_grad_norm)
    batches = _batches(4)
    for m_, o in ((model, opt), (twin, plain)):                            # one ordinary step first: moments and counts are not all zero
        _backward(m_, *batches[3])
        o.step()
    assert opt._accum is None and _same_state(_state(opt), _state(plain))
    opt.accumulate_steps = 3                                               # no window is open: allowed
    start = _state(opt)
    params = list(model.parameters())
    micro_grads = []
    for m in range(3):
        assert opt.micro_step == m
        _backward(model, *batches[m])
        micro_grads.append([None if p.grad is None else p.grad.clone() for p in params])
        opt.step()
        for p, g in zip(params, micro_grads[-1]):                          # p.grad is read, never modified
            assert (p.grad is None) == (g is None) and (g is None or _same_bits(p.grad, g))
        if m < 2:
            assert _same_state(_state(opt), start), f"micro-step {m} changed a parameter, a moment or a step count"
            if max_grad_norm is not None:
                assert float(opt.grad_norm) == 0.0 and float(opt.clip_scale) == 1.0
    assert opt.micro_step == 0
    _mean_into(list(twin.parameters()), micro_grads)
    plain.step()
    after, want = _state(opt), _state(plain)
    assert _same_state(after, want)
    has_grad = [[g is not None for g in micro_grads[0]]]
    assert after[1] == [[s + (1 if h else 0) for s, h in zip(start[1][0], has_grad[0])]] and sum(has_grad[0]) >= 4      # advanced by exactly 1
    assert not _same_state(after, start)
    if max_grad_norm is not None:
        assert _same_bits(opt.grad_norm, plain.grad_norm) and _same_bits(opt.clip_scale, plain.clip_scale)
        assert 0.0 < float(opt.clip_scale) < 1.0                           # small enough to clip
        assert _same_bits(opt.grad_norms(), plain.grad_norms())
    sd = opt.state_dict()                                                  # unchanged format, loads into torch's AdamW
    torch.optim.AdamW(copy.deepcopy(twin).parameters(), foreach=False).load_state_dict(sd)


# ------------------------------------------------------------------------------------------------ 5.4 parameters without a gradient
@pytest.mark.parametrize("capturable", [False, True], ids=["classic", "capturable"])
def test_parameters_without_a_gradient_in_the_window(capturable, gpu_lib):
    """Five parameters in two groups over a window of 3: never a gradient; one only in the middle micro-step; one only in the last; one only in
    the first; one in all three."""
    import convkan_amd as K
    sizes, when = [5, 8193, 300, 4, 8192], [(), (1,), (2,), (0,), (0, 1, 2)]
    gen = torch.Generator().manual_seed(9)
    init = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[torch.randn(n, generator=gen) * 0.1 if m in w else None for n, w in zip(sizes, when)] for m in range(3)]
    rigs = []
    for accumulate in (True, False):
        ps = [nn.Parameter(x.clone().cuda()) for x in init]
        o = K.FusedAdamW([dict(params=ps[:2]), dict(params=ps[2:], lr=3e-3)], lr=1e-2, capturable=capturable)
        rigs.append((ps, o))
    (ps, opt), (qs, plain) = rigs
    opt.accumulate_steps = 3
    start = _state(opt)
    for m in range(3):
        for p, g in zip(ps, grads[m]):
            p.grad = None if g is None else g.clone().cuda()
        opt.step()
        if m < 2:
            assert _same_state(_state(opt), start)
    _mean_into(qs, grads)
    assert qs[0].grad is None and _same_bits(qs[1].grad, (grads[1][1] * np.float32(1.0 / 3.0)).cuda())         # g / 3
    plain.step()
    assert _same_state(_state(opt), _state(plain))
    assert _state(opt)[1] == [[0, 1], [1, 1, 1]]                           # the parameter without a gradient did not age
    assert _same_bits(ps[0], init[0].cuda()) and not _same_bits(ps[1], init[1].cuda())
    assert not opt._flat[0]["block"][1:, :64].any()                        # nor did its moments move


# ------------------------------------------------------------------------------------------------ 5.5 the guard
def test_guard_skips_the_poisoned_window_and_the_next_one_is_clean(gpu_lib):
    """capturable, skip_nonfinite, k = 2, two windows; ONE inf pixel in the first micro-batch.  The twin has no guard and only ever sees the second
    window."""
    import convkan_amd as K
    model = _model()
    twin = copy.deepcopy(model)
    opt = K.FusedAdamW(model.parameters(), lr=1e-2, capturable=True)
    opt.skip_nonfinite = True
    opt.accumulate_steps = 2
    clean = K.FusedAdamW(twin.parameters(), lr=1e-2, capturable=True)
    clean.accumulate_steps = 2
    batches = _batches(4)
    batches[0][0][1, 2, 3, 4] = PINF
    start = _state(opt)
    reports = []
    for i, (d, t) in enumerate(batches):
        K.train_step(model, d, t, opt)
        r = opt.guard_report()
        reports.append((r["guarded_steps"], r["skipped_steps"], int(opt.last_step_skipped), opt.micro_step))
        if i < 2:
            assert _same_state(_state(opt), start), f"call {i + 1} of the poisoned window changed something"
        if i == 2:
            assert _same_state(_state(opt), start)                         # the first call of window 2 is no step either
    # (guarded steps, skipped steps, last_step_skipped, micro_step) after each call: the calls inside a window add to no counter
    assert reports == [(0, 0, 0, 1), (1, 1, 1, 0), (1, 1, 0, 1), (2, 1, 0, 0)]
    assert int(opt.skipped_steps) == 1 and int(opt.last_step_skipped) == 0
    r = opt.guard_report()
    assert (r["first_skipped"], r["last_skipped"]) == (1, 1) and r["nonfinite_params"]
    for d, t in batches[2:]:
        K.train_step(twin, d, t, clean)
    assert _same_state(_state(opt), _state(clean))                         # the poisoned accumulator did not leak
    assert torch.isfinite(opt._flat[0]["block"]).all() and not _same_state(_state(opt), start)
    has_grad = [p.grad is not None for p in opt._flat[0]["params"]]
    assert _state(opt)[1] == [[1 if h else 0 for h in has_grad]]


# ------------------------------------------------------------------------------------------------ 5.6 recorded against eager
@pytest.mark.parametrize("norm_layer", [None, nn.BatchNorm2d], ids=["instancenorm", "batchnorm"])
def test_recorded_window_equals_eager(norm_layer, gpu_lib):
    import convkan_amd as K
    model = _model(norm_layer)
    twin = copy.deepcopy(model)
    opt = K.FusedAdamW(model.parameters(), lr=1e-2, weight_decay=1e-2, capturable=True)
    opt.accumulate_steps = 2
    eager = K.FusedAdamW(twin.parameters(), lr=1e-2, weight_decay=1e-2, capturable=True)
    eager.accumulate_steps = 2
    batches = _batches(4)
    start = _state(opt)
    buffers = [b.clone() for b in model.buffers()]
    step = K.GraphedStep(model, *batches[0], optimizer=opt)
    for b, was in zip(model.buffers(), buffers):                           # the warm-up moved the running buffers, which belong to the model
        b.copy_(was)
    assert opt.micro_step == 0                                             # three warm-up calls and one recording later: the warm-up was undone
    assert _same_state(_state(opt), start)
    losses = [[], []]
    for i, (d, t) in enumerate(batches):
        losses[0].append(step(d, t).clone())
        losses[1].append(K.train_step(twin, d, t, eager).clone())
        assert opt.micro_step == eager.micro_step == (i + 1) % 2
        if i == 0:
            assert _same_state(_state(opt), start)                         # the first replay is micro-step 0 of a fresh window: no update
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(*losses)):
        assert _same_bits(a, b), f"loss of micro-batch {i}: {float(a)} recorded, {float(b)} eager"
    assert _same_state(_state(opt), _state(eager)) and not _same_state(_state(opt), start)
    has_grad = [p.grad is not None for p in eager._flat[0]["params"]]
    assert _state(opt)[1] == [[2 if h else 0 for h in has_grad]] and sum(has_grad) >= 4
    for (name, a), (_, b) in zip(model.named_buffers(), twin.named_buffers()):
        assert torch.equal(a, b), name                                     # BatchNorm: running mean / variance / batch count
    if norm_layer is not None:
        counts = [b for n, b in model.named_buffers() if n.endswith("num_batches_tracked")]
        assert counts and all(int(c) == 4 for c in counts)                 # statistics per micro-batch, as per-rank BatchNorm takes them


def test_the_attribute_cannot_change_while_capturing(gpu_lib):
    import convkan_amd as K
    from convkan_amd._lib import KanConvError
    ps = [nn.Parameter(torch.randn(8, device="cuda"))]
    opt = K.FusedAdamW(ps, capturable=True)
    opt.accumulate_steps = 2
    scratch = torch.zeros(4, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for change in (lambda: setattr(opt, "accumulate_steps", 3), opt.reset_accumulation):
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(KanConvError, match="capturing"):
            with torch.cuda.graph(graph, stream=side):
                scratch.add_(1.0)
                change()
        torch.cuda.synchronize()
    assert opt.accumulate_steps == 2 and opt.micro_step == 0


# ------------------------------------------------------------------------------------------------ 5.7 snapshot, restore, reset
def test_snapshot_restore_and_reset_inside_a_window(gpu_lib):
    import convkan_amd as K
    sizes = [3, 8193, 70]
    gen = torch.Generator().manual_seed(21)
    init = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[torch.randn(n, generator=gen).cuda() for n in sizes] for _ in range(5)]

    def rig():
        ps = [nn.Parameter(x.clone().cuda()) for x in init]
        o = K.FusedAdamW(ps, lr=1e-2, capturable=True)
        o.accumulate_steps = 3
        return ps, o

    def call(ps, o, g):
        for p, x in zip(ps, g):
            p.grad = x.clone()
        o.step()

    ps, straight = rig()
    for g in grads[:3]:
        call(ps, straight, g)
    want = _state(straight)
    assert want[1] == [[1, 1, 1]]
    # a snapshot after micro-step 0, two calls of something else (they finish the window), restore, the rest of the window
    ps, opt = rig()
    call(ps, opt, grads[0])
    saved = opt.snapshot()
    call(ps, opt, grads[3]); call(ps, opt, grads[4])
    assert opt.micro_step == 0 and not _same_state(_state(opt), want)
    opt.restore(saved)
    assert opt.micro_step == 1
    call(ps, opt, grads[1]); call(ps, opt, grads[2])
    assert _same_state(_state(opt), want)
    # reset in the middle of a window: the next call is an m == 0 overwrite
    ps, opt = rig()
    call(ps, opt, grads[3]); call(ps, opt, grads[4])
    assert opt.micro_step == 2
    opt.reset_accumulation()
    assert opt.micro_step == 0
    for g in grads[:3]:
        call(ps, opt, g)
    assert _same_state(_state(opt), want)


def test_launch_list_of_a_capturable_micro_step(gpu_lib, monkeypatch):
    """k > 1, two groups, clipping: per call the two accumulate launches, ONE gate, then exactly the launches of the plain step."""
    import convkan_amd as K
    from convkan_amd import optim as O
    ps = [nn.Parameter(torch.randn(n, device="cuda")) for n in (5, 8193, 70)]
    opt = K.FusedAdamW([dict(params=ps[:2]), dict(params=ps[2:])], capturable=True, max_grad_norm=1.0)
    opt.accumulate_steps = 2
    calls = []

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(gpu_lib, name)
            return lambda *a: (calls.append(name), fn(*a))[1]
    for p in ps:
        p.grad = torch.randn_like(p)
    opt.step()                                                             # uploads lr, max_grad_norm and the address tables
    monkeypatch.setattr(O.L, "load", lambda: Recorder())
    opt.step()
    monkeypatch.undo()
    assert calls == ["kan_grad_accumulate"] * 2 + ["kan_accum_gate"] + ["kan_grad_sqnorm_chunks"] * 2 + ["kan_grad_norm_finish"] + \
        ["kan_adamw_advance", "kan_adamw_step_segments_dev_clip"] * 2


def test_train_model_generic_accumulates(gpu_lib):
    import convkan_amd as K
    for graphed in (False, True):
        model = _model()
        history = K.train_model_generic(model, _batches(3), epochs=2, learning_rate=1e-2, graphed=graphed, accumulate_steps=2)
        assert len(history) == 2 and all(h == h and h > 0 for h in history)
    # six micro-batches, windows of two: the window left open by the first epoch's third batch closes in the second epoch
    model, twin = _model(), _model()
    opt = K.FusedAdamW(twin.parameters(), lr=1e-2, weight_decay=1e-4)
    opt.accumulate_steps = 2
    K.train_model_generic(model, _batches(3), epochs=2, learning_rate=1e-2, gamma=1.0, accumulate_steps=2)
    for d, t in _batches(3) * 2:
        K.train_step(twin, d, t, opt)
    assert opt._flat[0]["steps"].count(3) >= 4 and opt.micro_step == 0
    for a, b in zip(model.parameters(), twin.parameters()):
        assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------ 5.8 against one big batch
def test_four_micro_batches_of_two_against_one_batch_of_eight(gpu_lib):
    """The only comparison with a tolerance.  Reference: the fp64 CPU gradient of the batch of 8.  Bound per parameter: relative L2 error at most
    max(1e-6, 4 x the relative L2 distance of torch's own fp32 gradient of the batch of 8 from that reference)."""
    import convkan_amd as K
    torch.manual_seed(8)
    net = nn.Sequential(nn.Linear(37, 19), nn.Tanh(), nn.Linear(19, 5))
    ref = copy.deepcopy(net).double()
    gen = torch.Generator().manual_seed(88)
    data, target = torch.randn(8, 37, generator=gen), torch.randint(0, 5, (8,), generator=gen)
    nn.functional.cross_entropy(ref(data.double()), target).backward()
    exact = [p.grad.clone() for p in ref.parameters()]
    net = net.cuda()
    big = copy.deepcopy(net)
    nn.functional.cross_entropy(big(data.cuda()), target.cuda()).backward()
    opt = K.FusedAdamW(net.parameters(), lr=1e-3)
    opt.accumulate_steps = 4
    for i in range(4):
        net.zero_grad(set_to_none=True)
        nn.functional.cross_entropy(net(data[2 * i:2 * i + 2].cuda()), target[2 * i:2 * i + 2].cuda()).backward()
        opt.step()
    assert opt.micro_step == 0 and opt._flat[0]["steps"] == [1, 1, 1, 1]
    flat, row = opt._flat[0], opt._accum["rows"][0]
    rel = lambda x, e: float((x.double().cpu().flatten() - e.flatten()).norm() / e.norm())
    bad = []
    for (name, p), off, e, b in zip(net.named_parameters(), flat["tab"]["seg_off"].tolist(), exact, big.parameters()):
        err, own = rel(row[off:off + p.numel()], e), rel(b.grad, e)
        bound = max(1e-6, 4 * own)
        print(f"[big batch] {name}: accumulated {err:.3e}, torch fp32 big batch {own:.3e}, bound {bound:.3e}")
        if not err <= bound:
            bad.append(f"{name}: {err:.3e} > {bound:.3e}")
    assert not bad, "; ".join(bad)

"""The device-side anomaly mode on the GPU: the probe kernel (kan_nonfinite_count through ops.count_nonfinite), the guarded FusedAdamW step
(kan_adamw_guard behind the statistics pass, the masked address tables), and both inside a recorded step, with AnomalyProbe.

Every comparison is exact: integer counters against torch's own count of the same tensor, and torch.equal between a guarded optimizer and a twin
that never saw the poisoned step.  Planting an inf or a NaN in a tensor is ordinary floating-point data: nothing here provokes a fault."""
import itertools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
BAD = (NAN, PINF, NINF)
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 2 ** 20 + 3)


def _i64(xs):
    return torch.tensor(xs, dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. the probe kernel
def _plants(n, gen):
    """The places the issue names: the first element, the last, every position of the float4 tail, and -- the larger sizes -- 17 random places."""
    out = [[0], [n - 1]] + [[i] for i in range(n & ~3, n)]
    if n >= 255:
        out.append(torch.randperm(n, generator=gen)[:17].tolist())
    return out


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_count_matches_torch_at_every_size_and_alignment(off, gpu_lib):
    """A view `off` elements into a 256-byte aligned buffer: off = 0 takes the float4 path (and its tail), 1..3 the scalar path.  One record per
    planting; all of them are read once at the end and compared with (~torch.isfinite(view)).sum() of the very tensor the kernel read."""
    from convkan_amd import ops
    gen = torch.Generator().manual_seed(100 + off)
    tick = _i64([7])
    cases = [(n, places) for n in SIZES for places in _plants(n, gen)]
    records = torch.zeros((len(cases), 3), dtype=torch.int64, device="cuda")
    expected, keep = [], []
    for k, (n, places) in enumerate(cases):
        store = torch.randn(n + 8, generator=gen).cuda()
        view = store[off:off + n]
        assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
        for j, i in enumerate(places):
            view[i] = BAD[(k + j) % 3]
        store[:off] = NAN                                                  # what lies around the view must not be counted
        store[off + n:] = PINF
        ops.count_nonfinite(view, records[k], tick)
        expected.append((~torch.isfinite(view)).sum())
        keep.append(store)
    got, want = records.tolist(), torch.stack(expected).tolist()
    bad = [f"n={n} off={off} places={places[:4]}: record {g}, torch counts {w}"
           for (n, places), g, w in zip(cases, got, want) if g != [w, 7, 7] or w != len(places)]
    assert not bad, "\n  ".join(bad)


def test_count_of_a_tensor_that_is_not_contiguous(gpu_lib):
    from convkan_amd import ops
    torch.manual_seed(1)
    full = torch.randn(6, 10, device="cuda")
    full[:, 1] = NAN                                                       # a column the view does not hold
    full[2, 3], full[5, 9], full[0, 0] = PINF, NINF, NAN
    view = full[:, ::3]                                                    # columns 0, 3, 6, 9
    assert not view.is_contiguous()
    rec, tick = _i64([0, 0, 0]), _i64([4])
    ops.count_nonfinite(view, rec, tick)
    assert rec.tolist() == [3, 4, 4] and int((~torch.isfinite(view)).sum()) == 3
    empty = _i64([0, 0, 0])
    ops.count_nonfinite(full[:0], empty, tick)                             # n == 0: nothing is launched
    assert empty.tolist() == [0, 0, 0]


@pytest.mark.parametrize("off", [0, 1])
def test_finite_extremes_count_zero_and_leave_the_ticks_alone(off, gpu_lib):
    from convkan_amd import ops
    flt_max, denorm, below_normal = 3.4028234663852886e38, 1.401298464324817e-45, 1.1754942106924411e-38
    vals = torch.tensor([flt_max, -flt_max, denorm, -denorm, below_normal, -below_normal, -0.0, 0.0, 1.0, -1.0], dtype=torch.float32)
    assert torch.isfinite(vals).all() and float(vals[2]) != 0.0
    tick = _i64([3])
    for n in (1, 5, 10, 1027, 8193):
        store = vals.repeat((n + 8) // 10 + 1).cuda()
        view = store[off:off + n]
        rec = _i64([0, 123, 456])
        ops.count_nonfinite(view, rec, tick)
        assert rec.tolist() == [0, 123, 456], (n, off)


def test_first_and_last_tick_and_reproducibility(gpu_lib):
    """Ticks 5 (3 elements), 7 (clean) and 9 (2 elements) on one record: [5, 5, 9]; the clean launch changes nothing; twice the same."""
    from convkan_amd import ops
    torch.manual_seed(2)
    dirty5, clean, dirty9 = torch.randn(70001, device="cuda"), torch.randn(9000, device="cuda"), torch.randn(4097, device="cuda")
    dirty5[[0, 33333, 70000]] = torch.tensor([NAN, PINF, NINF], device="cuda")
    dirty9[[17, 4096]] = torch.tensor([NINF, NAN], device="cuda")
    runs = []
    for _ in range(2):
        rec, tick, seen = _i64([0, 0, 0]), _i64([0]), []
        for value, t in ((5, dirty5), (7, clean), (9, dirty9)):
            tick.fill_(value)
            ops.count_nonfinite(t, rec, tick)
            seen.append(rec.clone())
        runs.append([s.tolist() for s in seen])
    assert runs[0] == [[3, 5, 5], [3, 5, 5], [5, 5, 9]]
    assert runs[1] == runs[0]


# ------------------------------------------------------------------------------------------------ 2. the guarded step
# (elements, group, kind): sizes at the float4 tail and the 8192-element chunk boundary of optim.py; one parameter never gets a gradient, one
# gradient is a view one element into its storage (the scalar path of the norm and step kernels)
LAYOUT = [(1, 0, "own"), (3, 0, "own"), (4, 0, "own"), (7, 0, "none"), (5, 0, "view"), (8191, 1, "own"), (8192, 1, "own"), (8193, 1, "view")]
WITH_GRAD = [i for i, (_, _, kind) in enumerate(LAYOUT) if kind != "none"]


class _Rig:
    """One FusedAdamW(capturable=True) over LAYOUT in two groups, with clean gradients that can be re-planted."""

    def __init__(self, max_grad_norm, guard):
        from convkan_amd.optim import FusedAdamW
        gen = torch.Generator().manual_seed(11)
        self.params = [nn.Parameter(torch.randn(n, generator=gen).cuda()) for n, _, _ in LAYOUT]
        self.clean = [torch.randn(n, generator=gen).cuda() * 0.1 for n, _, _ in LAYOUT]
        self.opt = FusedAdamW([dict(params=[p for p, (_, g, _) in zip(self.params, LAYOUT) if g == 0]),
                               dict(params=[p for p, (_, g, _) in zip(self.params, LAYOUT) if g == 1], lr=3e-3, weight_decay=0.1)],
                              lr=1e-2, capturable=True, max_grad_norm=max_grad_norm)
        self.opt.skip_nonfinite = guard
        self.stores = []
        for p, (n, _, kind) in zip(self.params, LAYOUT):
            if kind == "none":
                continue
            store = torch.zeros(n + 5, device="cuda")
            p.grad = store[1:1 + n] if kind == "view" else store[:n]
            assert p.grad.data_ptr() % 16 == (4 if kind == "view" else 0)
            self.stores.append(store)

    def load(self, plant=()):
        """Clean gradients, then `plant`: (parameter, element, value) triples."""
        for p, c in zip(self.params, self.clean):
            if p.grad is not None:
                p.grad.copy_(c)
        for i, e, v in plant:
            self.params[i].grad[e] = v

    def state(self):
        return [f["block"].clone() for f in self.opt._flat], [f["tab"]["seg_step"].clone() for f in self.opt._flat]

    def same(self, other_state):
        blocks, steps = self.state()
        return (all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(blocks, other_state[0]))
                and all(torch.equal(a, b) for a, b in zip(steps, other_state[1])))


def _places(n):
    return sorted({0, n - 1} | set(range(n & ~3, n)))                      # first, last, and every element of the float4 tail


@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
def test_poisoned_step_changes_nothing_and_the_next_one_is_the_twins(max_grad_norm, gpu_lib):
    """Every (gradient, place, value): the poisoned step leaves the flat blocks and the step counts bit for bit, says so, and names the
    parameter; the clean step behind it lands where a twin lands that only ever saw the clean step."""
    rig, twin = _Rig(max_grad_norm, True), _Rig(max_grad_norm, False)
    for r in (rig, twin):                                                  # one clean step first: moments and counts are not all zero
        r.load()
        r.opt.step()
    assert rig.same(twin.state())
    start, s0 = rig.opt.snapshot(), rig.state()
    twin.load()
    twin.opt.step()
    after_clean = twin.state()
    bad, cases = [], 0
    for i, value in itertools.product(WITH_GRAD, BAD):
        for e in _places(LAYOUT[i][0]):
            cases += 1
            rig.opt.restore(start)
            rig.load([(i, e, value)])
            rig.opt.step()
            report = rig.opt.guard_report()
            if not rig.same(s0):
                bad.append(f"param {i} elem {e} {value}: the skipped step changed a block or a step count")
            if int(rig.opt.last_step_skipped) != 1 or report["nonfinite_params"] != [i] or (report["skipped_steps"], report["last_skipped"]) != (1, 2):
                bad.append(f"param {i} elem {e} {value}: report {report}, last_step_skipped {int(rig.opt.last_step_skipped)}")
            rig.load()
            rig.opt.step()
            if not rig.same(after_clean):
                bad.append(f"param {i} elem {e} {value}: the clean step after the skipped one differs from the twin's")
            if int(rig.opt.last_step_skipped) != 0 or int(rig.opt.skipped_steps) != 1:
                bad.append(f"param {i} elem {e} {value}: counters after the clean step: {rig.opt.guard_report()}")
    assert cases == 3 * (1 + 3 + 2 + 2 + 4 + 2 + 2) and not bad, "\n  ".join(bad[:20])
    # two poisoned parameters in two groups, one decision
    rig.opt.restore(start)
    rig.load([(1, 2, NAN), (7, 8192, NINF)])
    rig.opt.step()
    assert rig.same(s0) and rig.opt.guard_report()["nonfinite_params"] == [1, 7]
    if max_grad_norm is not None:                                          # the statistics show what caused the skip
        assert not torch.isfinite(rig.opt.grad_norm) and not torch.isfinite(rig.opt.grad_norms()[[1, 7]]).any()
        assert torch.isfinite(rig.opt.grad_norms()[[0, 2, 3, 4, 5, 6]]).all()


@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
def test_clean_gradients_guard_on_equals_guard_off(max_grad_norm, gpu_lib):
    rig, twin = _Rig(max_grad_norm, True), _Rig(max_grad_norm, False)
    for k in range(3):
        for r in (rig, twin):
            r.load()
            for p in r.params:
                if p.grad is not None:
                    p.grad.mul_(1.0 + k)                                   # three different steps
            r.opt.step()
        assert rig.same(twin.state()), f"step {k + 1}"
        assert int(rig.opt.last_step_skipped) == 0
    assert rig.opt.guard_report() == dict(guarded_steps=3, skipped_steps=0, first_skipped=None, last_skipped=None, nonfinite_params=[])
    assert [f["tab"]["seg_step"].tolist() for f in rig.opt._flat] == [[3, 3, 3, 0, 3], [3, 3, 3]]
    assert twin.opt._guard is None


def test_finite_but_huge_gradients_are_not_skipped(gpu_lib):
    """Two elements of 3e38: the norm, 4.24e38, does not fit fp32 -- grad_norm reads inf -- but the decision is taken on the double."""
    rig, twin = _Rig(1.0, True), _Rig(1.0, False)
    for r in (rig, twin):
        r.load([(6, 0, 3e38), (6, 8191, 3e38)])
        r.opt.step()
    assert float(rig.opt.grad_norm) == PINF
    assert int(rig.opt.last_step_skipped) == 0 and int(rig.opt.skipped_steps) == 0
    assert rig.same(twin.state())
    assert [f["tab"]["seg_step"].tolist() for f in rig.opt._flat] == [[1, 1, 1, 0, 1], [1, 1, 1]]


def test_snapshot_restore_and_state_dict(gpu_lib):
    rig = _Rig(None, True)
    rig.load()
    rig.opt.step()
    rig.load([(5, 8190, PINF)])
    rig.opt.step()
    want = dict(guarded_steps=2, skipped_steps=1, first_skipped=2, last_skipped=2, nonfinite_params=[5])
    assert rig.opt.guard_report() == want
    saved, state = rig.opt.snapshot(), rig.state()
    rig.opt.reset_guard()
    assert rig.opt.guard_report() == dict(guarded_steps=0, skipped_steps=0, first_skipped=None, last_skipped=None, nonfinite_params=[])
    rig.load()
    rig.opt.step()
    assert not rig.same(state)
    rig.opt.restore(saved)
    assert rig.same(state) and rig.opt.guard_report() == want
    sd = rig.opt.state_dict()                                              # one clean and one skipped step: step 1 wherever there was a gradient
    steps = [int(sd["state"][i]["step"]) for i in range(len(LAYOUT))]
    assert steps == [1, 1, 1, 0, 1, 1, 1, 1]
    ref = torch.optim.AdamW([dict(params=[nn.Parameter(torch.zeros(n, device="cuda")) for n, g, _ in LAYOUT if g == gi]) for gi in (0, 1)], foreach=False)
    ref.load_state_dict(sd)
    assert [int(ref.state_dict()["state"][i]["step"]) for i in range(len(LAYOUT))] == steps


class _Recorder:
    """Stands in for the loaded library: passes every call on and keeps the names."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
def test_launch_lists_with_the_switch_off_and_on(max_grad_norm, gpu_lib, monkeypatch):
    """Off -- never set, or set and cleared again -- the step calls what it called before the switch existed; on, the statistics pass (when
    clipping did not already run it) and ONE guard launch are all that is added."""
    from convkan_amd import optim as O
    step = "kan_adamw_step_segments_dev" + ("_clip" if max_grad_norm is not None else "")
    norm = ["kan_grad_sqnorm_chunks", "kan_grad_sqnorm_chunks", "kan_grad_norm_finish"]
    plain = (norm if max_grad_norm is not None else []) + ["kan_adamw_advance", step] * 2
    seen = {}
    for name, guard in (("never", None), ("on", True), ("off_again", False)):
        rig = _Rig(max_grad_norm, bool(guard))
        if guard is False:
            rig.opt.skip_nonfinite = True
            rig.opt.skip_nonfinite = False
        rig.load()
        rig.opt.step()                                                     # uploads lr, max_grad_norm and the address tables
        rec = _Recorder(gpu_lib)
        monkeypatch.setattr(O.L, "load", lambda rec=rec: rec)
        rig.opt.step()
        monkeypatch.undo()
        seen[name] = rec.calls
    assert seen["never"] == plain and seen["off_again"] == plain
    assert seen["on"] == norm + ["kan_adamw_guard"] + ["kan_adamw_advance", step] * 2


def test_train_model_generic_warns_once_per_epoch_that_skipped(gpu_lib):
    import warnings
    import convkan_amd as K
    model = _tiny()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        history = K.train_model_generic(model, _batches(), epochs=2, learning_rate=1e-2, graphed=True, skip_nonfinite=True)
    ours = [str(w.message) for w in caught if "skipped for non-finite" in str(w.message)]
    assert len(ours) == 2 and all("1 of 3 optimizer steps" in m for m in ours), ours      # the poisoned batch comes round once per epoch
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert len(history) == 2 and all(h != h for h in history)              # the poisoned batch's loss is still NaN: the guard protects the state
    with pytest.raises(ValueError, match="graphed"):
        K.train_model_generic(_tiny(), _batches(), epochs=1, skip_nonfinite=True)


# ------------------------------------------------------------------------------------------------ 3. the recorded step
def _tiny():
    import convkan_amd as K
    torch.manual_seed(3)
    return nn.Sequential(K.KANConv2DLayer(3, 8, 3, padding=1), nn.MaxPool2d(2), nn.Flatten(), nn.Linear(8 * 4 * 4, 10)).cuda().train()


def _batches():
    gen = torch.Generator().manual_seed(5)
    out = [(torch.randn(4, 3, 8, 8, generator=gen).cuda(), torch.randint(0, 10, (4,), generator=gen).cuda()) for _ in range(3)]
    out[1][0][2, 1, 3, 4] = PINF                                           # ONE +inf pixel in the second batch
    return out


def _optimizer(model, guard):
    import convkan_amd as K
    opt = K.FusedAdamW(model.parameters(), lr=1e-2, weight_decay=1e-2, capturable=True)
    opt.skip_nonfinite = guard
    return opt


def _recorded(guard):
    import convkan_amd as K
    model = _tiny()
    opt = _optimizer(model, guard)
    probe = K.AnomalyProbe(model)                                          # BEFORE the step is recorded: its launches become graph nodes
    step = K.GraphedStep(model, *_batches()[0], optimizer=opt)
    probe.reset()                                                          # forget the warm-up: replay k is tick k
    for d, t in _batches():
        step(d, t)
    torch.cuda.synchronize()
    return model, opt, probe


def test_recorded_guarded_step_skips_the_poisoned_batch_and_the_probe_names_the_layer(gpu_lib):
    import convkan_amd as K
    model, opt, probe = _recorded(guard=True)
    twin = _tiny()
    twin_opt = _optimizer(twin, False)
    batches = _batches()
    for d, t in (batches[0], batches[2]):                                  # the eager twin never sees the poisoned batch
        K.train_step(twin, d, t, twin_opt)
    torch.cuda.synchronize()
    a, b = opt._flat[0], twin_opt._flat[0]
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    for name, (pa, ma, va), (pb, mb, vb) in zip(names, a["views"], b["views"]):
        for what, x, y in (("parameter", pa, pb), ("exp_avg", ma, mb), ("exp_avg_sq", va, vb)):
            print(f"[recorded guard] {name} {what}: max |recorded - eager| {float((x.double() - y.double()).abs().max()):.3e}")
    assert torch.isfinite(a["block"]).all()
    assert torch.equal(a["block"], b["block"]) and torch.equal(a["tab"]["seg_step"], b["tab"]["seg_step"])
    has_grad = [i for i, p in enumerate(opt._flat[0]["params"]) if p.grad is not None]
    assert a["tab"]["seg_step"].tolist() == [2 if i in has_grad else 0 for i in range(len(names))] and len(has_grad) >= 4
    report = opt.guard_report()
    assert int(opt.skipped_steps) == 1 and int(opt.last_step_skipped) == 0
    assert (report["guarded_steps"], report["skipped_steps"], report["first_skipped"], report["last_skipped"]) == (3, 1, 2, 2)
    linear = [i for i, n in enumerate(names) if n.startswith("3.")]        # the NaN loss reaches the Linear layer's gradients whatever else it reaches
    assert len(linear) == 2 and set(linear) <= set(report["nonfinite_params"]) <= set(has_grad)
    found = probe.report()
    print("[recorded guard] probe:", found)
    assert found and (found[0]["name"], found[0]["direction"], found[0]["first_tick"]) == ("0", "forward", 2)
    assert all(e["first_tick"] == 2 and e["last_tick"] == 2 for e in found)      # nothing was born in a clean replay
    assert {(e["name"], e["direction"]) for e in found} == set(probe.slots)
    assert [e["direction"] for e in found] == ["forward", "forward", "backward", "backward"]
    assert [e["name"] for e in found] == ["0", "<output>", "<output>", "0"]


def test_the_same_batches_without_the_guard_poison_the_parameters(gpu_lib):
    """What the guard prevents -- and that the probe alone changes nothing: it reports, the parameters are NaN all the same."""
    model, opt, probe = _recorded(guard=False)
    assert opt._guard is None
    assert not torch.isfinite(opt._flat[0]["block"][0]).all()
    assert all(torch.isnan(p).all() for p in model[3].parameters())        # the poisoned sample's row of the loss gradient reaches every element
    found = probe.report()
    assert (found[0]["name"], found[0]["direction"], found[0]["first_tick"]) == ("0", "forward", 2)
    assert all(e["first_tick"] == 2 for e in found)
    assert {(e["name"], e["direction"]): e["last_tick"] for e in found}[("<output>", "forward")] == 3      # the third replay runs on garbage


def test_the_probe_is_bit_neutral(gpu_lib):
    """One eager step with and without a probe: loss, logits and every gradient are torch.equal; a no_grad forward registers no gradient hook."""
    import convkan_amd as K
    d, t = _batches()[0]
    got = []
    for attach in (False, True):
        model = _tiny()
        probe = K.AnomalyProbe(model) if attach else None
        logits = model(d)
        loss = nn.functional.cross_entropy(logits, t)
        loss.backward()
        got.append([loss.detach().clone(), logits.detach().clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
        if probe is not None:
            probe.check(loss, "loss")
            assert probe.report() == [] and int(probe.tick) == 1
            with torch.no_grad():
                out = model(d)
            assert out.grad_fn is None and int(probe.tick) == 2
            probe.check(torch.full((3,), NAN, device="cuda"), "planted")
            assert [(e["name"], e["direction"], e["elements"], e["first_tick"]) for e in probe.report()] == [("planted", "forward", 3, 2)]
            assert probe.slots[-2:] == [("loss", "forward"), ("planted", "forward")]
            probe.remove()
    assert len(got[0]) == len(got[1]) >= 2 + 4
    for k, (x, y) in enumerate(zip(*got)):
        assert torch.equal(x, y), f"tensor {k} differs by {float((x - y).abs().max()):.3e}"

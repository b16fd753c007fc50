"""The loss kernels of csrc/kan_loss.hip and the evaluation loop built on them (ops.cross_entropy, K.CrossEntropyLoss, K.ClassMetrics,
K.evaluate, K.train_and_test_models) on the device.

Loss, lse and dlogits against torch.nn.functional.cross_entropy in fp64 on the CPU under the project's one tolerance rule,
    max(stated, 4 x the distance of torch's own fp32 CPU result from fp64 on the same inputs, measured live),
stated = helpers.TOL_Y for the loss and lse (relative to max(1, |reference|)) and helpers.TOL_DX, max-normalised, for dlogits.  Predictions and
counters are integers: exact equality with counts made on the CPU from the same fp32 logits.  Determinism is bit equality.  Every case
prints what it measured."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from helpers import TOL_DX, TOL_Y, relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL = os.path.join(ROOT, "tests", "golden", "eval")
FIXTURES = sorted(f[:-4] for f in os.listdir(EVAL) if f.endswith(".npz")) if os.path.isdir(EVAL) else []
# one class; one row; rows shorter than, equal to and just past a wavefront; multi-pass rows; a row count that is no multiple of the 4 rows
# of a workgroup; more rows than the 256 threads of the final reduction hold at once
SHAPES = [(1, 1), (1, 2), (5, 10), (256, 10), (257, 100), (3, 64), (3, 65), (7, 1000), (2, 4097), (4100, 3)]
GRAD_SCALE = 1.7                     # the upstream gradient of the loss: a device scalar that is not 1
HEADER = 8                           # words before tp / pred / true in the metrics buffer (include/kanconv.h)
PAD, SENT = 64, 0x7FA5A5A5           # sentinel words on each side of a guarded output (a NaN pattern no kernel writes)


def load_eval(name):
    return dict(np.load(os.path.join(EVAL, name + ".npz")))


def run_hip(logits, target, metrics=None):
    """(loss, lse, dlogits) of ops.cross_entropy on the device for CPU inputs, all back on the CPU."""
    from convkan_amd import ops
    lg = logits.cuda().requires_grad_(True)
    loss = ops.cross_entropy(lg, target.cuda(), metrics)
    lse = loss.grad_fn.saved_tensors[2]
    (loss * GRAD_SCALE).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), lse.detach().cpu(), lg.grad.cpu()


def run_cpu(logits, target, dtype):
    lg = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(lg, target)
    (loss * GRAD_SCALE).backward()
    return loss.detach(), torch.logsumexp(lg.detach(), 1), lg.grad


def scalar_err(a, ref):
    """|a - ref| relative to max(1, |ref|), elementwise maximum; infinities must agree exactly."""
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    inf = torch.isinf(ref)
    assert torch.equal(a[inf], ref[inf]), (a, ref)
    if bool(inf.all()):
        return 0.0
    return float((a[~inf] - ref[~inf]).abs().max() / max(1.0, float(ref[~inf].abs().max())))


def check_against_fp64(tag, logits, target, metrics=None):
    loss, lse, dl = run_hip(logits, target, metrics)
    l32, s32, d32 = run_cpu(logits, target, torch.float32)
    l64, s64, d64 = run_cpu(logits, target, torch.float64)
    rows = [("loss", scalar_err(loss, l64), max(TOL_Y, 4 * scalar_err(l32, l64))),
            ("lse", scalar_err(lse, s64), max(TOL_Y, 4 * scalar_err(s32, s64))),
            ("dlogits", relerr(dl, d64), max(TOL_DX, 4 * relerr(d32, d64)))]
    print(f"[xent {tag}] " + "  ".join(f"{n}: err {e:.2e} tol {t:.2e}" for n, e, t in rows))
    bad = [(n, e, t) for n, e, t in rows if not e <= t]
    assert not bad, (tag, bad)
    return loss, lse, dl


def cpu_counters(logits, target, Cn):
    """[correct, samples], tp, pred, true from fp32 logits on the CPU; torch.max returns the lowest index among the maxima."""
    pred = logits.max(1)[1]
    hit = pred == target
    return (int(hit.sum()), len(target), torch.bincount(target[hit], minlength=Cn), torch.bincount(pred, minlength=Cn),
            torch.bincount(target, minlength=Cn))


def assert_counters(m, logits, target, batches=1):
    Cn = logits.shape[1]
    host = m.buffer.cpu()
    correct, samples, tp, pred, true = cpu_counters(logits, target, Cn)
    assert host[:4].tolist() == [correct, samples, batches, 0], host[:4].tolist()
    got = host[HEADER:].reshape(3, Cn)
    assert torch.equal(got[0], tp) and torch.equal(got[1], pred) and torch.equal(got[2], true)
    return host


def make(B, Cn, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(B, Cn, generator=g), torch.randint(0, Cn, (B,), generator=g)


# ------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("B,Cn", SHAPES, ids=lambda v: str(v))
def test_loss_lse_dlogits_and_counters(B, Cn, gpu_lib):
    import convkan_amd as K
    logits, target = make(B, Cn, 100 + B + Cn)
    m = K.ClassMetrics(Cn, "cuda")
    loss, _, _ = check_against_fp64(f"{B}x{Cn}", logits, target, m)
    host = assert_counters(m, logits, target)
    assert float(host[4:5].view(torch.float64)) == float(loss)                  # one batch: loss_sum is that batch's fp32 mean
    r = m.result()
    assert r["accuracy"] == cpu_counters(logits, target, Cn)[0] / B and r["loss"] == float(loss) and (r["samples"], r["batches"]) == (B, 1)


def test_large_logits_need_the_max_subtracted(gpu_lib):
    logits, target = make(5, 10, 7, scale=3.0e4)
    loss, _, _ = check_against_fp64("5x10 scaled 1e4", logits, target)
    assert bool(torch.isfinite(loss))


def test_infinite_logits(gpu_lib):
    """-inf entries add nothing to a row's sum; a row whose TARGET logit is -inf has an infinite loss, as torch gives."""
    logits, target = make(4, 6, 11)
    ninf = float("-inf")
    logits[0, 1] = logits[0, 4] = logits[2, 0] = ninf
    target[0], target[2] = 2, 3
    check_against_fp64("4x6 with -inf, finite loss", logits, target)
    logits[1, 5], target[1] = ninf, 5
    loss, _, _ = check_against_fp64("4x6 with -inf at a target", logits, target)
    assert float(loss) == float("inf") and float(F.cross_entropy(logits, target)) == float("inf")


# ------------------------------------------------------------------------------------------ predictions: torch.max's tie rule
@pytest.mark.parametrize("name", [n for n in FIXTURES if n.startswith("ties")])
def test_ties_fixture_counters(name, gpu_lib):
    import convkan_amd as K
    d = load_eval(name)
    logits, target = torch.from_numpy(d["logits"]), torch.from_numpy(d["targets"])
    assert int((logits == logits.max(1, keepdim=True)[0]).sum(1).gt(1).sum()) > 0
    m = K.ClassMetrics(logits.shape[1], "cuda")
    run_hip(logits, target, m)
    assert_counters(m, logits, target)


@pytest.mark.parametrize("Cn,lo,hi", [(10, 2, 7), (130, 63, 64), (10, 0, 9), (200, 0, 199), (4097, 63, 4096)],
                         ids=lambda v: str(v))
def test_constructed_ties_take_the_lowest_index(Cn, lo, hi, gpu_lib):
    """The row maximum sits at exactly two indices, (63, 64) on the two sides of a wavefront's edge: the lower one is the prediction."""
    import convkan_amd as K
    B = 6
    logits = -torch.rand(B, Cn, generator=torch.Generator().manual_seed(Cn + lo))
    logits[:, lo] = logits[:, hi] = 5.0
    target = torch.tensor([lo, hi, lo, hi, (lo + 1) % Cn, hi])
    m = K.ClassMetrics(Cn, "cuda")
    run_hip(logits, target, m)
    host = assert_counters(m, logits, target)
    pred = host[HEADER:].reshape(3, Cn)[1]
    assert int(pred[lo]) == B and int(pred.sum()) == B and int(host[0]) == 2


# ------------------------------------------------------------------------------------------ determinism
def test_same_inputs_same_bits(gpu_lib):
    import convkan_amd as K
    logits, target = make(257, 10, 21)
    a = run_hip(logits, target)
    b = run_hip(logits, target)
    c = run_hip(logits, target, K.ClassMetrics(10, "cuda"))
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    big, tb = make(4100, 3, 22)                                       # the mean's loop and tree
    assert torch.equal(run_hip(big, tb)[0], run_hip(big, tb)[0])


def test_lse_of_a_row_does_not_depend_on_its_batch(gpu_lib):
    logits, target = make(257, 10, 23)
    _, lse257, _ = run_hip(logits, target)
    for rows in (slice(0, 5), slice(252, 257), slice(126, 131)):
        _, lse5, _ = run_hip(logits[rows].clone(), target[rows].clone())
        assert torch.equal(lse5, lse257[rows]), rows


# ------------------------------------------------------------------------------------------ out-of-range targets
def _guarded(n, dtype=torch.float32):
    """(buffer, view): n elements of `dtype` (4 or 8 bytes) placed PAD words into a larger int32 buffer filled with a sentinel."""
    words = n * (2 if dtype == torch.int64 else 1)
    buf = torch.full((words + 2 * PAD,), SENT, dtype=torch.int32, device="cuda")
    return buf, buf[PAD:PAD + words].view(dtype)


def _borders_intact(buf):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all())


def _direct(lib, logits, target, B, Cn, with_metrics=True):
    """kan_xent_fwd + kan_xent_bwd through the C ABI with every output, the workspace and the metrics buffer between sentinel words."""
    from convkan_amd import _lib as L

    def p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bufs, out = {}, {}
    for name, n, dt in (("loss", 1, torch.float32), ("lse", B, torch.float32), ("dlogits", B * Cn, torch.float32),
                        ("workspace", lib.kan_xent_workspace_bytes(B) // 4, torch.int32), ("metrics", lib.kan_xent_metrics_bytes(Cn) // 8, torch.int64)):
        bufs[name], out[name] = _guarded(n, dt)
    out["metrics"].zero_()
    g = torch.full((1,), GRAD_SCALE, device="cuda")
    L.check(lib.kan_xent_fwd(p(logits), p(target), B, Cn, p(out["loss"]), p(out["lse"]), p(out["metrics"] if with_metrics else None),
                             p(out["workspace"]), st), "fwd")
    L.check(lib.kan_xent_bwd(p(logits), p(target), p(out["lse"]), p(g), p(out["dlogits"]), B, Cn, st), "bwd")
    torch.cuda.synchronize()
    return out, bufs


def test_out_of_range_targets(gpu_lib):
    """One target equal to C and one equal to -1: flagged, 0 in the loss, in no counter, zero gradient rows; the other rows as without them;
    nothing written outside any buffer."""
    import convkan_amd as K
    from convkan_amd import _lib as L
    B, Cn = 9, 7
    logits, target = make(B, Cn, 31)
    bad_rows, good = [2, 5], [0, 1, 3, 4, 6, 7, 8]
    bad_target = target.clone()
    bad_target[2], bad_target[5] = Cn, -1
    lg = logits.cuda()
    clean, clean_bufs = _direct(gpu_lib, lg, target.cuda(), B, Cn)
    out, bufs = _direct(gpu_lib, lg, bad_target.cuda(), B, Cn)
    for name in bufs:
        assert _borders_intact(bufs[name]) and _borders_intact(clean_bufs[name]), name
    assert torch.equal(out["lse"], clean["lse"])
    d, dc = out["dlogits"].view(B, Cn).cpu(), clean["dlogits"].view(B, Cn).cpu()
    assert torch.equal(d[good], dc[good]) and bool((d[bad_rows] == 0).all()) and bool((dc[bad_rows] != 0).any())
    l64 = F.cross_entropy(logits[good].double(), target[good], reduction="sum") / B
    l32 = F.cross_entropy(logits[good], target[good], reduction="sum") / B
    err, tol = scalar_err(out["loss"].cpu(), l64), max(TOL_Y, 4 * scalar_err(l32, l64))
    print(f"[xent bad targets] loss err {err:.2e} tol {tol:.2e}")
    assert err <= tol
    host = out["metrics"].cpu()
    correct, samples, tp, pred, true = cpu_counters(logits[good], target[good], Cn)
    assert host[:4].tolist() == [correct, len(good), 1, 2]
    got = host[HEADER:].reshape(3, Cn)
    assert torch.equal(got[0], tp) and torch.equal(got[1], pred) and torch.equal(got[2], true)
    m = K.ClassMetrics(Cn, "cuda")
    m.buffer = out["metrics"]
    with pytest.raises(L.KanConvError, match="outside"):
        m.result()
    # the same through the op: sticky over a later clean batch, cleared by reset()
    m = K.ClassMetrics(Cn, "cuda")
    _, _, dl = run_hip(logits, bad_target, m)
    assert bool((dl[bad_rows] == 0).all())
    run_hip(logits, target, m)
    with pytest.raises(L.KanConvError, match="outside"):
        m.result()
    m.reset()
    run_hip(logits, target, m)
    assert m.result()["samples"] == B


# ------------------------------------------------------------------------------------------ the evaluation loop
@pytest.mark.parametrize("name", FIXTURES)
def test_evaluate_reproduces_the_reference(name, gpu_lib):
    """K.evaluate over an Identity model and the fixture's batches against what the reference's evaluations.test returned."""
    import convkan_amd as K
    d = load_eval(name)
    logits, target, bs = torch.from_numpy(d["logits"]), torch.from_numpy(d["targets"]), int(d["batch_size"])
    batches = [(logits[i:i + bs], target[i:i + bs]) for i in range(0, len(target), bs)]
    model = nn.Identity()
    model.train()
    r = K.evaluate(model, batches)
    assert model.training
    for key in ("accuracy", "precision", "recall", "f1"):
        assert abs(r[key] - float(d[key])) <= 1e-12, (key, r[key], float(d[key]))
    assert (r["samples"], r["batches"]) == (len(target), len(batches))
    l64 = torch.stack([F.cross_entropy(a.double(), b) for a, b in batches]).mean()
    err, tol = scalar_err(torch.tensor(r["loss"]), l64), max(TOL_Y, 4 * scalar_err(torch.tensor(float(d["loss"])), l64))
    print(f"[evaluate {name}] loss {r['loss']:.9f} reference {float(d['loss']):.9f} fp64 {float(l64):.9f} err {err:.2e} tol {tol:.2e}")
    assert err <= tol
    # a metrics object handed in is reset first and reused
    m = K.ClassMetrics(logits.shape[1], "cuda")
    K.ops.cross_entropy(logits.cuda(), target.cuda(), m)
    assert K.evaluate(model, batches, metrics=m) == r


def _small_model(classes):
    import convkan_amd as K
    return nn.Sequential(K.KANConv2DLayer(3, 8, 3, padding=1), nn.Flatten(), nn.Linear(8 * 8 * 8, classes))


def test_train_step_takes_the_criterion(gpu_lib):
    """Three K.train_step calls with criterion=K.CrossEntropyLoss(metrics=m): the losses are those of torch's criterion on the same logits (the
    rule above), and m holds the training counts of exactly those logits -- with no host read in the loop."""
    import convkan_amd as K
    torch.manual_seed(5)
    model = _small_model(10).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(16, 3, 8, 8, device="cuda", generator=g), torch.randint(0, 10, (16,), device="cuda", generator=g)) for _ in range(3)]
    seen = []
    model.register_forward_hook(lambda mod, args, out: seen.append(out.detach().clone()))
    m = K.ClassMetrics(10, "cuda")
    crit = K.CrossEntropyLoss(metrics=m)
    opt = K.FusedAdamW(model.parameters(), lr=1e-3)
    losses = [K.train_step(model, d, t, opt, criterion=crit) for d, t in batches]
    assert all(l.is_cuda and not l.requires_grad for l in losses)
    logits, target = torch.cat(seen).cpu(), torch.cat([t for _, t in batches]).cpu()
    host = assert_counters(m, logits, target, batches=3)
    for i, (loss, (_, t)) in enumerate(zip(losses, batches)):
        l64, l32 = F.cross_entropy(seen[i].double().cpu(), t.cpu()), F.cross_entropy(seen[i].cpu(), t.cpu())
        assert scalar_err(loss.cpu(), l64) <= max(TOL_Y, 4 * scalar_err(l32, l64))
    assert float(host[4:5].view(torch.float64)) == sum(float(l) for l in losses)
    assert m.result()["samples"] == 48 and losses[0].item() != losses[2].item()


def test_train_and_test_models(gpu_lib):
    """Two epochs on 64 separable samples: seven lists of two, learning rates following gamma, and test metrics equal to those recomputed on
    the CPU from the model's own logits (exact: the same integers through the same fp64 formulas)."""
    import convkan_amd as K
    torch.manual_seed(9)
    classes, gamma, lr = 4, 0.5, 1e-2
    target = torch.arange(64) % classes
    data = 0.3 * torch.randn(64, 3, 8, 8)
    for i, t in enumerate(target.tolist()):                          # class = which quadrant is bright (InstanceNorm keeps spatial structure)
        data[i, :, 4 * (t // 2):4 * (t // 2) + 4, 4 * (t % 2):4 * (t % 2) + 4] += 1.5
    train = [(data[i:i + 16], target[i:i + 16]) for i in range(0, 64, 16)]
    test = [(data[i:i + 24], target[i:i + 24]) for i in range(0, 64, 24)]                    # 24, 24, 16
    model = _small_model(classes).cuda()
    opt = K.FusedAdamW(model.parameters(), lr=lr, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=gamma)
    out = K.train_and_test_models(model, train, test, opt, sched, epochs=2)
    assert len(out) == 7 and all(isinstance(h, list) and len(h) == 2 for h in out)
    train_loss, test_loss, acc, prec, rec, f1, rates = out
    assert rates == pytest.approx([lr, lr * gamma], rel=1e-12) and opt.param_groups[0]["lr"] == pytest.approx(lr * gamma ** 2, rel=1e-12)
    assert all(np.isfinite(v) for h in out for v in h)
    assert model.training
    model.eval()
    with torch.no_grad():
        logits = [model(d.cuda()).cpu() for d, _ in test]
    all_logits = torch.cat(logits)
    correct, samples, tp, pred, true = cpu_counters(all_logits, target, classes)
    l64 = torch.stack([F.cross_entropy(a.double(), t) for a, (_, t) in zip(logits, test)]).mean()
    l32 = torch.stack([F.cross_entropy(a, t) for a, (_, t) in zip(logits, test)]).mean()
    want = K.ClassMetrics.summarize(tp, pred, true, correct, samples, len(test), 0.0)
    assert (acc[1], prec[1], rec[1], f1[1]) == (want["accuracy"], want["precision"], want["recall"], want["f1"])
    err, tol = scalar_err(torch.tensor(test_loss[1]), l64), max(TOL_Y, 4 * scalar_err(l32, l64))
    print(f"[train_and_test_models] train {train_loss} test {test_loss} acc {acc}  test-loss err {err:.2e} tol {tol:.2e}")
    assert err <= tol

"""Every cell of the InstanceNorm (+ PReLU, + max-pool) dispatch against the fp64 reference (tests/norm_cells.py: one row per kernel
variant and per side of every switch point, kept complete by tests/test_norm_matrix.py).

Per row, through ops._norm_fwd / ops._norm_bwd (the only callers of the six kan_instnorm_prelu* entry points):
  - the launch must still route to the row's declared keys, so the GPU really ran that variant;
  - y, mean, rstd, the summed z (S > 1), dz and the parameter gradients against fp64; on a pooled row the kernel's argmax bytes must
    EQUAL the first maximum in scan order of the fp64 reference on every window the conditioning leaves in (exact ties included);
  - a second run -- through a test-side copy of the launchers' argument marshalling that places y, pidx, mean, rstd, the summed z
    and dz inside larger buffers filled with a sentinel -- must be bit-identical in all of those (no atomics there; the parameter
    gradients use float atomics and are exempt) and must leave the sentinels on both sides of every output untouched.

Tolerance, per tensor: max(floor, 4 x the error of the fp32 CPU execution of the same reference against fp64, measured live).
Floors: 2e-6 for y, mean, rstd, z and dz (test_gpu_pool.py's figure for this kernel's output), 2e-5 for the parameter gradients
(helpers.check_vs_oracle).  Tensors are normalised by the reference's largest element; each slope gradient by the reference's
sum |n g| over that slope's elements on the negative side, not by its net value, which may cancel.  The summed z is also held
to the fp32 sum of the slabs, within what two fp32 summation orders can differ by.  Measured figures: DESIGN.md."""
import ctypes as C

import pytest
import torch

from norm_cells import EPS, NORM_CASES, case_ids, norm_key, pool_args, reference_pair, route

pytestmark = pytest.mark.gpu

FLOOR = dict(y=2e-6, mean=2e-6, rstd=2e-6, z=2e-6, dz=2e-6, dgamma=2e-5, dbeta=2e-5, dslope=2e-5)
PAD = 64                      # sentinel elements on each side of a guarded output
SENT_F, SENT_B = 0x7FA5A5A5, 0xA5      # (a NaN pattern no kernel writes)


def _guarded(shape, dtype=torch.float32):
    """(buffer, view): a tensor of `shape` placed PAD elements into a larger buffer filled with a sentinel."""
    n = 1
    for d in shape:
        n *= d
    if dtype == torch.uint8:
        buf = torch.full((n + 2 * PAD,), SENT_B, dtype=torch.uint8, device="cuda")
    else:
        buf = torch.full((n + 2 * PAD,), SENT_F, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[PAD:PAD + n].view(shape)


def _borders_intact(buf):
    raw = buf if buf.dtype == torch.uint8 else buf.view(torch.int32)
    want = SENT_B if buf.dtype == torch.uint8 else SENT_F
    return bool((raw[:PAD] == want).all()) and bool((raw[-PAD:] == want).all())


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _guarded_run(case, zs, go, gamma, beta, slope):
    """ops._norm_fwd + ops._norm_bwd's argument marshalling with every output inside a guarded buffer.  Returns ({name: view}, {name: buffer})."""
    from convkan_amd import _lib as L
    lib = L.load()
    S, B, Ct, H, W = zs.shape
    HW, span = H * W, (Ct // case["groups"] if case["groups"] > 1 else 0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p2, pk, ps = pool_args(case["pool"], H, W)
    k, s = (2, 2) if p2 else (pk, ps)
    yshape = (B, Ct, (H - k) // s + 1, (W - k) // s + 1) if case["pool"] else (B, Ct, H, W)
    bufs, out = {}, {}
    for name, shape, dt in (("y", yshape, torch.float32), ("mean", (B * Ct,), torch.float32), ("rstd", (B * Ct,), torch.float32),
                            ("dz", (B, Ct, H, W), torch.float32)) + ((("pidx", yshape, torch.uint8),) if case["pool"] else ()) + \
                           ((("z", (B, Ct, H, W), torch.float32),) if S > 1 else ()):
        bufs[name], out[name] = _guarded(shape, dt)
    z = out["z"] if S > 1 else zs[0]
    head = (_p(zs), S, B * Ct * HW, _p(z), _p(gamma), _p(beta), _p(slope), _p(out["y"]))
    if not case["pool"]:
        L.check(lib.kan_instnorm_prelu_fwd(*head, _p(out["mean"]), _p(out["rstd"]), B, Ct, HW, Ct * HW, EPS, span, st), "fwd")
    elif p2:
        L.check(lib.kan_instnorm_prelu_pool_fwd(*head, _p(out["pidx"]), _p(out["mean"]), _p(out["rstd"]), B, Ct, H, W, Ct * HW, EPS, span, st), "pool_fwd")
    else:
        L.check(lib.kan_instnorm_prelu_poolk_fwd(*head, _p(out["pidx"]), _p(out["mean"]), _p(out["rstd"]), B, Ct, H, W, Ct * HW, EPS, span, pk, ps, st),
                "poolk_fwd")
    grads = [torch.zeros_like(t) if t is not None else None for t in (gamma, beta, slope)]
    tail = (_p(z), _p(out["mean"]), _p(out["rstd"]), _p(gamma), _p(beta), _p(slope), _p(out["dz"]), *(_p(g) for g in grads), B, Ct)
    if not case["pool"]:
        L.check(lib.kan_instnorm_prelu_bwd(_p(go), *tail, HW, Ct * HW, span, st), "bwd")
    elif p2:
        L.check(lib.kan_instnorm_prelu_pool_bwd(_p(go), _p(out["pidx"]), *tail, H, W, Ct * HW, span, st), "pool_bwd")
    else:
        L.check(lib.kan_instnorm_prelu_poolk_bwd(_p(go), _p(out["pidx"]), *tail, H, W, Ct * HW, span, pk, ps, st), "poolk_bwd")
    torch.cuda.synchronize()
    return out, bufs


def _slabs_on_device(case, zs):
    """The slabs on the GPU; kind "unaligned": starting one float into their storage, so that data_ptr() & 7 == 4."""
    if case["kind"] != "unaligned":
        return zs.cuda()
    store = torch.empty(zs.numel() + 1, device="cuda")
    view = store[1:].view(zs.shape)
    view.copy_(zs)
    assert view.data_ptr() & 7 == 4
    return view


@pytest.mark.parametrize("idx", range(len(NORM_CASES)), ids=case_ids(NORM_CASES))
def test_norm_cell_vs_fp64(idx, gpu_lib):
    from convkan_amd import ops
    case = NORM_CASES[idx]
    (zs, gamma, beta, slope), go, mask, pidx64, r64, r32 = reference_pair(idx)
    S, B, Ct, H, W = zs.shape
    zs1, zs2 = _slabs_on_device(case, zs), _slabs_on_device(case, zs)
    aligned = zs1.data_ptr() & 7 == 0
    keys = tuple(norm_key(route(bwd, B, Ct, H, W, S, case["pool"], aligned), bwd) for bwd in (False, True))
    assert keys == (case["fwd"], case["bwd"]), f"{case}: the launch routes to {keys}"
    gamma, beta, slope = (t.cuda() if t is not None else None for t in (gamma, beta, slope))
    god, pool = go.cuda(), case["pool"] or False

    # one slab: the [B, C, H, W] tensor itself (z_out aliases it); more: the [S, B, C, H, W] stack
    y, z, mean, rstd, pidx = ops._norm_fwd(zs1 if S > 1 else zs1[0], B * Ct * H * W, gamma, beta, slope, EPS, case["groups"], pool)
    dz, dgam, dbet, dslo = ops._norm_bwd(god, z, mean, rstd, gamma, beta, slope, pidx, case["groups"], pool)
    torch.cuda.synchronize()
    got = dict(y=y, mean=mean, rstd=rstd, dz=dz, dgamma=dgam, dbeta=dbet, dslope=dslo, z=z if S > 1 else None)
    again, bufs = _guarded_run(case, zs2, god, gamma, beta, slope)

    bad, line = [], []
    for name, floor in FLOOR.items():
        if got[name] is None:
            assert r64.get(name) is None or name == "z", name
            continue
        a, b64, b32 = got[name].detach().double().cpu().reshape(-1), r64[name].reshape(-1), r32[name].double().reshape(-1)
        # (a slope gradient: each slope against its own sum |n g|, the largest ratio counts)
        scale = r64["dslope_scale"].reshape(-1) if name == "dslope" else b64.abs().max()
        err, noise = float(((a - b64).abs() / (scale + 1e-30)).max()), float(((b32 - b64).abs() / (scale + 1e-30)).max())
        tol = max(floor, 4.0 * noise)
        line.append(f"{name} {err:.1e} (tol {tol:.1e}, fp32 reference {noise:.1e})")
        if not err <= tol:
            worst = int((a - b64).abs().argmax())
            bad.append(f"{name}: error {err:.3e} > {tol:.3e} (fp32 reference {noise:.3e}); worst flat index {worst}: {float(a[worst])} vs {float(b64[worst])}")
    if S > 1:
        # the summed z against the fp32 sum of the slabs taken in order: both are fp32 sums of the same S terms, each within
        # (S - 1) 2^-24 sum |z_s| of the exact sum whatever its order, so they differ by at most twice that, element by element
        seq = zs[0].clone()
        for sl in range(1, S):
            seq += zs[sl]
        over = (z.cpu() - seq).abs() - 2 * (S - 1) * 2.0 ** -24 * zs.abs().sum(0)
        if float(over.max()) > 0:
            bad.append(f"z: {int((over > 0).sum())} elements further from the in-order fp32 sum of the slabs than two fp32 sums of {S} terms can be")
    print(f"[norm] {case['fwd']} | {case['bwd']} | {case_ids([case])[0]}: " + "; ".join(line))
    if case["pool"]:
        keep = ~mask
        if not torch.equal(pidx.cpu()[keep], pidx64[keep]):
            w = (pidx.cpu() != pidx64) & keep
            bad.append(f"pidx: {int(w.sum())} unmasked windows pick another element than the first fp64 maximum, first at {w.nonzero()[0].tolist()}")
    for name in ("y", "mean", "rstd", "dz") + (("pidx",) if case["pool"] else ()) + (("z",) if S > 1 else ()):
        first = pidx if name == "pidx" else got[name]
        if not torch.equal(first.reshape(-1), again[name].reshape(-1)):
            bad.append(f"{name}: two runs on the same inputs differ in {int((first.reshape(-1) != again[name].reshape(-1)).sum())} elements")
        if not _borders_intact(bufs[name]):
            bad.append(f"{name}: memory next to the tensor was written")
    assert not bad, f"{case}:\n  " + "\n  ".join(bad)

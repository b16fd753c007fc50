"""Every row of the BatchNorm (+ PReLU, + 2x2 max-pool) cell matrix (tests/bnorm_cells.py) against the fp64 reference, through
ops._norm_fwd / ops._norm_bwd with the batch-norm descriptor (the only callers of the kan_batchnorm_prelu* entry points).

Per row:
  - y, the summed z (S > 1), mean, rstd, the updated running_mean / running_var, dz, dgamma, dbeta and dslope against fp64; on a pooled
    row the kernel's argmax bytes must EQUAL the first maximum in scan order of the fp64 reference on every window the conditioning
    leaves in;
  - a second run -- through a test-side copy of the launchers' argument marshalling that places every output, the parameter gradients
    and the running buffers included, inside larger buffers filled with a sentinel -- must be bit-identical in all of them (this path
    accumulates nothing with atomics) and must leave the sentinels on both sides of every output untouched;
  - the running buffers of a training=0 row are unchanged, bit for bit.

Tolerance, per tensor: max(floor, 4 x the error of the fp32 CPU execution of the same reference against fp64, measured live).  Floors
are test_gpu_norm_matrix.py's: 2e-6 for data and statistics, 2e-5 for the parameter gradients.  Tensors are normalised by the
reference's largest element; each slope gradient by the reference's sum |n g| over that slope's elements on the negative side.
Measured figures: DESIGN.md section 4c."""
import ctypes as C

import pytest
import torch

from bnorm_cells import BNORM_CASES, EPS, MOMENTUM, case_id, reference_pair

pytestmark = pytest.mark.gpu

FLOOR = dict(y=2e-6, z=2e-6, mean=2e-6, rstd=2e-6, running_mean=2e-6, running_var=2e-6, dz=2e-6, dgamma=2e-5, dbeta=2e-5, dslope=2e-5)
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


def _guarded_run(case, zs, go, gamma, beta, slope, rmean, rvar):
    """ops._norm_fwd + ops._norm_bwd's argument marshalling for the BatchNorm entry points, every output inside a guarded buffer.
    Returns ({name: view}, {name: buffer})."""
    from convkan_amd import _lib as L
    lib = L.load()
    S, B, Ct, H, W = zs.shape
    span = Ct // case["groups"] if case["groups"] > 1 else 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    yshape = (B, Ct, H // 2, W // 2) if case["pool"] else (B, Ct, H, W)
    wanted = [("y", yshape, torch.float32), ("mean", (Ct,), torch.float32), ("rstd", (Ct,), torch.float32), ("dz", (B, Ct, H, W), torch.float32)]
    wanted += [("pidx", yshape, torch.uint8)] if case["pool"] else []
    wanted += [("z", (B, Ct, H, W), torch.float32)] if S > 1 else []
    wanted += [(n, (Ct,), torch.float32) for n, t in (("dgamma", gamma), ("dbeta", beta), ("running_mean", rmean), ("running_var", rvar)) if t is not None]
    wanted += [("dslope", tuple(slope.shape), torch.float32)] if slope is not None else []
    bufs, out = {}, {}
    for name, shape, dt in wanted:
        bufs[name], out[name] = _guarded(shape, dt)
    if rmean is not None:
        out["running_mean"].copy_(rmean)
        out["running_var"].copy_(rvar)
    z = out["z"] if S > 1 else zs[0]
    ws = torch.empty(lib.kan_batchnorm_workspace_bytes(B, Ct), dtype=torch.uint8, device="cuda")
    L.check(lib.kan_batchnorm_prelu_fwd(_p(zs), S, B * Ct * H * W, _p(z), _p(gamma), _p(beta), _p(slope), _p(out["y"]), _p(out.get("pidx")), _p(out["mean"]),
                                        _p(out["rstd"]), _p(out.get("running_mean")), _p(out.get("running_var")), _p(ws), B, Ct, H, W, Ct * H * W, EPS,
                                        MOMENTUM, span, int(case["training"]), st), "fwd")
    batch = case["training"] or rmean is None
    L.check(lib.kan_batchnorm_prelu_bwd(_p(go), _p(out.get("pidx")), _p(z), _p(out["mean"]), _p(out["rstd"]), _p(gamma), _p(beta), _p(slope), _p(out["dz"]),
                                        _p(out.get("dgamma")), _p(out.get("dbeta")), _p(out.get("dslope")), _p(ws), B, Ct, H, W, Ct * H * W, span,
                                        int(batch), st), "bwd")
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


@pytest.mark.parametrize("idx", range(len(BNORM_CASES)), ids=[case_id(c) for c in BNORM_CASES])
def test_bnorm_cell_vs_fp64(idx, gpu_lib):
    from convkan_amd import ops
    case = BNORM_CASES[idx]
    inputs, go, mask, pidx64, r64, r32 = reference_pair(idx)
    f32 = lambda t: t.float() if t is not None else None
    zs, gamma, beta, slope, rmean, rvar = (f32(inputs[k]) for k in ("zs", "gamma", "beta", "slope", "rmean", "rvar"))
    S, B, Ct, H, W = zs.shape
    zs1, zs2 = _slabs_on_device(case, zs), _slabs_on_device(case, zs)
    gamma, beta, slope, rmean, rvar = (t.cuda() if t is not None else None for t in (gamma, beta, slope, rmean, rvar))
    run_m, run_v = (t.clone() if t is not None else None for t in (rmean, rvar))
    bn = ops.BatchStats(run_m, run_v, MOMENTUM, case["training"])
    god, pool = go.cuda(), case["pool"] or False

    # one slab: the [B, C, H, W] tensor itself (z_out aliases it); more: the [S, B, C, H, W] stack
    y, z, mean, rstd, pidx = ops._norm_fwd(zs1 if S > 1 else zs1[0], B * Ct * H * W, gamma, beta, slope, EPS, case["groups"], pool, bn=bn)
    dz, dgam, dbet, dslo = ops._norm_bwd(god, z, mean, rstd, gamma, beta, slope, pidx, case["groups"], pool, bn=bn)
    torch.cuda.synchronize()
    assert mean.shape == rstd.shape == (Ct,)
    got = dict(y=y, mean=mean, rstd=rstd, running_mean=run_m, running_var=run_v, dz=dz, dgamma=dgam, dbeta=dbet, dslope=dslo, z=z if S > 1 else None)
    again, bufs = _guarded_run(case, zs2, god, gamma, beta, slope, rmean, rvar)

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
    print(f"[bnorm] {case_id(case)}: " + "; ".join(line))
    if case["pool"]:
        keep = ~mask
        if not torch.equal(pidx.cpu()[keep], pidx64[keep]):
            w = (pidx.cpu() != pidx64) & keep
            bad.append(f"pidx: {int(w.sum())} unmasked windows pick another element than the first fp64 maximum, first at {w.nonzero()[0].tolist()}")
    if not case["training"] and rmean is not None:
        if not (torch.equal(run_m, rmean) and torch.equal(run_v, rvar)):
            bad.append("an eval-mode launch changed the running buffers")
    got["pidx"] = pidx
    for name in again:
        if not torch.equal(got[name].reshape(-1), again[name].reshape(-1)):
            bad.append(f"{name}: two runs on the same inputs differ in {int((got[name].reshape(-1) != again[name].reshape(-1)).sum())} elements")
        if not _borders_intact(bufs[name]):
            bad.append(f"{name}: memory next to the tensor was written")
    assert not bad, f"{case}:\n  " + "\n  ".join(bad)


def test_single_value_per_channel_raises(gpu_lib):
    """torch: "Expected more than 1 value per channel when training"."""
    from convkan_amd import ops
    x = torch.randn(1, 3, 1, 1, device="cuda")
    with pytest.raises(ValueError):
        ops.batch_norm(x, training=True)
    assert torch.isfinite(ops.batch_norm(x, None, None, torch.zeros(3, device="cuda"), torch.ones(3, device="cuda"), False)).all()

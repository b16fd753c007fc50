"""Every cell of the Wav-KAN wavelet stage's dispatch against the fp64 reference (tests/wav_cells.py: one row per reachable key of
the forward, the input-gradient and the parameter-gradient launch and per side of every switch point, kept complete by
tests/test_wav_matrix.py).

Per row:
  - the launch must still route to the row's declared keys, so the GPU really ran those kernels;
  - ops.wav_stage forward and backward (all four inputs require grad, fixed du): u, dx, dw, dscale and dtrans against fp64;
  - a second run -- through a test-side copy of ops._WavStage's argument marshalling that places u, dx, dw, dscale, dtrans and the
    partial-sum workspace (exactly kan_wav_param_workspace floats) inside larger buffers filled with a sentinel -- must be
    bit-identical in all five tensors (fixed-order partial sums, no atomics: DESIGN.md section 9) and must leave the sentinels on
    both sides of every buffer untouched;
  - `bstride` rows once more with x / du / u / dx laid out with a batch stride larger than dense (the C ABI's x_bstride / u_bstride):
    the gaps of x and du hold NaN, those of u and dx the sentinel; the results must be bit-identical to the dense run and the gaps
    untouched;
  - the `refuse` row: ops.wav_stage raises KanConvError (the forward tile does not fit LDS; decided on the host, nothing is launched).

Tolerance, per tensor: max(stated, 4 x the error of the fp32 CPU execution of the same reference against fp64, measured live);
stated: helpers.TOL_Y / TOL_DX / TOL_DW for u / dx / dw, 2e-5 for dscale and dtrans (helpers.check_vs_oracle's figure for parameter
tensors below three dimensions).  Tensors are normalised by the fp64 reference's largest element.  Measured figures: DESIGN.md."""
import ctypes as C

import pytest
import torch

from helpers import TOL_DW, TOL_DX, TOL_Y
from wav_cells import WAV_CASES, WAVELETS, _pair, case_geom, case_id, case_ids, case_keys, reference_pair, route_of, wav_key

pytestmark = pytest.mark.gpu

STATED = dict(u=TOL_Y, dx=TOL_DX, dw=TOL_DW, dscale=2e-5, dtrans=2e-5)
PAD = 64                      # sentinel elements on each side of a guarded buffer
SENT = 0x7FA5A5A5             # (a NaN pattern no kernel writes)
GAP_X, GAP_U = 7, 5           # extra elements between consecutive images on the bstride rows


def _guarded(rows, per, gap=0, data=None):
    """(buffer, [rows, per] view): `rows` runs of `per` floats, `gap` more between consecutive runs, PAD elements in from both ends of a
    buffer filled with the sentinel.  data: the runs' contents; the gaps then hold NaN."""
    buf = torch.full((rows * (per + gap) + 2 * PAD,), SENT, dtype=torch.int32, device="cuda").view(torch.float32)
    body = buf[PAD:PAD + rows * (per + gap)].view(rows, per + gap)
    if data is not None:
        body.fill_(float("nan"))
        body[:, :per].copy_(data.reshape(rows, per))
    return buf, body[:, :per]


def _untouched(buf, rows, per, gap, inputs=False):
    """The borders of a guarded buffer, and the gaps between its runs, still hold what _guarded put there."""
    raw = buf.view(torch.int32)
    ok = bool((raw[:PAD] == SENT).all()) and bool((raw[-PAD:] == SENT).all())
    if gap:
        gaps = buf[PAD:PAD + rows * (per + gap)].view(rows, per + gap)[:, per:]
        ok = ok and bool(gaps.isnan().all() if inputs else (gaps.view(torch.int32) == SENT).all())
    return ok


def _p(t):
    return C.c_void_p(t.data_ptr())


def _guarded_run(case, x, scale, trans, w, du, gap_x=0, gap_u=0):
    """ops._WavStage's marshalling (forward, bwd-input, bwd-params) with every output and the workspace inside guarded buffers.
    Returns ({name: tensor}, [names of buffers that were written outside their tensors])."""
    from convkan_amd import _lib as L
    lib = L.load()
    B, Cn, H, W = x.shape
    O = w.shape[0]
    geom = case_geom(case, Cn * H * W + gap_x, None)
    geom.u_bstride = O * geom.Ho * geom.Wo + gap_u
    nx, nu = Cn * H * W, O * geom.Ho * geom.Wo
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xb, xv = _guarded(B, nx, gap_x, x)
    dub, duv = _guarded(B, nu, gap_u, du)
    ub, uv = _guarded(B, nu, gap_u)
    dxb, dxv = _guarded(B, nx, gap_x)
    n_ws = lib.kan_wav_param_workspace(C.byref(geom))
    assert n_ws == route_of(geom).chunks * O * Cn * (w.shape[2] * w.shape[3] + 2)
    wsb, wsv = _guarded(1, n_ws)
    dwb, dwv = _guarded(1, w.numel())
    dsb, dsv = _guarded(1, scale.numel())
    dtb, dtv = _guarded(1, trans.numel())
    L.check(lib.kan_wav_fwd(_p(xv), _p(scale), _p(trans), _p(w), _p(uv), C.byref(geom), st), "kan_wav_fwd")
    L.check(lib.kan_wav_bwd_input(_p(duv), _p(xv), _p(scale), _p(trans), _p(w), _p(dxv), C.byref(geom), st), "kan_wav_bwd_input")
    L.check(lib.kan_wav_bwd_params(_p(duv), _p(xv), _p(scale), _p(trans), _p(w), _p(dwv), _p(dsv), _p(dtv), _p(wsv), C.byref(geom), st),
            "kan_wav_bwd_params")
    torch.cuda.synchronize()
    out = dict(u=uv.reshape(B, O, geom.Ho, geom.Wo), dx=dxv.reshape(x.shape), dw=dwv.reshape(w.shape), dscale=dsv.reshape(scale.shape),
               dtrans=dtv.reshape(trans.shape))
    checks = (("x", xb, B, nx, gap_x, True), ("du", dub, B, nu, gap_u, True), ("u", ub, B, nu, gap_u, False), ("dx", dxb, B, nx, gap_x, False),
              ("workspace", wsb, 1, n_ws, 0, False), ("dw", dwb, 1, w.numel(), 0, False), ("dscale", dsb, 1, scale.numel(), 0, False),
              ("dtrans", dtb, 1, trans.numel(), 0, False))
    return out, [name for name, buf, rows, per, gap, inp in checks if not _untouched(buf, rows, per, gap, inp)]


@pytest.mark.parametrize("idx", range(len(WAV_CASES)), ids=case_ids(WAV_CASES))
def test_wav_cell_vs_fp64(idx, gpu_lib):
    from convkan_amd import _lib as L
    from convkan_amd import ops
    case = WAV_CASES[idx]
    wt, geo = WAVELETS.index(case["wavelet"]), (_pair(case["s"]), _pair(case["p"]), _pair(case["d"]))
    assert case_keys(case) == (case["fwd"], case["bi"], case["par"]), f"{case_id(case)}: the launch routes to {case_keys(case)}"
    if case["kind"] == "refuse":
        kh, kw = _pair(case["k"])
        x, par, w = torch.randn(case["B"], case["C"], case["H"], case["W"]), torch.ones(case["O"], case["C"]), torch.randn(case["O"], case["C"], kh, kw)
        with pytest.raises(L.KanConvError, match="does not fit in LDS"):
            ops.wav_stage(wt, x.cuda(), par.cuda(), par.cuda(), w.cuda(), *geo)
        torch.cuda.synchronize()
        return
    inputs, r64, r32 = reference_pair(idx)
    assert all(float(v.abs().max()) > 0 for v in r64.values()), f"{case_id(case)}: a reference tensor is all zero"
    x, scale, trans, w, du = (t.cuda() for t in inputs)
    leaves = [t.clone().requires_grad_(True) for t in (x, scale, trans, w)]
    u = ops.wav_stage(wt, *leaves, *geo)
    u.backward(du)
    torch.cuda.synchronize()
    got = dict(u=u.detach(), dx=leaves[0].grad, dscale=leaves[1].grad, dtrans=leaves[2].grad, dw=leaves[3].grad)
    again, written = _guarded_run(case, x, scale, trans, w, du)

    bad, line = [], []
    for name, stated in STATED.items():
        a, b64, b32 = got[name].double().cpu().reshape(-1), r64[name].reshape(-1), r32[name].double().reshape(-1)
        top = float(b64.abs().max())
        err, noise = float((a - b64).abs().max()) / top, float((b32 - b64).abs().max()) / top
        tol = max(stated, 4.0 * noise)
        line.append(f"{name} {err:.1e} (tol {tol:.1e}, fp32 reference {noise:.1e})")
        if not err <= tol:
            worst = int((a - b64).abs().argmax())
            bad.append(f"{name}: error {err:.3e} > {tol:.3e} (fp32 reference {noise:.3e}); worst flat index {worst}: {float(a[worst])} vs {float(b64[worst])}")
    print(f"[wav] {case['fwd']} | {case['bi']} | {case['par']} | {case_id(case)}: " + "; ".join(line))
    runs = [("a second run", again, written)]
    if case["kind"] == "bstride":
        runs.append(("the batch-strided run", *_guarded_run(case, x, scale, trans, w, du, GAP_X, GAP_U)))
    for what, res, touched in runs:
        for name in STATED:
            if not torch.equal(got[name], res[name]):
                bad.append(f"{name}: {what} differs from the first in {int((got[name] != res[name]).sum())} elements")
        bad += [f"{name}: {what} wrote next to the tensor (or into a gap between images)" for name in touched]
    assert not bad, f"{case_id(case)}:\n  " + "\n  ".join(bad)

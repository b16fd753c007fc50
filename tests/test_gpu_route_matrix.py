"""Every route cell of the planner against the fp64 oracle (tests/route_cells.py: one row per reachable (spec class, fwd, bwd-data,
bwd-weight) cell, kept complete by tests/test_route_matrix.py).

Per row: the layer's plan must still be the row's cell (so the GPU really ran that route); forward, input gradient and every
parameter gradient must meet check_vs_oracle's tolerance against the oneDNN fp32 execution alone (fallback=False); and two runs on
the same inputs must give bit-identical y, dx and conv-weight gradients -- split-K slabs are summed in a fixed order and the data
path has no float atomics (test_training_step_is_bitwise_deterministic), so a difference is a race (slab writes, LDS reuse,
longest-first / XCD tile orders)."""
import pytest
import torch

from helpers import check_vs_oracle
from route_cells import ROUTE_CASES, case_cfg, case_ids, case_layer, case_structs, route_key

pytestmark = pytest.mark.gpu


def _perturb(layer, case, gen):
    """Trainable basis parameters away from their init, as test_gpu_fuzz.test_random_family_vs_oracle does."""
    with torch.no_grad():
        if hasattr(layer, "phase_low"):                   # ReLU-KAN: phases drift apart per channel and plane
            layer.phase_low.add_(0.06 * torch.randn(layer.phase_low.shape, generator=gen))
            layer.phase_high.add_(0.06 * torch.randn(layer.phase_high.shape, generator=gen))
        if hasattr(layer, "beta_weights"):                # GRAM-KAN: recurrence coefficients away from their ~1e-3 init
            layer.beta_weights.copy_(0.2 * torch.randn(layer.beta_weights.shape, generator=gen))
        if case.get("affine"):
            for m in layer.layer_norm:
                m.weight.add_(0.2 * torch.randn(m.weight.shape, generator=gen))
                m.bias.add_(0.2 * torch.randn(m.bias.shape, generator=gen))


def _run(layer, x, go):
    layer.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    y = layer(xg)
    y.backward(go)
    torch.cuda.synchronize()
    dw = {n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None and p.dim() >= 3 and not n.startswith("phase")}
    return y.detach().clone(), xg.grad.clone(), dw


@pytest.mark.parametrize("case", ROUTE_CASES, ids=case_ids(ROUTE_CASES))
def test_route_cell_vs_oracle(case, gpu_lib):
    torch.manual_seed(0)
    layer = case_layer(case)
    gen = torch.Generator().manual_seed(1)
    _perturb(layer, case, gen)
    g, b, p = case_structs(case, layer)
    assert route_key(g, b, p) == case["key"], f"{case}: the layer plans to {route_key(g, b, p)}"
    x = torch.randn(case["B"], case["C"], case["H"], case["W"], generator=gen) * case.get("scale", 1.0)
    check_vs_oracle(layer, case_cfg(case, layer), x, groups=case["G"], tag=case, fallback=False)

    xd = x.cuda()
    go = torch.randn(layer(xd).shape, generator=gen).cuda()
    y1, dx1, dw1 = _run(layer, xd, go)
    y2, dx2, dw2 = _run(layer, xd, go)
    assert torch.equal(y1, y2), f"{case}: forward differs between two identical runs"
    assert torch.equal(dx1, dx2), f"{case}: input gradient differs between two identical runs"
    assert dw1.keys() == dw2.keys() and dw1, f"{case}: no conv-weight gradients to compare"
    for n in dw1:
        assert torch.equal(dw1[n], dw2[n]), f"{case}: gradient of {n} differs between two identical runs"

#!/usr/bin/env python3
"""Golden vectors for the MLP KAN heads with one [I, O, degree + 1] coefficient tensor (ChebyKAN and the six recurrence families),
from the REFERENCE itself: its layer classes, imported unmodified, run on CPU in fp32 and once more in fp64.

The fixtures go to tests/golden/heads/<family>_<case>.npz -- a subdirectory, so the enumerations of tests/golden/*.npz
(conftest.golden_cases, make_plan_snapshot.py) see nothing new.  Each file holds
    cfg (JSON)             family, B, I, O, degree, extra constructor arguments; for the model fixture layers_hidden and l1_decay
    x ~ N(0, 1), g         input and upstream gradient
    sd.*                   the reference module's state_dict
    y, dx, grad.*          its fp32 forward / backward
    y64, dx64, grad64.*    the same module, same values, run under torch.set_default_dtype(torch.float64) (the reference allocates
                           its basis tensors with the default dtype)
A parameter-only dependence (Fibonacci degree 1: the basis is constant) leaves x.grad None in the reference; zeros are stored.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_heads.py <path of the reference checkout>
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "heads")
sys.dont_write_bytecode = True

FAMILIES = {            # family -> (reference layer class, reference factory, extra constructor arguments of the fixtures)
    "cheby": ("ChebyKANLayer", "mlp_chebykan", {}),
    "bessel": ("BesselKANLayer", "mlp_besselkan", {}),
    "fibonacci": ("FibonacciKANLayer", "mlp_fibonaccikan", {}),
    "gegenbauer": ("GegenbauerKANLayer", "mlp_gegenbauerkan", {"alpha_param": 0.7}),     # the default 0 zeroes every plane above the first
    "hermite": ("HermiteKANLayer", "mlp_hermitekan", {}),
    "laguerre": ("LaguerreKANLayer", "mlp_laguerrekan", {"alpha": 0.5}),
    "lucas": ("LucasKANLayer", "mlp_lucaskan", {}),
}
SHAPES = [                                  # (case, B, I, O, degree)
    ("deg3", 5, 7, 3, 3),
    ("deg1", 5, 7, 3, 1),
    ("o130", 4, 9, 130, 2),                 # crosses the 128-output tile
    ("deg12", 3, 5, 9, 12),                 # 13 planes: recurrence coefficients as a device table
    ("i300", 2, 300, 5, 3),                 # depth 1200
]
DEG15 = ("deg15", 3, 5, 4, 15)              # 16 planes, the launch maximum: ChebyKAN and LucasKAN only
SEED0 = 9100


def cases():
    out = []
    for fam, (_, _, extra) in FAMILIES.items():
        out += [(fam, *s, extra) for s in SHAPES]
        if fam in ("cheby", "lucas"):
            out.append((fam, *DEG15, extra))
    out.append(("gegenbauer", "alpha0", 5, 7, 3, 3, {"alpha_param": 0.0}))               # the models' default, reproduced as it is
    return out


def run(build, x, g):
    """fp32 and fp64 forward + backward of the module `build()` returns (same parameter values in both)."""
    torch.set_default_dtype(torch.float32)
    m32 = build()
    sd = {k: v.clone() for k, v in m32.state_dict().items()}
    res = {}
    for tag, dt, m in (("", torch.float32, m32), ("64", torch.float64, None)):
        torch.set_default_dtype(dt)
        if m is None:
            m = build()
            m.load_state_dict({k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()})
        xi = x.to(dt).clone().requires_grad_(True)
        y = m(xi)
        y.backward(g.to(dt))
        res["y" + tag] = y.detach()
        res["dx" + tag] = xi.grad if xi.grad is not None else torch.zeros_like(xi)
        for n, p in m.named_parameters():
            res[f"grad{tag}.{n}"] = p.grad
    torch.set_default_dtype(torch.float32)
    return sd, res


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def save(name, cfg, x, g, sd, res):
    arrays = {"cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8), "x": x.numpy(), "g": g.numpy()}
    arrays.update({"sd." + k: v.numpy() for k, v in sd.items()})
    arrays.update({k: v.numpy() for k, v in res.items()})
    path = os.path.join(OUT, name + ".npz")
    np.savez(path, **arrays)
    dist = {k: rel(res[k], res[k.replace("grad.", "grad64.") if k.startswith("grad.") else k + "64"])
            for k in res if not (k.endswith("64") or k.startswith("grad64."))}
    size = os.path.getsize(path)
    print(f"{name:22s} {size / 1024:6.1f} KiB  fp32 vs fp64: " + " ".join(f"{k}={v:.1e}" for k, v in dist.items()))
    assert size <= 128 * 1024, (name, size)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import layers as REF_LAYERS                  # the reference package
    # models/kans.py alone: the reference's `models` package imports torchvision-based networks that these fixtures do not need
    spec = importlib.util.spec_from_file_location("ref_kans", os.path.join(sys.path[0], "models", "kans.py"))
    REF_KANS = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(REF_KANS)
    os.makedirs(OUT, exist_ok=True)
    for i, (fam, case, B, I, O, degree, extra) in enumerate(cases()):
        torch.manual_seed(SEED0 + i)
        x, g = torch.randn(B, I), torch.randn(B, O)
        cls = getattr(REF_LAYERS, FAMILIES[fam][0])

        def build():
            torch.manual_seed(SEED0 + 1000 + i)
            return cls(I, O, degree, **extra)
        sd, res = run(build, x, g)
        save(f"{fam}_{case}", dict(kind="layer", family=fam, B=B, I=I, O=O, degree=degree, extra=extra), x, g, sd, res)
    # one two-layer model with l1_decay: the L1 wrapper's `module.` key prefix and its penalty in the gradients
    fam, hidden, l1 = "lucas", [6, 5, 3], 0.01
    torch.manual_seed(SEED0 + 500)
    x, g = torch.randn(4, hidden[0]), torch.randn(4, hidden[-1])

    def build_model():
        torch.manual_seed(SEED0 + 1500)
        return getattr(REF_KANS, FAMILIES[fam][1])(hidden, l1_decay=l1)
    sd, res = run(build_model, x, g)
    save(f"{fam}_mlp_l1", dict(kind="model", family=fam, B=4, layers_hidden=hidden, l1_decay=l1, degree=3, extra={}), x, g, sd, res)


if __name__ == "__main__":
    main()

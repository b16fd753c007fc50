#!/usr/bin/env python3
"""Golden vectors for layers ABOVE the one-launch plane limit (any degree / grid size), from the REFERENCE itself.

The case runner is make_golden.py's own (`run_case`: reference layer, forward + backward, the reference's fp32-vs-fp64 `noise`
record, and the oracle pinned against the reference -- it aborts on any mismatch); only the cases and the output folder differ.
The fixtures go to tests/golden/windows/, so the enumerations of tests/golden/*.npz (conftest.golden_cases, make_plan_snapshot.py)
see nothing new.  Needs the reference checkout, like make_golden.py.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_windows.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as MG  # noqa: E402

OUT = os.path.join(HERE, "windows")
C = MG.C
SEED0 = 7500                      # own seed range, as every fixture family of make_golden.py

# stated tolerances of the GPU comparison (tests/helpers.py TOL_Y / TOL_DX / TOL_DW, 2e-5 for non-conv parameters)
TOL = {"y": 1e-5, "dx": 1e-5, "conv": 5e-5, "other": 2e-5}

CASES = [
    # FourierKAN (`degree` carries grid_size): 2 * grid_size + 1 planes; a window is a range of frequencies
    C("fourier", "grid8", 2, 3, 4, 8, 8, degree=8),                                   # 17 planes: the smallest above the limit
    C("fourier", "grid20_s2g2", 2, 4, 6, 8, 7, s=2, groups=2, degree=20, act="silu"),  # 41 planes, three windows
    C("fourier", "1d_grid9", 2, 3, 4, 1, 8, ndim=1, degree=9),
    # recurrence families: degree + 1 planes (+ base); above 11 planes the coefficients travel as a device table
    C("lucas", "deg11", 2, 3, 4, 8, 8, degree=11),                                    # 12 planes + base in ONE launch, device table, no window
    C("lucas", "deg16", 2, 4, 5, 7, 6, degree=16, act="silu"),
    C("taylor", "deg18", 2, 3, 4, 8, 8, degree=18),                                   # plane count = degree, not degree + 1
    C("gegenbauer", "deg20_d2", 2, 3, 4, 8, 8, d=2, p=2, degree=20, extra={"alpha_param": 0.7}),
    C("cheby", "deg17", 2, 3, 4, 8, 8, degree=17),
    # plane-major poly_weights (identity base branch)
    C("jacobi", "deg12", 2, 3, 4, 8, 8, degree=12, extra={"a": 1.0, "b": 0.5}),
    C("legendre", "deg32", 2, 3, 4, 6, 5, degree=32),                                 # three windows, x_n as the second input of each
    C("bersnstein", "deg12", 2, 3, 4, 8, 8, degree=12),
    # host-only windows: slices of the centres / of the per-channel phases
    C("rbf", "grid20", 2, 3, 4, 8, 8, grid_size=20),
    C("relu", "g12k4", 2, 3, 4, 8, 8, extra={"g": 12, "k": 4}),                       # phases perturbed per channel by run_case, as every ReLU fixture
    # Bessel and Hermite planes grow factorially with the degree: degree 12 on a small input scale (|tanh x| stays well below 1), at which
    # the reference's own fp32-vs-fp64 noise is below the stated tolerances (checked below)
    C("bessel", "deg12", 2, 3, 4, 8, 8, degree=12, xs=0.1),
    C("hermite", "deg12", 2, 3, 4, 8, 8, degree=12, xs=0.1),
]
NOISE_CHECKED = ("bessel_deg12", "hermite_deg12")


def main():
    os.makedirs(OUT, exist_ok=True)
    MG.HERE = OUT                                      # run_case writes <kind>_<name>.npz next to its module's HERE
    for i, c in enumerate(CASES):
        worst, sz = MG.run_case(SEED0 + i, c)
        name = f"{c['kind']}_{c['name']}"
        noise = json.loads(bytes(np.load(os.path.join(OUT, name + ".npz"))["noise"]).decode())
        print(f"{name:24s} oracle-vs-ref max rel err {worst:.2e}  {sz / 1024:.0f} KiB  reference fp32 noise: "
              + " ".join(f"{k}={v:.1e}" for k, v in noise.items()))
        assert 1 < sz < 64 * 1024, (name, sz)
        if name in NOISE_CHECKED:
            for k, v in noise.items():
                bound = TOL[k] if k in TOL else TOL["conv"] if ("conv" in k or "poly_weights" in k) else TOL["other"]
                assert v < bound, f"{name}: the reference's own noise on {k} is {v:.2e} >= {bound:.0e}: lower the degree or the input scale"


if __name__ == "__main__":
    main()

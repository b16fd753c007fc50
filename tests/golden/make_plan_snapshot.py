"""Generate plan_snapshot.json: every KanPlan field and kan_pack_cacheable for ~1.3k (geometry, basis) cases, recorded from the library
as built.  tests/test_plan_snapshot.py asserts the library reproduces it, so a change to the planner that moves any split count, tile
choice or route shows up as a diff here.  Rejected geometries record kan_plan's return code and message.

    python tests/golden/make_plan_snapshot.py          # rewrites tests/golden/plan_snapshot.json (CPU only)
"""
import ctypes as C
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "plan_snapshot.json")

GEOM_FIELDS = ("B", "C", "H", "W", "O", "Ho", "Wo", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw", "groups", "x_bstride", "y_bstride")


def plan_fields():
    from convkan_amd import _lib as L
    return [n for n, _ in L.KanPlan._fields_]


def basis_key(spec):
    return [spec.kind, spec.n_basis, spec.order, spec.act, spec.p0, spec.p1, [float(v) for v in spec.table]]


def make_structs(gl, bl):
    from convkan_amd import _lib as L
    g, b = L.KanGeom(), L.KanBasis()
    for n, v in zip(GEOM_FIELDS, gl):
        setattr(g, n, v)
    b.kind, b.n_basis, b.order, b.act, b.p0, b.p1 = bl[:6]
    for i, v in enumerate(bl[6]):
        b.table[i] = v
    return g, b


def run_case(lib, gl, bl):
    """[rc, message] for a rejected geometry, else [plan values in KanPlan field order, kan_pack_cacheable]."""
    from convkan_amd import _lib as L
    g, b = make_structs(gl, bl)
    p = L.KanPlan()
    rc = lib.kan_plan(C.byref(g), C.byref(b), C.byref(p))
    if rc != 0:
        return {"rc": rc, "msg": lib.kan_last_error().decode()}
    return {"plan": [getattr(p, n) for n in plan_fields()], "cacheable": lib.kan_pack_cacheable(C.byref(g), C.byref(b))}


def geom(B, C_, H, W, O, k=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1), G=1, x_bstride=None):
    Ho = (H + 2 * p[0] - d[0] * (k[0] - 1) - 1) // s[0] + 1
    Wo = (W + 2 * p[1] - d[1] * (k[1] - 1) - 1) // s[1] + 1
    xb = G * C_ * H * W if x_bstride is None else x_bstride
    return [B, C_, H, W, O, Ho, Wo, k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1], G, xb, G * O * max(Ho, 0) * max(Wo, 0)]


def basis_specs():
    """Name -> basis of every family and every compile-time spec (fast variant), taken from the layers themselves."""
    import torch.nn as nn
    import convkan_amd as K
    mk = lambda cls, **kw: basis_key(cls(4, 4, 3, **kw).conv_spec())
    out = {
        "kan_silu": mk(K.KANConv2DLayer, base_activation=nn.SiLU),                         # fast 1
        "kan_gelu": mk(K.KANConv2DLayer, base_activation=nn.GELU),                         # fast 2
        "kan_g3o2": mk(K.KANConv2DLayer, grid_size=3, spline_order=2, base_activation=nn.SiLU),
        "kan_g8o1": mk(K.KANConv2DLayer, grid_size=8, spline_order=1, base_activation=nn.GELU),
        "fast_g8": mk(K.FastKANConv2DLayer, grid_size=8, base_activation=nn.SiLU),         # fast 3
        "fast_g5": mk(K.FastKANConv2DLayer, grid_size=5, base_activation=nn.SiLU),         # fast 8
        "fast_g4_gelu": mk(K.FastKANConv2DLayer, grid_size=4, base_activation=nn.GELU),
        "cheby_d4": mk(K.ChebyKANConv2DLayer, degree=4),                                   # fast 4
        "cheby_d3": mk(K.ChebyKANConv2DLayer, degree=3),                                   # fast 5
        "cheby_d6": mk(K.ChebyKANConv2DLayer, degree=6),
        "lucas_d3": mk(K.LucasKANConv2DLayer, degree=3),                                   # fast 6
        "hermite_d2": mk(K.HermiteKANConv2DLayer, degree=2),                               # fast 7
        "taylor_d1": mk(K.TaylorKANConv2DLayer, degree=1),                                 # fast 11 (one plane)
        "gegen_d5": mk(K.GegenbauerKANConv2DLayer, degree=5, alpha_param=1.0),
        "legendre_d3": mk(K.LegendreKANConv2DLayer, degree=3),                             # order 0: second input tensor
        "legendre_d2": mk(K.LegendreKANConv2DLayer, degree=2),
        "fourier_g3": mk(K.FourierKANConv2DLayer, grid_size=3),
        "fourier_g5": mk(K.FourierKANConv2DLayer, grid_size=5),
        "relu_g5k3": mk(K.ReLUKANConv2DLayer, g=5, k=3),                                   # fast 9
        "relu_g3k2": mk(K.ReLUKANConv2DLayer, g=3, k=2),
        "gram_d3": mk(K.GRAMKANConv2DLayer, degree=3),                                     # fast 10
        "gram_d5": mk(K.GRAMKANConv2DLayer, degree=5),
    }
    for mode in (1, 2):                                     # ReLU-KAN value / phase-derivative planes, GRAM-KAN modes
        out[f"relu_g5k3_m{mode}"] = out["relu_g5k3"][:2] + [mode] + out["relu_g5k3"][3:]
    for mode in (1, 2):
        out[f"gram_d3_m{mode}"] = out["gram_d3"][:2] + [mode] + out["gram_d3"][3:]
    return out


def layer_specs(layer):
    """The launch specs of a layer: one, or one per plane window of a B-spline layer of more than KAN_MAX_PLANES planes."""
    from convkan_amd import _lib as L
    s = layer.conv_spec()
    if s.n_basis + (s.act != L.ACT_NONE) > L.KAN_MAX_PLANES and hasattr(layer, "_plane_windows"):
        return [w[0] for w in layer._plane_windows()]
    return [s]


def model_layers():
    """(basis, C, O, H, W, kernel, stride, padding) of every conv layer of KAN-VGG11 / FastKAN-VGG11 (3x32x32) and ChebyKAN-AlexNet
    (3x224x224), walked in forward order with MaxPool2d shrinking the plane."""
    import torch.nn as nn
    from convkan_amd.models.kan_vgg import vggkan
    from convkan_amd.models.kan_alexnet import alexnet_kan
    out = []
    for model, hw in ((vggkan(3, 10, kan_conv="KAN", arch="VGG11"), 32), (vggkan(3, 10, kan_conv="FastKAN", arch="VGG11"), 32),
                      (alexnet_kan(10, kan_conv="ChebyKAN"), 224)):
        H = W = hw
        for m in model.modules():
            if hasattr(m, "conv_spec"):
                for s in layer_specs(m):
                    out.append((basis_key(s), m.input_dim // m.groups, m.output_dim // m.groups, H, W, s.kernel, s.stride, s.padding, s.groups))
                H, W = s.out_hw(H, W)
            elif isinstance(m, nn.MaxPool2d):
                k = m.kernel_size if isinstance(m.kernel_size, int) else m.kernel_size[0]
                st = m.stride if isinstance(m.stride, int) else m.stride[0]
                H, W = (H - k) // st + 1, (W - k) // st + 1
    return out


def golden_cfg_cases():
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import build_layer
    out = []
    for fn in sorted(os.listdir(HERE)):
        if not fn.endswith(".npz") or fn.startswith(("model_", "basis_", "mlp_", "wav_")):
            continue
        c = json.loads(bytes(np.load(os.path.join(HERE, fn))["cfg"]).decode())
        if c.get("ndim", 2) == 3:
            continue                                        # 3-D layers run as stacks of 2-D launches of other planes: not a 2-D cfg
        layer = build_layer(c)
        H, W = (1, c["W"]) if c.get("ndim", 2) == 1 else (c["H"], c["W"])
        for s in layer_specs(layer):
            out.append((fn[:-4], basis_key(s), c["C"] // c["groups"], c["O"] // c["groups"], H, W, s.kernel, s.stride, s.padding, s.dilation, s.groups))
    return out


def generate():
    import convkan_amd
    lib = convkan_amd._lib.load()
    specs = basis_specs()
    bases, cases = [], []
    index = {}

    def add(tag, gl, bl):
        key = json.dumps(bl)
        if key not in index:
            index[key] = len(bases)
            bases.append(bl)
        cases.append({"tag": tag, "g": gl, "b": index[key], **run_case(lib, gl, bl)})

    for i, (bl, C_, O, H, W, k, s, p, G) in enumerate(model_layers()):
        for B in (2, 128, 256):
            add(f"model{i}", geom(B, C_, H, W, O, k, s, p, G=G), bl)
    for name, bl, C_, O, H, W, k, s, p, d, G in golden_cfg_cases():
        add(f"golden:{name}", geom(2, C_, H, W, O, k, s, p, d, G=G), bl)

    rng = random.Random(20261015)
    names = sorted(specs)
    KS = [(1, 1), (3, 3), (5, 5), (11, 11), (3, 3), (3, 3)]
    PLANES = [2, 3, 4, 5, 7, 8, 13, 16, 27, 32]
    for i in range(1100):
        name = names[i % len(names)]
        bl = specs[name]
        shape = rng.random()
        if shape < 0.45:                                    # the halo / pmdma / band neighbourhood: 3x3 stride-1 pad-1 square planes
            H = W = rng.choice([2, 4, 8, 16, 32])
            k, s, p, d = (3, 3), (1, 1), (1, 1), (1, 1)
        else:
            H = rng.choice(PLANES); W = H if rng.random() < 0.7 else rng.choice(PLANES)
            k = rng.choice(KS); s = (rng.randint(1, 4),) * 2; p = (rng.randint(0, 2),) * 2; d = (2, 2) if rng.random() < 0.15 else (1, 1)
        if rng.random() < 0.08:                             # 1-D layers: H = 1
            H, k, s, p, d = 1, (1, k[1]), (1, s[1]), (0, p[1]), (1, d[1])
        C_ = rng.choice([1, 2, 3, 16, 64, 256, 512])
        O = rng.choice([16, 64, 96, 128, 192, 256, 512])
        B = rng.choice([1, 8, 16, 128, 256])
        G = 1
        r = rng.random()
        if r < 0.08:                                        # depthwise: one channel, one or two outputs per group
            C_, O, G = 1, rng.choice([1, 2]), rng.choice([16, 64, 256])
        elif r < 0.14:
            G = rng.choice([2, 4])
        add(f"grid:{name}", geom(B, C_, H, W, O, k, s, p, d, G), bl)

    # rejections: the messages tests and callers match on
    knots = specs["kan_silu"]
    bent = knots[:6] + [[v + (0.3 if j == 5 else 0.0) for j, v in enumerate(knots[6])]]
    add("reject:uniform", geom(2, 3, 8, 8, 4), bent)
    add("reject:planes", geom(2, 3, 8, 8, 4), [0, 16, 3, 2, 0.0, 0.0, [(-3 + 6 * j / 19) for j in range(20)]])
    add("reject:bstride", geom(8, 16, 14, 14, 24, G=4, x_bstride=16 * 14 * 14), specs["kan_silu"])
    add("reject:empty", geom(2, 3, 2, 2, 4, k=(5, 5), p=(0, 0)), specs["kan_silu"])
    add("reject:gram_mode", geom(2, 3, 8, 8, 4), specs["gram_d3"][:2] + [3] + specs["gram_d3"][3:])
    return {"geom_fields": list(GEOM_FIELDS), "plan_fields": plan_fields(), "bases": bases, "cases": cases}


def coverage(snap):
    f = {n: i for i, n in enumerate(snap["plan_fields"])}
    flags = ("fwd_halo", "fwd_band", "bwd_weight_halo", "bwd_weight_band", "fwd_expanded", "bwd_weight_expanded", "x_pm_wanted", "dz_pm_wanted")
    n = {k: 0 for k in flags + ("row_blocks&1", "row_blocks&2", "dw", "rejected", "cacheable")}
    for c in snap["cases"]:
        if "plan" not in c:
            n["rejected"] += 1
            continue
        pl = c["plan"]
        for k in flags:
            n[k] += pl[f[k]] != 0
        n["row_blocks&1"] += (pl[f["row_blocks"]] & 1) != 0
        n["row_blocks&2"] += (pl[f["row_blocks"]] & 2) != 0
        n["dw"] += c["g"][1] == 1 and c["g"][4] <= 2
        n["cacheable"] += c["cacheable"]
    return n


if __name__ == "__main__":
    snap = generate()
    with open(OUT, "w") as fh:
        json.dump(snap, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{len(snap['cases'])} cases, {len(snap['bases'])} bases, {os.path.getsize(OUT) // 1024} KB -> {OUT}")
    print(coverage(snap))

"""Recipes shared by the ILRA fixture generator (make_golden_ilra.py) and the tests that replay them.

A bag and a parameter set are (seed, recipe) pairs replayed with numpy's legacy ``RandomState``; the fixtures hold the reference's
OUTPUTS only, never parameters.  The full gradients of a case are 12.6 MB, so a fixture keeps a DIGEST per tensor: its float64 largest
entry, ``g v`` and ``u^T g`` for seeded Gaussian u, v (the tensor as a matrix of rows of its last dimension) and 256 seeded entries.

Parameter recipe "live": the reference's initial distributions (xavier-normal ``Linear`` weights, ``nn.MultiheadAttention``'s
xavier-uniform ``in_proj_weight``, xavier-uniform latents), every weight matrix except ``classifier`` times 2, latents and ``S`` times
2, every bias from U(-0.05, 0.05); rows are ``dsmil_cases.make_rows`` times 4 (exact in bf16).  With the default initialisation every
attention of the model is uniform to 1e-4 and two different bags give the same logits to 1e-4: a parity test on it cannot see a kernel
that reads the wrong rows.  The "default" recipe is kept for the state-dict / initialisation check only."""
import numpy as np

from dsmil_cases import make_rows

GAIN = 2.0
ROW_GAIN = 4.0
BAND = 1e-06           # mask band: written by make_golden_ilra.py (10 x the largest |t64| at which the reference's fp32 run flips a ReLU, floor 1e-6)

# name -> (N, rows, num_layers, num_cls, seed, recipe)
CASES = {
    "n1":      (1,    "bf16", 2, 4, 101, "live"),
    "n17":     (17,   "bf16", 2, 4, 102, "live"),
    "n64":     (64,   "bf16", 2, 4, 103, "live"),
    "n65":     (65,   "bf16", 2, 4, 104, "live"),
    "n130":    (130,  "bf16", 2, 4, 105, "live"),
    "n257":    (257,  "bf16", 2, 4, 106, "live"),
    "n2798":   (2798, "bf16", 2, 4, 107, "live"),
    "f32_600": (600,  "f32",  2, 4, 108, "live"),
    "l1_c1":   (130,  "bf16", 1, 1, 109, "live"),
    "l3":      (130,  "bf16", 3, 4, 110, "live"),
    "default_n130": (130, "bf16", 2, 4, 111, "default"),
}
PARITY = tuple(k for k, v in CASES.items() if v[5] == "live")


def _mha_shapes(prefix, dim_q, dim_k, gated):
    s = {prefix + "multihead_attn.in_proj_weight": (768, 256), prefix + "multihead_attn.in_proj_bias": (768,),
         prefix + "multihead_attn.out_proj.weight": (256, 256), prefix + "multihead_attn.out_proj.bias": (256,),
         prefix + "fc_q.weight": (256, dim_q), prefix + "fc_q.bias": (256,), prefix + "fc_k.weight": (256, dim_k), prefix + "fc_k.bias": (256,),
         prefix + "fc_v.weight": (256, dim_k), prefix + "fc_v.bias": (256,), prefix + "fc_o.weight": (256, 256), prefix + "fc_o.bias": (256,)}
    if gated:
        s[prefix + "gate.0.weight"] = (256, dim_q)
        s[prefix + "gate.0.bias"] = (256,)
    return s


def shapes(num_layers, num_cls):
    """state-dict keys -> shapes in the reference's order (dim_in = 512, dim_hid = 256, topk = 1)"""
    s = {}
    for i in range(num_layers):
        d = 512 if i == 0 else 256
        s[f"gab_blocks.{i}.latent"] = (1, 1, 256)
        s.update(_mha_shapes(f"gab_blocks.{i}.project_forward.", 256, d, True))
        s.update(_mha_shapes(f"gab_blocks.{i}.project_backward.", d, 256, True))
    s["pooling.S"] = (1, 1, 256)
    s.update(_mha_shapes("pooling.mha.", 256, 256, False))
    s["classifier.weight"] = (num_cls, 256)
    s["classifier.bias"] = (num_cls,)
    return s


def make_params(num_layers, num_cls, seed, recipe="live"):
    rs = np.random.RandomState(seed + 1000)
    live = recipe == "live"
    out = {}
    for k, sh in shapes(num_layers, num_cls).items():
        if k.endswith("latent") or k.endswith(".S"):
            b = np.sqrt(6.0 / 512.0)
            v = rs.uniform(-b, b, size=sh) * (GAIN if live else 1.0)
        elif k.endswith("in_proj_weight"):
            b = np.sqrt(6.0 / (768 + 256))
            v = rs.uniform(-b, b, size=sh) * (GAIN if live else 1.0)
        elif k.endswith("weight"):
            v = rs.standard_normal(sh) * np.sqrt(2.0 / (sh[0] + sh[1])) * (GAIN if live and not k.startswith("classifier") else 1.0)
        elif live:
            v = rs.uniform(-0.05, 0.05, size=sh)
        elif k.endswith("in_proj_bias") or k.endswith("out_proj.bias"):
            v = np.zeros(sh)
        else:
            fan_in = 512 if (k.startswith("gab_blocks.0.project_backward") and (".fc_q." in k or ".gate." in k)) or \
                (k.startswith("gab_blocks.0.project_forward") and (".fc_k." in k or ".fc_v." in k)) else 256
            b = 1.0 / np.sqrt(fan_in)
            v = rs.uniform(-b, b, size=sh)
        out[k] = v.astype(np.float32)
    return out


def make_bag(N, rows, seed):
    return make_rows(N, rows, seed) * np.float32(ROW_GAIN)


def make_w(num_cls, seed):
    return np.random.RandomState(seed + 2000).standard_normal((1, num_cls)).astype(np.float32)


def make_case(name):
    N, rows, num_layers, num_cls, seed, recipe = CASES[name]
    return make_bag(N, rows, seed), make_params(num_layers, num_cls, seed, recipe), make_w(num_cls, seed)


def digest(key, g, seed):
    """(gmax, g v, u^T g, 256 seeded entries) of a float64 gradient; u, v and the entries depend on the key's shape and the seed"""
    g = np.asarray(g, dtype=np.float64)
    g2 = g.reshape(-1, g.shape[-1])
    rs = np.random.RandomState(seed + 3000 + g2.shape[0] * 7 + g2.shape[1])
    u, v = rs.standard_normal(g2.shape[0]), rs.standard_normal(g2.shape[1])
    idx = rs.randint(0, g2.size, size=256)
    return {"gmax": np.float64(np.abs(g).max()), "gv": g2 @ v, "ug": u @ g2, "pick": g2.reshape(-1)[idx]}

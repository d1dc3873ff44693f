"""Recipes shared by the DeepAttnMISL fixture generator (make_golden_deepattnmisl.py) and the tests that replay them.

A bag, its cluster ids and a parameter set are (seed, recipe) pairs replayed with numpy's legacy ``RandomState``; the fixtures hold the
reference's OUTPUTS only.  The float64 gradient of ``phis.0.weight`` (512 KB as float32) lives whole in a file of its own per case
(``deepattnmisl_<case>_gp.npz``, rounded to float32; its float64 maximum is in the main file); the three [256, 256] gradients are
rounded to float32 as well (6e-8 of an entry), so that the main file stays under 1 MiB; every other tensor is stored in float64."""
import numpy as np

from dsmil_cases import make_rows

BIG = {"phis.0.weight": "gp"}                      # gradient tensors kept in files of their own
ROUNDED = ("phis.0.weight", "attention_net.0.weight", "attention_net.3.fc1.0.weight", "attention_net.3.score.0.weight")     # stored as float32
KEYS = ("phis.0.weight", "phis.0.bias", "attention_net.0.weight", "attention_net.0.bias", "attention_net.3.fc1.0.weight",
        "attention_net.3.fc1.0.bias", "attention_net.3.score.0.weight", "attention_net.3.score.0.bias", "attention_net.3.fc2.weight",
        "attention_net.3.fc2.bias", "output_layer.weight", "output_layer.bias")
NEAR_ZERO = 1e-5       # the fixtures list every entry of pre with |pre| below this
BAND = 1e-6            # the kernel's ReLU mask must equal pre64 > 0 wherever |pre64| >= BAND

# name -> (N, Kc, num_cls, rows, seed);  rows: "f32" = unit-norm fp32 rows, "bf16" = the same rounded to bf16
CASES = {
    "n8":      (8,    8,  1, "bf16", 31),
    "n17":     (17,   8,  1, "bf16", 32),
    "n130":    (130,  8,  4, "bf16", 33),
    "f32_600": (600,  8,  1, "f32",  34),
    "n2798":   (2798, 8,  4, "bf16", 35),
    "n257_k16": (257, 16, 4, "bf16", 36),
}


def make_ids(N, Kc, seed):
    """[N] int64 cluster ids, every cluster populated (the reference's conv2d fails on an empty one)"""
    ids = np.random.RandomState(seed + 3000).randint(0, Kc, size=N)
    ids[:Kc] = np.arange(Kc)
    return ids.astype(np.int64)


def shapes(Kc, num_cls):
    return {KEYS[0]: (256, 512, 1, 1), KEYS[1]: (256,), KEYS[2]: (256, 256), KEYS[3]: (256,), KEYS[4]: (256, 256), KEYS[5]: (256,),
            KEYS[6]: (256, 256), KEYS[7]: (256,), KEYS[8]: (1, 256), KEYS[9]: (1,), KEYS[10]: (num_cls, 256), KEYS[11]: (num_cls,)}


def make_params(Kc, num_cls, seed):
    """the twelve DeepAttnMISL parameters (float32) drawn as torch's default initialisation draws them: U(-1/sqrt(fan_in), 1/sqrt(fan_in))"""
    rs = np.random.RandomState(seed + 1000)
    out = {}
    for k, sh in shapes(Kc, num_cls).items():
        fan_in = 512 if k.startswith("phis") else 256
        b = 1.0 / np.sqrt(fan_in)
        out[k] = rs.uniform(-b, b, size=sh).astype(np.float32)
    return out


def make_w(num_cls, seed):
    """the weights w of the scalar sum(logits * w) whose gradients the fixtures hold"""
    return np.random.RandomState(seed + 2000).standard_normal((1, num_cls)).astype(np.float32)


def make_case(name):
    N, Kc, num_cls, rows, seed = CASES[name]
    return make_rows(N, rows, seed), make_ids(N, Kc, seed), make_params(Kc, num_cls, seed), make_w(num_cls, seed)

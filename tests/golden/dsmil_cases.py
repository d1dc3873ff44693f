"""Recipes shared by the DSMIL fixture generator (make_golden_dsmil.py) and the tests that replay them.

A bag, and a parameter set, is a (seed, recipe) pair replayed with numpy's legacy ``RandomState`` (bit-stable across numpy versions):
[N, 512] rows and the two [256, 512] matrices are 0.5 - 100 MB each, far over what a committed fixture may weigh, so the fixtures hold
the reference's OUTPUTS only.  The float64 gradients of ``b_classifier.q.weight`` / ``v.1.weight`` (512 KB each as float32) live whole in
files of their own per case (``dsmil_<case>_gq.npz`` / ``_gv.npz``, rounded to float32: 6e-8 of an entry, their float64 maxima are in the
main file); every other tensor is stored in ``dsmil_<case>.npz``."""
import numpy as np

BIG = {"b_classifier.q.weight": "gq", "b_classifier.v.1.weight": "gv"}      # gradient tensors kept in files of their own
KEYS = ("i_classifier.fc.0.weight", "i_classifier.fc.0.bias", "b_classifier.q.weight", "b_classifier.q.bias",
        "b_classifier.v.1.weight", "b_classifier.v.1.bias", "b_classifier.fcc.weight", "b_classifier.fcc.bias")
FP_KEYS = ("feat_proj.projecter.0.weight", "feat_proj.projecter.0.bias", "feat_proj.projecter.1.weight", "feat_proj.projecter.1.bias")

# name -> (N, C, rows, seed, sharp, feat_proj);  rows: "f32" = unit-norm fp32 rows, "bf16" = the same rounded to bf16
CASES = {
    "n1":        (1,     4,  "bf16", 11, False, False),
    "n17":       (17,    4,  "bf16", 12, False, False),
    "f32_2798":  (2798,  4,  "f32",  13, False, False),
    "b_2798_c4": (2798,  4,  "bf16", 14, False, False),
    "b_2798_c12": (2798, 12, "bf16", 15, False, False),
    "b_2798_c6": (2798,  6,  "bf16", 21, False, False),
    "b_10k_c4":  (10000, 4,  "bf16", 16, False, False),
    "b_10k_c12": (10000, 12, "bf16", 27, False, False),
    "b_50k_c4":  (50000, 4,  "bf16", 18, False, False),
    "sharp":     (2798,  4,  "bf16", 19, True,  False),
    "featproj":  (2798,  4,  "bf16", 20, False, True),
}


def _bf16_round(a):
    import torch
    return torch.from_numpy(a).bfloat16().float().numpy()


def make_rows(N, rows, seed):
    """[N, 512] float32 unit-norm rows around a few cluster directions (bf16-rounded for rows == "bf16")"""
    rs = np.random.RandomState(seed)
    centers = rs.standard_normal((8, 512)).astype(np.float32)
    x = centers[rs.randint(0, 8, size=N)] * 0.5 + rs.standard_normal((N, 512)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return _bf16_round(x) if rows == "bf16" else x.astype(np.float32)


def make_params(C, seed, feat_proj=False, q_scale=1.0):
    """the eight DSMIL parameters (float32) drawn as torch's default initialisation draws them: U(-1/sqrt(fan_in), 1/sqrt(fan_in));
    biases likewise.  q_scale multiplies b_classifier.q.weight (the "sharp" case)."""
    rs = np.random.RandomState(seed + 1000)

    def u(shape, fan_in):
        b = 1.0 / np.sqrt(fan_in)
        return rs.uniform(-b, b, size=shape).astype(np.float32)
    p = {KEYS[0]: u((C, 512), 512), KEYS[1]: u((C,), 512), KEYS[2]: u((256, 512), 512) * np.float32(q_scale), KEYS[3]: u((256,), 512),
         KEYS[4]: u((256, 512), 512), KEYS[5]: u((256,), 512), KEYS[6]: u((C, C, 256), C * 256), KEYS[7]: u((C,), C * 256)}
    if feat_proj:
        p[FP_KEYS[0]] = u((512, 512), 512)
        p[FP_KEYS[1]] = u((512,), 512)
        p[FP_KEYS[2]] = (1.0 + 0.1 * rs.standard_normal(512)).astype(np.float32)
        p[FP_KEYS[3]] = (0.1 * rs.standard_normal(512)).astype(np.float32)
    return p


def make_w(C, seed):
    """the weights w of the scalar sum(logits * w) whose gradients the fixtures hold"""
    return np.random.RandomState(seed + 2000).standard_normal((1, C)).astype(np.float32)

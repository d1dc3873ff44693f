"""Generate tests/golden/deepattnmisl_<case>.npz (and deepattnmisl_<case>_gp.npz: the [256, 512, 1, 1] gradient, whole) from the upstream
reference's own DeepAttnMISL (model/deepmil.py:542-580) in float64.

Container-only (imports the reference through _ref_import.py).  Per case: logits, h_cluster and the gradients of all twelve tensors for
sum(logits * w), all from the ``.double()`` model on the ``.double()`` input in eval mode; the entries of pre = Wp x + bp with |pre| <
1e-5 as (row, unit, value) triples; the number of ReLU decisions on which the reference's own fp32 run differs from its float64 run; and
the state-dict keys and shapes.  Inputs, ids and parameters are recipes (deepattnmisl_cases.py)."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import deepattnmisl_cases as AC  # noqa: E402
from _ref_import import import_reference  # noqa: E402


def build(ref, Kc, num_cls, params, dtype):
    with contextlib.redirect_stdout(io.StringIO()):
        m = ref.deepmil.DeepAttnMISL(dim_in=512, dim_hid=256, num_cls=num_cls, num_clusters=Kc, dropout=0.25)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m.to(dtype).eval()


def run(m, x, ids, w, dtype):
    X = torch.from_numpy(x).to(dtype)[None]
    m.zero_grad(set_to_none=True)
    kept = {}
    hook = m.attention_net.register_forward_pre_hook(lambda mod, args: kept.__setitem__("hc", args[0].detach()))
    logits = m(X, torch.from_numpy(ids).float())
    hook.remove()
    (logits * torch.from_numpy(w).to(dtype)).sum().backward()
    grads = {k: p.grad.detach().double().numpy() for k, p in m.named_parameters()}
    with torch.no_grad():
        pre = X[0] @ m.phis[0].weight.view(256, 512).t() + m.phis[0].bias
    return logits.detach().double().numpy(), kept["hc"].double().numpy(), pre.numpy(), grads


def main():
    ref = import_reference()
    for name, (N, Kc, num_cls, rows, seed) in AC.CASES.items():
        x, ids, params, w = AC.make_case(name)
        m64 = build(ref, Kc, num_cls, params, torch.float64)
        assert tuple(m64.state_dict()) == AC.KEYS
        logits, hc, pre, grads = run(m64, x, ids, w, torch.float64)
        l32, h32, pre32, g32 = run(build(ref, Kc, num_cls, params, torch.float32), x, ids, w, torch.float32)
        r, u = np.nonzero(np.abs(pre) < AC.NEAR_ZERO)
        out = {"logits": logits, "hc": hc, "keys": np.array(AC.KEYS), "near_row": r.astype(np.int32), "near_unit": u.astype(np.int32),
               "near_value": pre[r, u], "ref32_mask_flips": np.int64(((pre32 > 0) != (pre > 0)).sum()),
               "near_counts": np.array([(np.abs(pre) < t).sum() for t in (1e-5, 1e-6, 1e-7)], dtype=np.int64),
               "referr/logits": np.float64(np.abs(l32 - logits).max()), "referr/hc": np.float64(np.abs(h32 - hc).max())}
        big = max(float(np.abs(grads[k]).max()) for k in AC.KEYS)
        for k in AC.KEYS:
            g = grads[k]
            gm = float(np.abs(g).max())
            out["gmax/" + k] = np.float64(gm)          # rounding noise for attention_net.3.fc2.bias: a softmax ignores a common shift
            out["referr/" + k] = np.float64(np.abs(g32[k] - g).max() / (gm if gm > 1e-9 * big else big))
            out["shape/" + k] = np.array(g.shape)
            if k in AC.BIG:
                np.savez(os.path.join(HERE, f"deepattnmisl_{name}_{AC.BIG[k]}.npz"), grad=g.astype(np.float32))
            else:
                out["grad/" + k] = g.astype(np.float32) if k in AC.ROUNDED else g
        path = os.path.join(HERE, f"deepattnmisl_{name}.npz")
        np.savez(path, **out)
        print(f"{name}: N={N} Kc={Kc} num_cls={num_cls} near-zero {out['near_counts'].tolist()} fp32 mask flips {int(out['ref32_mask_flips'])} "
              f"max referr={max(float(out['referr/' + k]) for k in AC.KEYS):.2e} {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

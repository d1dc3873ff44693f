"""Generate tests/golden/dsmil_<case>.npz (and dsmil_<case>_gq.npz / _gv.npz: the two [256, 512] gradients, whole) from the upstream reference's own DSMIL (model/deepmil.py:692-721) in float64.

Container-only (imports the reference through _ref_import.py).  Per case: logits, attention, critical rows and the parameter
gradients of sum(logits * w), all from the ``.double()`` model on the ``.double()`` input, plus, per gradient tensor, the error of the
reference's own fp32 run against that float64 result relative to the tensor's largest float64 entry (``referr/<key>``) and that
largest entry (``gmax/<key>``).  Inputs and parameters are recipes (dsmil_cases.py).  Asserts that no comparison hinges on an argmax
the reference decides by rounding: per class the two largest instance scores are >= 1e-4 apart."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dsmil_cases as DC  # noqa: E402
from _ref_import import import_reference  # noqa: E402


def build(ref, C, params, feat_proj, dtype):
    m = ref.deepmil.DSMIL(dim_in=512, dim_hid=256, num_cls=C, use_feat_proj=feat_proj, drop_rate=0.25)
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    m.load_state_dict(sd, strict=True)
    return m.to(dtype).eval()


def run(m, x, w, dtype):
    X = torch.from_numpy(x).to(dtype)[None]
    m.zero_grad(set_to_none=True)
    logits, attn = m(X, ret_with_attn=True)
    (logits * torch.from_numpy(w).to(dtype)).sum().backward()
    grads = {k: p.grad.detach().double().numpy() for k, p in m.named_parameters() if k in DC.KEYS}
    with torch.no_grad():
        feats = m.feat_proj(X).squeeze(0) if m.feat_proj is not None else X.squeeze(0)
        scores = m.i_classifier(feats)[1]
    return logits.detach().double().numpy(), attn.detach().double().numpy(), scores.double().numpy(), grads


def main():
    ref = import_reference()
    torch.manual_seed(0)
    for name, (N, C, rows, seed, sharp, fp) in DC.CASES.items():
        x = DC.make_rows(N, rows, seed)
        w = DC.make_w(C, seed)
        q_scale = 1.0
        while True:
            params = DC.make_params(C, seed, fp, q_scale)
            logits, attn, scores, grads = run(build(ref, C, params, fp, torch.float64), x, w, torch.float64)
            if not sharp:
                break
            m64 = build(ref, C, params, fp, torch.float64)      # the largest single attention weight A[n, k]
            with torch.no_grad():
                X = torch.from_numpy(x).double()
                A = m64.b_classifier(X, m64.i_classifier(X)[1])[1]
            if float(A.max()) > 0.05:
                break
            q_scale *= 1.5
        top2 = np.sort(scores, axis=0)[-2:] if N > 1 else None
        gap = float((top2[1] - top2[0]).min()) if N > 1 else float("inf")
        assert gap >= 1e-4, f"{name}: instance-score gap {gap:.2e} < 1e-4, choose another seed"
        l32, a32, _, g32 = run(build(ref, C, params, fp, torch.float32), x, w, torch.float32)
        out = {"logits": logits, "attn": attn.astype(np.float32), "crit": scores.argmax(axis=0).astype(np.int32),
               "q_scale": np.float64(q_scale), "gap": np.float64(gap), "keys": np.array(DC.KEYS),
               "referr/logits": np.float64(np.abs(l32 - logits).max()),
               "referr/attn": np.float64(np.abs(a32 - attn).max() / np.abs(attn).max())}
        for k in DC.KEYS:
            g = grads[k]
            gm = float(np.abs(g).max())
            out["gmax/" + k] = np.float64(gm)
            out["referr/" + k] = np.float64(np.abs(g32[k] - g).max() / max(gm, 1e-300))
            out["shape/" + k] = np.array(g.shape)
            if k in DC.BIG:
                np.savez(os.path.join(HERE, f"dsmil_{name}_{DC.BIG[k]}.npz"), grad=g.astype(np.float32))
            else:
                out["grad/" + k] = g
        path = os.path.join(HERE, f"dsmil_{name}.npz")
        np.savez(path, **out)
        print(f"{name}: N={N} C={C} gap={gap:.2e} q_scale={q_scale:.3g} max attn={float(attn.max()):.3e} "
              f"max referr={max(float(out['referr/' + k]) for k in DC.KEYS):.2e} {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

"""Generate tests/golden/ilra_<case>.npz and ilra_keys.json from the upstream reference's own ILRA (model/deepmil.py:409-535) in float64.

Container-only (imports the reference through _ref_import.py, ``nystrom_attention`` stubbed).  Per case, from the ``.double()`` model:
logits, every block's Z (the per-head attention weights of the reference's own ``nn.MultiheadAttention`` applied to the block's input
rows) and H, the NLP's Z, max|xhat| per block, the gradient digests of sum(logits * w) (ilra_cases.digest), ``referr/*`` (the reference's
own fp32 error), ``sens/drop_last`` (relative change of the logits when the last row is dropped), the smallest |t| over all ReLU
pre-activations (rows and tails), the number of ReLU decisions the reference's fp32 run flips and the largest |t64| among them.

ASSERTED per parity case: referr/logits <= 1e-5 max|logits|; sens/drop_last >= 1e-3 (N > 1); no tail pre-activation within 1e-4 of zero.
A seed that fails is replaced by another seed in ilra_cases.py; the thresholds stay.  The mask band (10 x the largest |t64| of a flipped
decision over all cases, floor 1e-6) is written into ilra_cases.py."""
import contextlib
import io
import json
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ilra_cases as IC  # noqa: E402
from _ref_import import import_reference  # noqa: E402


def build(ref, num_layers, num_cls, params, dtype):
    with contextlib.redirect_stdout(io.StringIO()):
        m = ref.deepmil.ILRA(dim_in=512, dim_hid=256, num_cls=num_cls, num_layers=num_layers)
    if params is not None:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m.to(dtype).eval()


def run(m, x, w, dtype):
    X = torch.from_numpy(x).to(dtype)[None]
    kept, hooks = {"t_rows": [], "t_tail": []}, []

    def pooled(tag):
        def hook(mod, args, out):          # mod: MultiHeadAttention(Q, K); the per-head weights of its own nn.MultiheadAttention on K
            with torch.no_grad():
                Q, K = args
                q = mod.fc_q(Q).transpose(0, 1)
                k, v = mod.fc_k(K).transpose(0, 1), mod.fc_v(K).transpose(0, 1)
                _, a = mod.multihead_attn(q, k, v, need_weights=True, average_attn_weights=False)      # [1, 8, 1, N]
                kept[tag] = (a[0, :, 0, :] @ K[0]).double().numpy()
        return hook
    for i, blk in enumerate(m.gab_blocks):
        hooks.append(blk.project_forward.register_forward_hook(pooled(f"Z{i}")))
        hooks.append(blk.project_forward.register_forward_hook(lambda mod, a, out, i=i: kept.__setitem__(f"H{i}", out.detach()[0, 0].double().numpy())))
        hooks.append(blk.register_forward_hook(lambda mod, a, out, i=i: kept.__setitem__(f"xmax{i}", float(out.detach().abs().max()))))
        hooks.append(blk.project_forward.fc_o.register_forward_hook(lambda mod, a, out: kept["t_tail"].append(out.detach().double().numpy().reshape(-1))))
        hooks.append(blk.project_backward.fc_o.register_forward_hook(lambda mod, a, out: kept["t_rows"].append(out.detach()[0].double().numpy())))
    hooks.append(m.pooling.mha.register_forward_hook(pooled("Zp")))
    hooks.append(m.pooling.mha.fc_o.register_forward_hook(lambda mod, a, out: kept["t_tail"].append(out.detach().double().numpy().reshape(-1))))
    m.zero_grad(set_to_none=True)
    logits = m(X)
    for h in hooks:
        h.remove()
    (logits * torch.from_numpy(w).to(dtype)).sum().backward()
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad).detach().double().numpy() for k, p in m.named_parameters()}
    return logits.detach().double().numpy(), kept, grads


def main():
    ref = import_reference()
    band, keys_json = 0.0, {}
    for name, (N, rows, num_layers, num_cls, seed, recipe) in IC.CASES.items():
        x, params, w = IC.make_case(name)
        m64 = build(ref, num_layers, num_cls, params, torch.float64)
        sd = m64.state_dict()
        assert list(sd) == list(IC.shapes(num_layers, num_cls)), name
        assert all(tuple(sd[k].shape) == sh for k, sh in IC.shapes(num_layers, num_cls).items()), name
        keys_json[f"{num_layers}/{num_cls}"] = [[k, list(v.shape)] for k, v in sd.items()]          # in the reference's order
        logits, kept, grads = run(m64, x, w, torch.float64)
        l32, k32, g32 = run(build(ref, num_layers, num_cls, params, torch.float32), x, w, torch.float32)
        lmax = float(np.abs(logits).max())
        out = {"logits": logits, "referr/logits": np.float64(np.abs(l32 - logits).max()), "keys": np.array(list(sd))}
        flips, flip_max, tmin = 0, 0.0, np.inf
        for i in range(num_layers):
            out[f"Z{i}"], out[f"H{i}"], out[f"xmax{i}"] = kept[f"Z{i}"], kept[f"H{i}"], np.float64(kept[f"xmax{i}"])
            out[f"referr/Z{i}"] = np.float64(np.abs(k32[f"Z{i}"] - kept[f"Z{i}"]).max() / np.abs(kept[f"Z{i}"]).max())
            t64, t32 = kept["t_rows"][i], k32["t_rows"][i]
            f = (t64 > 0) != (t32 > 0)
            flips += int(f.sum())
            flip_max = max(flip_max, float(np.abs(t64[f]).max()) if f.any() else 0.0)
            tmin = min(tmin, float(np.abs(t64).min()))
        out["Zp"] = kept["Zp"]
        tail_min = min(float(np.abs(t).min()) for t in kept["t_tail"])
        out["relu/min_abs_rows"], out["relu/min_abs_tail"] = np.float64(tmin), np.float64(tail_min)
        out["relu/ref32_flips"], out["relu/ref32_flip_max"] = np.int64(flips), np.float64(flip_max)
        if N > 1:
            l_drop, _, _ = run(m64, x[:-1], w, torch.float64)
            out["sens/drop_last"] = np.float64(np.abs(l_drop - logits).max() / lmax)
        gbig = max(float(np.abs(g).max()) for g in grads.values())
        for k, g in grads.items():
            for part, v in IC.digest(k, g, seed).items():
                out[f"dg/{k}/{part}"] = v
            gm = float(np.abs(g).max())
            out[f"referr/dg/{k}"] = np.float64(np.abs(g32[k] - g).max() / (gm if gm > 1e-9 * gbig else gbig))
        if recipe == "live":
            assert float(out["referr/logits"]) <= 1e-5 * lmax, (name, "referr", float(out["referr/logits"]), lmax)
            assert N == 1 or float(out["sens/drop_last"]) >= 1e-3, (name, "sens", float(out["sens/drop_last"]))
            assert tail_min >= 1e-4, (name, "tail pre-activation near zero", tail_min)
            band = max(band, flip_max)
        path = os.path.join(HERE, f"ilra_{name}.npz")
        np.savez(path, **out)
        print(f"{name}: N={N} L={num_layers} C={num_cls} max|logit| {lmax:.3f} referr {float(out['referr/logits']):.1e} "
              f"sens {float(out.get('sens/drop_last', np.nan)):.1e} tail min|t| {tail_min:.1e} rows min|t| {tmin:.1e} "
              f"fp32 flips {flips} (largest |t64| {flip_max:.1e}) max grad referr "
              f"{max(float(out['referr/dg/' + k]) for k in grads):.1e} {os.path.getsize(path)} bytes")
    with open(os.path.join(HERE, "ilra_keys.json"), "w") as f:
        json.dump(keys_json, f, indent=0)
    band = max(10.0 * band, 1e-6)
    src = open(os.path.join(HERE, "ilra_cases.py")).read()
    src = re.sub(r"^BAND = \S+", f"BAND = {band:.3g}", src, count=1, flags=re.M)
    open(os.path.join(HERE, "ilra_cases.py"), "w").write(src)
    print(f"mask band {band:.3g}")


if __name__ == "__main__":
    main()

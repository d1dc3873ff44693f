"""Host time of the drop-in model's cache keys in steady state, on the CPU (no device needed): ``_provider_key()``, ``_text_features()``,
``_same_state(s0, _eval_state(T))`` and ``_defer_key()`` of a ``VLSA`` whose provider has about 120 tensors (a 12-block stub tower plus
a learner) and whose MIL encoder is a VLFAN.  These run once per ``net(X)`` in loops that are host-bound.

    python tools/bench_state_keys.py [--number 20000] [--repeat 7]

prints one JSON line: microseconds per call (best of ``repeat`` runs of ``number`` calls each)."""
import argparse
import json
import os
import sys
import timeit

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402


class Learner(nn.Module):
    def __init__(self):
        super().__init__()
        self.context_embeds = nn.Parameter(torch.randn(4, 6, 16))
        self.register_buffer("pseudo_sentence_tokens", torch.ones(4, 6, dtype=torch.long), persistent=False)

    def forward(self):
        return self.context_embeds


class Block(nn.Module):
    """10 tensors, as a transformer block of the text tower carries them (two norms, fused qkv, out projection, two bias-free MLP layers)"""

    def __init__(self, w=16):
        super().__init__()
        self.ln_1, self.qkv, self.out_proj = nn.LayerNorm(w), nn.Linear(w, 3 * w), nn.Linear(w, w)
        self.ln_2, self.fc, self.proj, self.drop = nn.LayerNorm(w), nn.Linear(w, 4 * w, bias=False), nn.Linear(4 * w, w, bias=False), nn.Dropout(0.1)

    def forward(self, x):
        x = x + self.out_proj(self.qkv(self.ln_1(x))[..., :x.shape[-1]])
        return x + self.drop(self.proj(self.fc(self.ln_2(x))))


class Tower(nn.Module):
    def __init__(self):
        super().__init__()
        self.blocks = nn.ModuleList([Block() for _ in range(12)])
        self.head = nn.Linear(16, 512)

    def forward(self, prompts_embedding, prompts_pseudo_tokens, **kw):
        x = prompts_embedding
        for b in self.blocks:
            x = b(x)
        return self.head(x.mean(dim=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--number", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=7)
    args = ap.parse_args()
    from vlsa_amd.vlsa import VLSA
    torch.manual_seed(0)
    cfg = dict(name="VLFAN", dim_in=512, use_feat_proj=False, query="Parameter", num_query=4, query_pooling="mean")
    net = VLSA.from_modules(cfg, prompt_learner=Learner(), prompt_encoder=Tower()).eval()
    n_tensors = sum(1 for _ in net.prompt_learner.parameters()) + sum(1 for _ in net.prompt_learner.buffers()) \
        + sum(1 for _ in net.prompt_encoder.parameters())
    with torch.no_grad():
        T = net._text_features()
        s0 = net._eval_state(T)
        assert net._text_features() is T and net._same_state(s0, net._eval_state(T)) and net._defer_key() == net._defer_key()
        legs = {"provider_key": net._provider_key, "text_features": net._text_features,
                "same_state": lambda: net._same_state(s0, net._eval_state(T)), "defer_key": net._defer_key}
        out = {"provider_tensors": n_tensors}
        for name, fn in legs.items():
            out[name + "_us"] = round(min(timeit.repeat(fn, number=args.number, repeat=args.repeat)) / args.number * 1e6, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
